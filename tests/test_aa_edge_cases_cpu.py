"""The sensitivity of tests/test_gpu_sketch_aa_edges.py, checked without a GPU: every case of tests/aa_edge_cases.py is
built, its non-rolling expectation equals the restated iterator of tests/aa_reference.py at every bin count the case is
run at, the conditions of that module hold, and the expectation really changes when one named valid start is removed or
one named invalid start is admitted.  The sample-end group and one k of the two thread-boundary groups also go through
the host sketcher (csrc/host/aahash.cpp behind tests/native/aa_check.cpp)."""
import subprocess

import numpy as np
import pytest

import aa_edge_cases as E
import aa_native
import aa_reference as R

GROUPS = E.groups()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_named_starts_decide_their_bins(group):
    bins, make = GROUPS[group]
    cases = make()
    assert cases and all(c.k == cases[0].k and c.level == cases[0].level and c.end_rule == cases[0].end_rule for c in cases)
    n_valid = n_invalid = 0
    for c in cases:
        starts, signs = E.window_table(c.seq, c.k, c.level)
        if not c.end_rule:
            assert np.array_equal(starts, c.table[0]) and np.array_equal(signs, c.table[1])
        for nb in bins:
            exp = c.expectation(nb)
            natural = R.natural_signs(c.seq, c.k, nb, c.level)
            assert np.array_equal(E.reduce_to_bins(signs, nb), natural), (c.name, nb)
            assert np.array_equal(exp, R.signs_or_max(c.seq, c.k, nb, c.level) if c.end_rule else natural), (c.name, nb)
            c.check(nb)
            for s in c.valid:
                assert not np.array_equal(c.expectation(nb, drop=s), exp), (c.name, nb, s)
            for s in c.invalid:
                assert not np.array_equal(c.expectation(nb, admit=s), exp), (c.name, nb, s)
        n_valid += len(c.valid)
        n_invalid += len(c.invalid)
        assert bool(c.invalid) == bool(c.breaks.size or c.ruled_out), c.name
    assert n_valid >= 1
    if group.startswith(("thread", "chunk-", "uthread")):
        assert n_invalid >= 6      # every pattern but "none" names the starts its separator breaks


@pytest.mark.parametrize("k", E.WIDE_KS)
def test_wide_bins_nearly_every_window_decides(k):
    case = E.wide_case(k)
    assert len(case.seq) == 40000 and case.breaks.size == 40
    E.check_wide(case)
    starts, signs = case.table
    exp = case.expectation(E.WIDE)
    assert np.array_equal(exp, R.natural_signs(case.seq, k, E.WIDE))
    single = np.flatnonzero(case.single_holders(E.WIDE))
    for i in (int(single[0]), int(single[len(single) // 3]), int(single[-1])):
        assert not np.array_equal(case.expectation(E.WIDE, drop=int(starts[i])), exp)


def test_break_patterns_are_the_ones_described():
    """B(p, k): none, {p - 1}, {p}, {p + 1}, {p - k}, {p + k - 2}, {p + k - 1}, {p + k}, on both sides of s <= o < s + k."""
    p, k = 128, 7
    assert list(E.break_patterns(p, k).values()) == [[], [p - 1], [p], [p + 1], [p - k], [p + k - 2], [p + k - 1], [p + k]]
    assert list(E.break_patterns(p, 2).values()) == [[], [127], [128], [129], [126], [130]]      # p + k - 2 = p, p + k - 1 = p + 1
    cases = E.staged_thread_boundary(k)
    assert [c.breaks.tolist() for c in cases] == list(E.break_patterns(p, k).values())
    assert all(len(c.seq) == 192 + k + 40 for c in cases)
    by = {c.name.split(":")[1]: c for c in cases}
    assert by["none"].invalid == [] and by["none"].valid == [p - k, p - k + 1, p - 1, p, p + 1]
    assert p - 1 in by["p-1"].invalid and p in by["p-1"].valid and p - k - 1 in by["p-1"].valid     # o = p - 1: s = p - k .. p - 1 broken
    assert p in by["p"].invalid and p - k + 1 in by["p"].invalid and p + 1 in by["p"].valid and p - k in by["p"].valid
    assert p in by["p+1"].invalid and p + 1 in by["p+1"].invalid and p - k + 1 in by["p+1"].valid
    assert p - k in by["p-k"].invalid and p - k + 1 in by["p-k"].valid
    assert p - 1 in by["p+k-2"].invalid and p in by["p+k-2"].invalid and p - k + 1 in by["p+k-2"].valid      # the last residue start p - 1 reads
    assert p - 1 in by["p+k-1"].valid and p in by["p+k-1"].invalid                                            # the first it does not read
    assert p in by["p+k"].valid and p + 1 in by["p+k"].invalid


def test_chunk_boundary_samples_are_the_ones_described():
    p = 16384
    assert (E.SPAN, E.CHUNK, E.K_STAGED_MAX, E.LDS_BINS, E.LONG_MIN) == (64, p, 256, (4096, 4097), 8192)
    assert E.CHUNK_KS == (2, 5, 64, 253, 254, 255, 256) and E.STAGED_THREAD_KS == (2, 5, 7, 8, 64, 65, 256)
    for k in (5, 256):
        cases = E.chunk_boundary(k)
        assert [c.breaks.tolist() for c in cases] == [[], [p - 1], [p], [p + 1], [p - k], [p + k - 2], [p + k - 1], [p + k]]
        assert all(len(c.seq) == p + 64 + k + 9 for c in cases)
        assert all(p - 1 in c.valid + c.invalid and p in c.valid + c.invalid for c in cases)
        two = E.two_chunk_boundaries(k)
        assert len(two.seq) == 2 * p + 100 and two.breaks.size == 0
        assert p - 1 in two.valid and p in two.valid and 2 * p - k in two.valid
        assert (2 * p in two.valid) == (2 * p + k <= len(two.seq))
    for level in (2, 3):
        (c,) = E.level_case(level)
        assert c.level == level and c.k == 5 and c.breaks.tolist() == [p + 3]


def test_sample_end_lengths_are_the_ones_described():
    assert E.END_KS == (3, 5, 20, 64)
    assert [E.short_span(k) for k in (1, 3, 5, 16, 17, 20, 40, 64, 256, 257, 300)] == [16, 16, 16, 16, 32, 32, 48, 64, 256, 256, 256]
    for place, span_of, m in (("staged2", lambda k: 64, 2), ("chunk", lambda k: 64, 256), ("unstaged2", E.short_span, 2)):
        for k in E.END_KS:
            want = [m * span_of(k) + k - 1 + d for d in (0, 1, 2)]
            for end_rule in (False, True):
                cases = E.sample_ends(place, k, end_rule)
                assert [len(c.seq) for c in cases] == [n for n in want for _ in (0, 1)]
                for c, sep in zip(cases, [False, True] * 3):
                    n = len(c.seq)
                    assert c.breaks.tolist() == ([n - k - 1] if sep else []) and c.end_rule == end_rule
                    # the last window: there unless the end rule finds a separator before it
                    assert (n - k in c.valid) == (not (sep and end_rule)) and (n - k in c.invalid) == (sep and end_rule)
                    assert (n - k - 1 in c.invalid) == sep and c.table[0].size == n - k + 1 - (k + int(end_rule) if sep else 0)
                # number of windows of the last thread: span, 1, 2
                assert [(len(c.seq) - k) % span_of(k) + 1 for c in cases[::2]] == [span_of(k), 1, 2]


def test_unstaged_samples_are_the_ones_described():
    assert E.UNSTAGED_KS == (2, 5, 16, 17, 64, 257, 300) and E.TWO_K_CALLS == ((3, 40), (5, 300))
    for k, kmax, span in ((5, None, 16), (257, None, 256), (3, 40, 48), (5, 300, 256)):
        p = 2 * span
        cases = E.unstaged_thread_boundary(k, kmax)
        assert [c.breaks.tolist() for c in cases] == list(E.break_patterns(p, k).values())
        assert all(len(c.seq) == 3 * span + (kmax or k) + 40 and c.k == k for c in cases)
    cases, at = E.packed_samples()
    span = E.short_span(E.PACK_K)
    threads = np.cumsum([0] + [-(-len(c.seq) // span) for c in cases])
    assert span == 16 and len(at) == 16
    assert all(threads[i] % 256 == 255 and len(cases[i].seq) == 3 * span for i in at)      # spans in threads 255 | 0, 1 of two workgroups
    assert [cases[i].breaks.tolist() for i in at] == [pos for p in (16, 32) for pos in E.break_patterns(p, 5).values()]
    assert all(16 in cases[i].valid + cases[i].invalid and 32 in cases[i].valid + cases[i].invalid for i in at)


def test_misaligned_copies_start_at_every_byte_offset():
    cases, at = E.misaligned(E.staged_thread_boundary(7))
    _, res_begin = E.pack(cases)
    assert [int(res_begin[i]) % 4 for i in at] == [0, 1, 2, 3] * 8
    assert all(cases[i].named and not cases[i - 1].named for i in at)


def test_k1_cannot_meet_the_conditions():
    """20 signs: of some 240 windows at most 20 can be alone in their bins (a letter that occurs once)."""
    for c in E.k1_samples():
        assert np.unique(c.table[1]).size <= 20 and c.table[0].size > 200 and int(c.single_holders(4096).sum()) <= 20
        assert np.array_equal(c.expectation(4096), R.natural_signs(c.seq, 1, 4096))


def test_hash_is_the_restated_iterator_at_every_k():
    """window_table reduced to bins equals natural_signs at k = 1 .. 256 and two k past it, all three levels."""
    rng = np.random.default_rng(31)
    seq = bytearray(E.random_letters(rng, 700).tobytes())
    for o in (0, 130, 131, 420, 699):
        seq[o] = E.SEP
    seq = bytes(seq)
    for k in list(range(1, 257)) + [257, 300]:
        for level in ((1, 2, 3) if k in (1, 2, 5, 31, 33, 256) else (1,)):
            starts, signs = E.window_table(seq, k, level)
            assert np.array_equal(E.reduce_to_bins(signs, 4097), R.natural_signs(seq, k, 4097, level)), (k, level)


# ---- the host sketcher ------------------------------------------------------------------------------------------------------

def host_signs(tmp_path, case, num_bins):
    """aa_check signs on a one-record FASTA file of the case: concat 0 appends a separator to the record (every window:
    the natural rule), concat 1 takes the record as it is (the end rule)."""
    path = tmp_path / "case.fa"
    path.write_bytes(b">case\n" + case.seq + b"\n")
    row = subprocess.check_output([aa_native.build(), "signs", str(case.level), str(case.k), str(num_bins), str(int(case.end_rule)),
                                   str(path)], text=True).splitlines()
    assert len(row) == 1
    _, length, invalid, signs = row[0].split("\t")
    assert int(length) == len(case.seq) + (0 if case.end_rule else 1) and int(invalid) == case.breaks.size
    if signs == "none":
        return np.full(num_bins, E.U64_MAX, dtype=np.uint64)
    return np.array([int(x) for x in signs.split(",")], dtype=np.uint64)


HOST_GROUPS = [g for g in sorted(GROUPS) if g.startswith("end-")] + ["thread-k7", "uthread-k17"]


@pytest.mark.parametrize("group", HOST_GROUPS)
def test_host_sketcher_on_the_same_cases(tmp_path, group):
    bins, make = GROUPS[group]
    for c in make():
        for nb in bins:
            got = host_signs(tmp_path, c, nb)
            exp = c.expectation(nb)
            assert np.array_equal(got, exp), (c.name, c.k, c.end_rule, nb, np.flatnonzero(got != exp)[:4].tolist())
