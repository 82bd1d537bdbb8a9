"""The sensitivity of tests/test_gpu_sketch_edges.py, checked without a GPU: every case of tests/sketch_edge_cases.py
is built, the conditions of that module hold at every bin count the case is run at, and the expectation really changes
when one named valid start is removed or one named invalid start is admitted."""
import numpy as np
import pytest

import reads_reference as R
import sketch_edge_cases as E

GROUPS = E.groups()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_named_starts_decide_their_bins(group):
    bins, make = GROUPS[group]
    cases = make()
    assert cases and all(c.k == cases[0].k and c.rc == cases[0].rc for c in cases)
    n_valid = n_invalid = 0
    for c in cases:
        if not c.valid and not c.invalid:
            assert len(c.codes) < c.k, c.name      # only a sample without any window has no named start
            assert c.table[0].size == 0
            continue
        for nb in bins:
            c.check(nb)
            exp = c.expectation(nb)
            for s in c.valid:
                assert not np.array_equal(c.expectation(nb, drop=s), exp), (c.name, nb, s)
            for s in c.invalid:
                assert not np.array_equal(c.expectation(nb, admit=s), exp), (c.name, nb, s)
        n_valid += len(c.valid)
        n_invalid += len(c.invalid)
        assert bool(c.invalid) == c.has_inner_break, c.name
    assert n_valid >= 1
    if "boundary" in group or "lastthread" in group:
        assert n_invalid >= 6      # the six break positions, the two runs of Ns


@pytest.mark.parametrize("k,rc", E.WIDE_K_RC)
def test_wide_bins_nearly_every_window_decides(k, rc):
    case = E.wide_case(k, rc)
    E.check_wide(case)
    starts, signs = case.table
    exp = case.expectation(E.WIDE)
    single = case.single_holders(E.WIDE)
    for i in (0, int(np.flatnonzero(single)[len(starts) // 3]), int(np.flatnonzero(single)[-1])):
        if single[i]:
            assert not np.array_equal(case.expectation(E.WIDE, drop=int(starts[i])), exp)


def test_thread_boundary_samples_are_the_ones_described():
    """The six break positions on both sides of `s < b < s + k`, the runs of Ns, the null and the trivial offsets."""
    k, p = 31, 128
    cases = E.thread_boundary(k, True)
    offs = [c.offsets.tolist() for c in cases]
    assert offs[:6] == [[p - 1], [p], [p + 1], [p + k - 1], [p + k], [p + k + 1]]
    assert offs[6:] == [[p] * 40, [p + 5] * 40, [0], [], [3000]]
    by = {c.name.split(":")[1]: c for c in cases}
    assert p in by["break@p+0"].valid and p - 1 in by["break@p+0"].invalid and p - k in by["break@p+0"].valid
    assert p in by["break@p+1"].invalid and p + 1 in by["break@p+1"].valid        # the thread's first window spans the break
    assert p in by["break@p+k-1"].invalid and p + k - 1 in by["break@p+k-1"].valid
    assert p in by["break@p+k+0"].valid and p + 1 in by["break@p+k+0"].invalid    # it just clears the break
    assert p - 1 in by["break@p-1"].valid and p - 2 in by["break@p-1"].invalid
    assert by["no offsets"].invalid == [] and by["offset@0"].valid[0] == 0 and by["offset@len"].valid[-1] == 3000 - k
    last = E.last_thread(129, True)
    assert all(len(c.codes) == 65536 + 300 for c in last) and last[1].offsets.tolist() == [65536 - 128]


def test_sample_end_lengths_are_the_ones_described():
    k = 129
    cases = E.sample_ends(k, True)
    lengths = [len(c.codes) for c in cases]
    assert lengths == [65535, 65536, 65537, 65536 + k - 2, 65536 + k - 1, 65536 + k, 65664, 65665, 131073]
    for c, n in zip(cases, lengths):
        starts = c.table[0]
        assert starts.size == n - k + 1 and c.valid[-1] == n - k
        assert (65536 in c.valid) == (n >= 65536 + k) and (65535 in c.valid) == (n >= 65535 + k)
    # the second workgroup: codes but no window up to 65 536 + k - 1 bases, exactly one window at 65 536 + k
    assert [int((c.table[0] >= 65536).sum()) for c in cases[3:6]] == [0, 0, 1]


def test_small_k_cannot_meet_the_conditions():
    """At most 4^k / 2 canonical signs (and the palindromes): of some 3 000 windows at most that many can be alone in
    their bins, at k = 1 none."""
    for k in (1, 2, 3):
        for c in E.small_k_samples(k, True):
            distinct = np.unique(c.table[1]).size
            assert distinct <= 4 ** k // 2 + 2 ** k     # (palindromes are their own reverse complements)
            assert c.table[0].size > 2900 and int(c.single_holders(4096).sum()) <= (0 if k == 1 else distinct)


def test_expectation_is_the_window_table_reduced():
    codes, offsets = E.bins_sample()
    c = E.plain_case(codes, offsets, 21, True)
    starts, signs = R.window_table(codes, offsets, 21, True)
    for nb in (1, 1000, 4097):
        exp = c.expectation(nb)
        bs = -(-R.SIGN_MOD // nb)
        for b in np.unique(signs // np.uint64(bs)).tolist()[:50]:
            assert exp[b] == signs[signs // np.uint64(bs) == np.uint64(b)].min()
        assert int((exp != E.U64_MAX).sum()) == np.unique(signs // np.uint64(bs)).size
