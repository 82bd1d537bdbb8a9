"""The two kernel forms of csrc/aa_sketch_kernel.hip behind skl_sketch_signs_aa -- aahash_binmin_lds_kernel with the bin
minima in LDS (up to 4 096 bins) and in global memory (more), and the unstaged aahash_binmin_kernel -- on the inputs of
tests/aa_edge_cases.py, in which the windows at a thread's first and last start, past a workgroup's chunk, next to a
separator and at the end of a sample each decide a bin of the output.  The expectation is aa_edge_cases.window_table (a
non-rolling hash, tied to the restated iterator by tests/test_aa_edge_cases_cpu.py) reduced to bin minima; equality as u64
is the only assertion on outputs, and a mismatch is reported by the named starts whose bins differ (start s of the staged
kernel is thread (s / 64) % 256 of chunk s / 16 384, its window j = s % 64).

Before any GPU call each case's conditions are asserted from the expectation alone (Case.check, check_wide).  Every
staged case is run four times in its call, its first residue at byte offset 0, 1, 2 and 3 mod 4 of the call's residues:
the staged kernel reads whole dwords and realigns.

Not covered: k = 1 (20 signs) is plain equality."""
import numpy as np
import pytest

import aa_edge_cases as E

pytestmark = pytest.mark.gpu
IN_LDS = "seed and roll tables and bin minima in LDS"
IN_GLOBAL = "seed and roll tables in LDS, 64 window starts per thread, bin minima in global memory"
STAGED, UNSTAGED = "aahash_binmin_lds_kernel", "aahash_binmin_kernel"
FORM_OF_BINS = {4096: IN_LDS, 4097: IN_GLOBAL}


def call(skl, ctx, cases, kmers, num_bins):
    """One call over the samples of `cases` (one level, one end-rule setting) -> [n_samples, nk, num_bins]."""
    codes, res_begin = E.pack(cases)
    assert len(cases) * len(kmers) * num_bins * 8 <= 256 << 20      # one batch: byte offsets in the call are byte offsets on the device
    return skl.sketch_signs_aa(ctx, codes, res_begin, kmers, num_bins, cases[0].level, cases[0].end_rule)


def differing_named_starts(case, got, num_bins, span):
    exp = case.expectation(num_bins)
    bs = np.uint64(E.bin_size_of(num_bins))
    first = int(np.flatnonzero(got != exp)[0])
    out = [f"first differing bin {first}: holds {int(got[first])}, not {int(exp[first])}"]
    for s in case.valid:
        b = int(case.would_be_sign(s) // bs)
        if got[b] != exp[b]:
            out.append(f"valid start {s} (span {s // span}, j {s % span}): bin {b} holds {int(got[b])}, not {int(exp[b])}")
    for s in case.invalid:
        w = case.would_be_sign(s)
        if got[int(w // bs)] == w:
            out.append(f"invalid start {s} (span {s // span}, j {s % span}) was hashed into bin {int(w // bs)}")
    return out


def assert_equal(got, cases, num_bins, span):
    """got [n_samples, num_bins] against the expectation of each case, exactly."""
    assert got.shape == (len(cases), num_bins) and got.dtype == np.uint64
    for s, c in enumerate(cases):
        exp = c.expectation(num_bins)
        if not np.array_equal(got[s], exp):
            raise AssertionError(f"sample {s} ({c.name}), k = {c.k}, level {c.level}, end rule {c.end_rule}, {num_bins} bins: "
                                 f"{int((got[s] != exp).sum())} bins differ; " + "; ".join(differing_named_starts(c, got[s], num_bins, span)))


def run_staged(skl, ctx, cases, bins=E.LDS_BINS, fillers_unstaged=False):
    """The cases four times each, at every byte offset mod 4, at 4 096 bins (minima in LDS) and 4 097 (in global memory)."""
    for nb in bins:
        for c in cases:
            c.check(nb)
    every, at = E.misaligned(cases)
    _, res_begin = E.pack(every)
    assert [int(res_begin[i]) % 4 for i in at] == [0, 1, 2, 3] * len(cases)
    assert np.array_equal(skl.aa_codes(cases[0].seq), cases[0].codes)
    for nb in bins:
        got = call(skl, ctx, every, [cases[0].k], nb)
        name = ctx.last_kernel()
        assert STAGED in name and FORM_OF_BINS[nb] in name and ((UNSTAGED + " (") in name) == fillers_unstaged, name
        assert_equal(got[:, 0], every, nb, E.SPAN)


def run_unstaged(skl, ctx, cases, kmers, groups):
    """One call at the k-mer lengths `kmers`; groups[i]: the cases (the same samples) of kmers[i]."""
    span = E.short_span(max(kmers))
    for nb in E.UNSTAGED_BINS:
        for group in groups:
            for c in group:
                c.check(nb)
        got = call(skl, ctx, cases, kmers, nb)
        assert STAGED not in ctx.last_kernel() and UNSTAGED in ctx.last_kernel()
        for i, group in enumerate(groups):
            assert [c.seq for c in group] == [c.seq for c in cases] and all(c.k == kmers[i] for c in group)
            assert_equal(got[:, i], group, nb, span)


def test_shapes_are_the_ones_the_cases_assume(skl):
    shape = skl.sketch_aa_shape()
    assert (shape["span_lds"], shape["wg_lds"], shape["k_staged_max"], shape["lds_bins_max"], shape["long_min"], shape["wg_short"]) == \
        (E.SPAN, E.WG_LDS, E.K_STAGED_MAX, E.LDS_BINS_MAX, E.LONG_MIN, E.WG_SHORT)
    assert E.CHUNK == shape["span_lds"] * shape["wg_lds"] == 16384
    for kmax in (1, 2, 5, 16, 17, 20, 40, 64, 255, 256, 257, 300):
        assert shape["short_span"](kmax) == E.short_span(kmax)


@pytest.mark.parametrize("k", E.STAGED_THREAD_KS)
def test_staged_thread_boundary(skl, gpu_ctx, set_switch, k):
    """Samples of 232 + k residues around the boundary p = 128 between two threads of the staged kernel: no separator,
    one at p - 1, p, p + 1 (the thread's first window holds it, after which its one seed must roll on exactly), at p - k,
    p + k - 2, p + k - 1, p + k (which the boundary windows just hold or just clear)."""
    set_switch("SKL_AA_LONG_MIN", 1)
    run_staged(skl, gpu_ctx, E.staged_thread_boundary(k))


def test_k1_on_the_thread_boundary_samples(skl, gpu_ctx, set_switch):
    set_switch("SKL_AA_LONG_MIN", 1)
    cases = E.k1_samples()
    for nb in (64,) + E.LDS_BINS:
        got = call(skl, gpu_ctx, cases, [1], nb)
        assert STAGED in gpu_ctx.last_kernel()
        assert_equal(got[:, 0], cases, nb, E.SPAN)


@pytest.mark.parametrize("form", ["as_planned", "all_staged"])
@pytest.mark.parametrize("k", E.CHUNK_KS)
def test_staged_chunk_boundary(skl, gpu_ctx, set_switch, k, form):
    """Samples of 16 384 + 73 + k residues around the boundary p = 16 384 between two workgroups: the windows of the last
    thread of chunk 0 read up to k - 1 residues past the chunk; at k = 253 .. 256 from the last staged dwords, at each of
    the four byte lags.  At k = 5 and 256 also a sample of three chunks with named starts at both boundaries."""
    if form == "all_staged":
        set_switch("SKL_AA_LONG_MIN", 1)
    cases = E.chunk_boundary(k) + ([E.two_chunk_boundaries(k)] if k in E.TWO_CHUNK_KS else [])
    run_staged(skl, gpu_ctx, cases, fillers_unstaged=form == "as_planned")


@pytest.mark.parametrize("place", E.END_PLACES)
@pytest.mark.parametrize("k", E.END_KS)
def test_sample_end(skl, gpu_ctx, set_switch, k, place):
    """Lengths m span + k - 1 + {0, 1, 2} -- the sample's last window is a thread's last, first or second window -- with the
    residue before that window valid and a separator, under both end-rule settings: two threads of the staged kernel,
    a whole chunk (the last window alone in a second workgroup), two threads of the unstaged kernel."""
    for end_rule in (False, True):
        cases = E.sample_ends(place, k, end_rule)
        if place == "unstaged2":
            run_unstaged(skl, gpu_ctx, cases, [k], [cases])
        else:
            set_switch("SKL_AA_LONG_MIN", 1)
            run_staged(skl, gpu_ctx, cases)


@pytest.mark.parametrize("k", E.UNSTAGED_KS)
def test_unstaged_thread_boundary(skl, gpu_ctx, k):
    """The same patterns around p = 2 span of the unstaged kernel, span = short_span(k): 16 to 256, capped there for
    k = 257 and 300, where a window is longer than a span."""
    cases = E.unstaged_thread_boundary(k)
    run_unstaged(skl, gpu_ctx, cases, [k], [cases])


@pytest.mark.parametrize("k,kmax", E.TWO_K_CALLS)
def test_unstaged_thread_boundary_at_the_span_of_a_longer_k(skl, gpu_ctx, k, kmax):
    """Two k-mer lengths in one call: the span follows the longer, so k = 3 runs at 48 starts per thread and k = 5 at 256.
    Named starts at the shorter k; the longer k of the same samples is compared for plain equality."""
    cases = E.unstaged_thread_boundary(k, kmax)
    run_unstaged(skl, gpu_ctx, cases, [k, kmax], [cases, E.companions(cases, kmax)])
    run_unstaged(skl, gpu_ctx, cases, [kmax, k], [E.companions(cases, kmax), cases])


def test_unstaged_samples_packed_across_a_workgroup_boundary(skl, gpu_ctx):
    """Samples of three spans behind fillers of 255 threads: each is the last thread of one workgroup and the first two of
    the next."""
    cases, at = E.packed_samples()
    span = skl.sketch_aa_shape()["short_span"](E.PACK_K)
    threads = np.cumsum([0] + [-(-len(c.seq) // span) for c in cases])
    assert all(threads[i] % E.WG_SHORT == E.WG_SHORT - 1 and threads[i + 1] - threads[i] == 3 for i in at)
    run_unstaged(skl, gpu_ctx, cases, [E.PACK_K], [cases])


@pytest.mark.parametrize("level", [2, 3])
def test_levels(skl, gpu_ctx, level):
    """A chunk-boundary sample at levels 2 and 3 (letters of a group share a seed)."""
    run_staged(skl, gpu_ctx, E.level_case(level), fillers_unstaged=True)


@pytest.mark.parametrize("k", E.WIDE_KS)
def test_wide_bins(skl, gpu_ctx, k):
    """A random protein of 40 000 residues (three chunks) with 40 separators at 2^20 bins, where at least 90 % of ALL
    windows decide a bin: the staged kernel with the minima in global memory."""
    case = E.wide_case(k)
    E.check_wide(case)
    got = call(skl, gpu_ctx, [case], [k], E.WIDE)[0, 0]
    assert STAGED in gpu_ctx.last_kernel() and IN_GLOBAL in gpu_ctx.last_kernel()
    exp = case.expectation(E.WIDE)
    if not np.array_equal(got, exp):
        starts, signs = case.table
        bins = (signs // np.uint64(E.bin_size_of(E.WIDE))).astype(np.int64)
        bad = starts[got[bins] != exp[bins]]
        raise AssertionError(f"k = {k}: {int((got != exp).sum())} bins differ; first windows whose bins differ: {bad[:20].tolist()}")
