"""The three kernel forms of csrc/sketch_kernel.hip behind skl_sketch_signs / skl_sketch_signs_packed -- the unstaged
nthash_binmin_kernel, nthash_binmin_lds_kernel with the bin minima in LDS (up to 4096 bins) and in global memory (more)
-- on the inputs of tests/sketch_edge_cases.py, in which the windows at a thread's first and last start, in the
workgroup's look-ahead row, next to a break and at the end of a sample each decide a bin of the output.  The
expectation is reads_reference.window_table reduced to bin minima; equality is the only assertion on outputs, and a
mismatch is reported by the named starts whose bins differ (start s of the staged kernel is thread (s / 128) % 512 of
workgroup s / 65 536, its window j = s % 128).

Before any GPU call each case's conditions are asserted from the reference alone (Case.check, check_wide: every named
valid start is the single holder of its bin's minimum, every named invalid start would lower its bin);
tests/test_sketch_edge_cases_cpu.py does the same, and shows that the expectation moves with each named start, on a
machine without a GPU.

Not covered (see sketch_edge_cases.py): k = 1, 2, 3 and the bin counts are plain equality; the `++bin` branch of the
bin correction (the reciprocal estimate below the true bin) needs a sign within about 2^-20 of a bin's upper edge in
relative terms, which no input of this size produces -- dropping that branch fails no case here.  That branch is pinned on
the CPU instead: csrc/nthash.hpp bin_of, which the kernels call or spell out, at every bin edge
(tests/test_sketch_plan_cpu.py), where the upload batch rule restated in host_batches below is checked too
(csrc/sketch_plan.hpp sketch_upload_batches)."""
import numpy as np
import pytest

import sketch_edge_cases as E

pytestmark = pytest.mark.gpu
U64_MAX = E.U64_MAX
IN_LDS, IN_GLOBAL, UNSTAGED = "bin minima in LDS)", "bin minima in global memory)", "skl::nthash_binmin_kernel ("
FORM_OF_BINS = {4096: IN_LDS, 4097: IN_GLOBAL}


def call(skl, ctx, cases, num_bins, packed=False):
    """One call over the samples of `cases` (one k, one strand setting) -> [n_samples, num_bins]."""
    k, rc = cases[0].k, cases[0].rc
    codes, cb, offs, ob = E.pack(cases)
    if packed:
        got = skl.sketch_signs_packed(ctx, skl.pack_codes(codes, cb), cb, offs, ob, [k], num_bins, rc)
    else:
        got = skl.sketch_signs(ctx, codes, cb, offs, ob, [k], num_bins, rc)
    return got[:, 0]


def differing_named_starts(case, got, num_bins):
    exp = case.expectation(num_bins)
    bs = np.uint64(E.bin_size_of(num_bins))
    starts, signs = case.table
    out = []
    for s in case.valid:
        b = int(signs[np.searchsorted(starts, s)] // bs)
        if got[b] != exp[b]:
            out.append(f"valid start {s} (span {s // E.SPAN}, j {s % E.SPAN}): bin {b} holds {int(got[b])}, not {int(exp[b])}")
    for s in case.invalid:
        w = case.would_be_sign(s)
        if got[int(w // bs)] == w:
            out.append(f"invalid start {s} (span {s // E.SPAN}, j {s % E.SPAN}) was hashed into bin {int(w // bs)}")
    return out


def assert_equal(got, cases, num_bins):
    assert got.shape == (len(cases), num_bins)
    for s, c in enumerate(cases):
        if not np.array_equal(got[s], c.expectation(num_bins)):
            wrong = np.flatnonzero(got[s] != c.expectation(num_bins))
            raise AssertionError(f"sample {s} ({c.name}), k = {c.k}, rc = {c.rc}, {num_bins} bins: {wrong.size} bins differ; "
                                 + "; ".join(differing_named_starts(c, got[s], num_bins)))
        if len(c.codes) < c.k:
            assert (got[s] == U64_MAX).all(), c.name


def run_staged(skl, ctx, cases, packed=False):
    """At 4096 bins (minima in LDS) and 4097 (the same kernel, minima in global memory)."""
    for nb in E.LDS_BINS:
        for c in cases:
            if c.valid or c.invalid:
                c.check(nb)
    out = {}
    for nb in E.LDS_BINS:
        got = call(skl, ctx, cases, nb, packed)
        assert "nthash_binmin_lds_kernel" in ctx.last_kernel() and ctx.last_kernel().endswith(FORM_OF_BINS[nb])
        assert_equal(got, cases, nb)
        out[nb] = got
    return out


@pytest.mark.parametrize("rc", [True, False])
@pytest.mark.parametrize("k", E.STAGED_KS)
def test_thread_boundary(skl, gpu_ctx, k, rc):
    """Eleven 3 000-base samples around a span boundary p = 128 m in one call: a break at p - 1, p, p + 1 (exactly at the
    thread's p0; inside its first window, after which the one seed must roll on exactly), at p + k - 1, p + k, p + k + 1
    (which the boundary windows just span or just clear), forty Ns at p and at p + 5, an offset at 0, none at all (a
    null pointer when the sample stands alone), one equal to the length.  Both entry points."""
    cases = E.thread_boundary(k, rc)
    byte_form = run_staged(skl, gpu_ctx, cases)
    packed_form = run_staged(skl, gpu_ctx, cases, packed=True)
    for nb in E.LDS_BINS:
        assert np.array_equal(byte_form[nb], packed_form[nb])
    alone = [c for c in cases if c.offsets.size == 0]
    assert len(alone) == 1
    run_staged(skl, gpu_ctx, alone)      # offsets == nullptr


@pytest.mark.parametrize("k,rc", E.STREAM_K_RC)
def test_k_against_the_dword_streams_in_the_last_thread(skl, gpu_ctx, k, rc):
    """The same samples around p = 65 536 - 128 of 65 836 bases: the named starts belong to the last thread of the first
    workgroup, whose entering stream reads the extra staged row; k = 16 / 17 and 32 / 33 put the entering code at bit
    30 / 0 of its dword, k = 128 / 129 eight dwords on, at 129 with the look-ahead dword clamped."""
    run_staged(skl, gpu_ctx, E.last_thread(k, rc))


@pytest.mark.parametrize("rc", [True, False])
@pytest.mark.parametrize("k", E.END_KS)
def test_workgroup_boundary_and_sample_end(skl, gpu_ctx, k, rc):
    """Samples of 65 535 .. 65 536 + k bases, 65 664, 65 665 and 131 073: the last start in the last thread of a
    workgroup, in the first of the next, a second workgroup with codes and no window (up to 65 536 + k - 1 bases) and
    with exactly one (65 536 + k), a third workgroup of one code."""
    run_staged(skl, gpu_ctx, E.sample_ends(k, rc))


@pytest.mark.parametrize("rc", [True, False])
def test_short_and_empty_samples_in_one_call(skl, gpu_ctx, rc):
    """Lengths 0, 1, k - 1, k, k + 1, 15, 16, 17, 0, 0, 200, 0 and then 70 000 at k = 21: the span -> sample search over
    empty samples at the front, in the middle and before the last, ragged last words, rows of u64::MAX for samples
    shorter than k.  Both entry points."""
    cases = E.short_and_empty(rc)
    assert [len(c.codes) for c in cases] == E.SHORT_LENGTHS + [70000]
    byte_form = run_staged(skl, gpu_ctx, cases)
    packed_form = run_staged(skl, gpu_ctx, cases, packed=True)
    for nb in E.LDS_BINS:
        assert np.array_equal(byte_form[nb], packed_form[nb])
        assert [bool((byte_form[nb][s] == U64_MAX).all()) for s in range(len(cases))] == [len(c.codes) < c.k for c in cases]


@pytest.mark.parametrize("k,rc", E.WIDE_K_RC)
def test_wide_bins(skl, gpu_ctx, k, rc):
    """A random sample of about 70 000 bases (three records, 0.1 % Ns) at 2^20 bins, where at least 90 % of ALL windows
    decide a bin: the staged kernel with the minima in global memory, and at k = 130 the unstaged kernel."""
    case = E.wide_case(k, rc)
    E.check_wide(case)
    got = call(skl, gpu_ctx, [case], E.WIDE)
    assert gpu_ctx.last_kernel().startswith(UNSTAGED) if k >= 130 else gpu_ctx.last_kernel().endswith(IN_GLOBAL)
    exp = case.expectation(E.WIDE)
    if not np.array_equal(got[0], exp):
        starts, signs = case.table
        bins = (signs // np.uint64(E.bin_size_of(E.WIDE))).astype(np.int64)
        bad = starts[got[0][bins] != exp[bins]]
        raise AssertionError(f"k = {k}, rc = {rc}: {int((got[0] != exp).sum())} bins differ; first windows whose bins differ: {bad[:20].tolist()}")


@pytest.mark.parametrize("k,rc", [(k, rc) for k in E.UNSTAGED_KS for rc in E.UNSTAGED_RC[k]])
def test_unstaged_kernel(skl, gpu_ctx, k, rc):
    """nthash_binmin_kernel (256 starts per thread, what k >= 130 takes) at 2^20 bins: the thread-boundary samples
    around p = 256 m and samples that end around 65 536; k = 257 and 300 make a window longer than a span.  A break
    makes this kernel re-seed, and the first valid start behind every break is named."""
    for cases in (E.unstaged_boundary(k, rc), E.unstaged_ends(k, rc)):
        for c in cases:
            c.check(E.WIDE)
            assert all(int(o) in c.valid for o in np.unique(c.offsets) if 0 < o <= len(c.codes) - k)
        got = call(skl, gpu_ctx, cases, E.WIDE)
        assert gpu_ctx.last_kernel().startswith(UNSTAGED)
        assert_equal(got, cases, E.WIDE)


@pytest.mark.ab_library
def test_staged_cases_on_the_unstaged_kernel(skl, gpu_ctx, set_switch):
    """SKL_SKETCH_KERNEL=global (A/B library): the staged cases through nthash_binmin_kernel equal the staged result and
    the reference."""
    groups = [E.thread_boundary(k, True) for k in E.STAGED_KS] + [E.last_thread(17, True), E.last_thread(129, False),
                                                                  E.sample_ends(31, True), E.short_and_empty(True)]
    staged = [run_staged(skl, gpu_ctx, cases) for cases in groups]
    set_switch("SKL_SKETCH_KERNEL", "global")
    for cases, want in zip(groups, staged):
        for nb in E.LDS_BINS:
            got = call(skl, gpu_ctx, cases, nb)
            assert gpu_ctx.last_kernel().startswith(UNSTAGED)
            assert_equal(got, cases, nb)
            assert np.array_equal(got, want[nb])


@pytest.mark.parametrize("num_bins", [1, 63, 64, 1000, 4096, 4097, 100032])
def test_bin_arithmetic(skl, gpu_ctx, num_bins):
    """3 000 random bases at k = 21 and 130 (both kernels' bin corrections) filed into one bin, odd and even counts, both
    sides of the LDS limit and 100 032 bins.  Plain equality; the `++bin` branch is not reached by inputs of this size."""
    codes, offsets = E.bins_sample()
    for k, form in ((21, IN_LDS if num_bins <= 4096 else IN_GLOBAL), (130, UNSTAGED)):
        case = E.plain_case(codes, offsets, k, True)
        got = call(skl, gpu_ctx, [case], num_bins)
        assert form in gpu_ctx.last_kernel()
        assert_equal(got, [case], num_bins)
        assert int((got != U64_MAX).sum()) >= min(num_bins, 2000) * 0.5


@pytest.mark.parametrize("k", [1, 2, 3])
def test_small_k(skl, gpu_ctx, k):
    """k = 1, 2, 3 on the thread-boundary samples: at most 4^k / 2 signs, so plain equality."""
    for rc in (True, False):
        cases = E.small_k_samples(k, rc)
        for nb in (64,) + E.LDS_BINS:
            assert_equal(call(skl, gpu_ctx, cases, nb), cases, nb)
            assert_equal(call(skl, gpu_ctx, cases, nb, packed=True), cases, nb)


def host_batches(words, setting):
    """The batches of whole samples sketch_signs_impl cuts (csrc/sketch_plan.hpp sketch_upload_batches): a batch is
    closed behind the sample with which it reaches `setting` words, unless that is the last -> ([(first, end)], cut
    exactly at the setting?)."""
    cuts, exact = [0], False
    begin = np.concatenate([[0], np.cumsum(words)])
    for s in range(len(words)):
        if begin[s + 1] - begin[cuts[-1]] >= setting and s + 1 < len(words):
            exact |= bool(begin[s + 1] - begin[cuts[-1]] == setting)
            cuts.append(s + 1)
    cuts.append(len(words))
    return list(zip(cuts[:-1], cuts[1:])), exact


@pytest.mark.parametrize("which", ["short", "seven"])
def test_batches_at_small_shapes(skl, gpu_ctx, set_switch, which):
    """SKL_SKETCH_BATCH_WORDS = 1 (every non-empty sample a batch: the two-slot ring reused, a trailing batch of empty
    samples alone), 4096, a value that closes a batch exactly at the setting, unset: the same output, equal to the
    reference, from both entry points.  The named starts of the later batches show `first_span != 0`."""
    cases = E.short_and_empty(True, E.LDS_BINS, 2) if which == "short" else E.batch_samples()
    words = np.array([(len(c.codes) + 15) // 16 for c in cases])
    exact_setting = int(words[:3].sum()) if which == "short" else int(words[0])
    one, _ = host_batches(words, 1)
    assert len(one) >= 3 and len(one) == int((words > 0).sum()) + (1 if which == "short" else 0)
    assert all(int((words[a:b] > 0).sum()) == 1 for a, b in one if words[a:b].any())
    if which == "short":
        assert not words[one[-1][0]:].any() and one[-1][1] - one[-1][0] == 2      # the `words == 0` batch
    assert len(host_batches(words, 4096)[0]) >= 2
    assert host_batches(words, exact_setting)[1] and len(host_batches(words, exact_setting)[0]) >= 2
    results = []
    for setting in (1, 4096, exact_setting, None):
        set_switch("SKL_SKETCH_BATCH_WORDS", setting)
        results.append((run_staged(skl, gpu_ctx, cases)[4096], run_staged(skl, gpu_ctx, cases, packed=True)[4096]))
    for byte_form, packed_form in results:
        assert np.array_equal(byte_form, results[-1][0]) and np.array_equal(packed_form, results[-1][0])
