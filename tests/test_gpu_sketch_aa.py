"""skl_sketch_signs_aa (csrc/aa_sketch_kernel.hip, dealt by csrc/aa_plan.hpp) against the undensified signs of
tests/aa_reference.py, the Python restatement of the reference's AaHashIterator (no reference binary has confirmed it: see its
docstring).  concat_end_rule = 1 is the iterator as it is (a sample it panics on comes back all-max); concat_end_rule = 0 is the
iterator over the sample with a separator appended, i.e. every window of k valid residues.

A sample of at least `long_min` residues takes the staged kernel, every other the unstaged one; SKL_AA_LONG_MIN=1 stages every
sample, so the small cases here run through both forms.  Every case is a few thousand to a few hundred thousand residues."""
import functools

import numpy as np
import pytest

import aa_reference as R

pytestmark = pytest.mark.gpu
LETTERS = np.frombuffer(R.LETTERS.encode(), dtype=np.uint8)


def protein(rng, n, separators=0):
    seq = LETTERS[rng.integers(0, 20, size=n)].copy()
    if separators and n:
        seq[rng.choice(n, size=min(separators, n), replace=False)] = ord("*")
    return seq.tobytes()


def call(skl, ctx, seqs, kmers, bins, level=1, end_rule=False):
    codes = [skl.aa_codes(s) for s in seqs]
    res_begin = np.concatenate([[0], np.cumsum([c.size for c in codes])]).astype(np.uint64)
    flat = np.concatenate(codes) if codes else np.zeros(0, dtype=np.uint8)
    return skl.sketch_signs_aa(ctx, flat, res_begin, kmers, bins, level, end_rule)


def want(seqs, kmers, bins, level=1, end_rule=False):
    f = R.signs_or_max if end_rule else R.natural_signs
    return np.stack([np.stack([f(s, k, bins, level) for k in kmers]) for s in seqs])


def check(skl, ctx, seqs, kmers, bins, level=1, end_rule=False, expect=None):
    got = call(skl, ctx, seqs, kmers, bins, level, end_rule)
    expect = want(seqs, kmers, bins, level, end_rule) if expect is None else expect
    bad = np.argwhere((got != expect).any(axis=2))
    assert bad.size == 0, f"(sample, k index) that differ: {bad[:8].tolist()} of {len(seqs)} samples; kernel: {ctx.last_kernel()}"
    return got


@pytest.fixture(scope="module")
def shape(skl):
    return skl.sketch_aa_shape()


@pytest.fixture(params=["as_planned", "all_staged"])
def form(request, set_switch):
    """The plan's own choice, and every sample forced through the staged kernel."""
    if request.param == "all_staged":
        set_switch("SKL_AA_LONG_MIN", 1)
    return request.param


def test_thread_span_boundary(skl, gpu_ctx, shape, form):
    """One sample of three thread spans, a single separator at each position from span - k - 1 to span + k + 1: the windows that
    straddle the boundary between two threads lose exactly the ones that hold the separator."""
    rng = np.random.default_rng(21)
    for which in ("1", "2", "3", "7", "span", "span+1"):
        span0 = shape["span_lds"] if form == "all_staged" else shape["short_span"](1)
        k = {"span": span0, "span+1": span0 + 1}.get(which) or int(which)
        span = shape["span_lds"] if form == "all_staged" else shape["short_span"](k)
        base = bytearray(protein(rng, 3 * span))
        seqs = []
        for pos in range(max(0, span - k - 1), min(3 * span, span + k + 2)):
            s = bytearray(base)
            s[pos] = ord("X")
            seqs.append(bytes(s))
        for end_rule in (False, True):
            check(skl, gpu_ctx, seqs, [k], 1024, end_rule=end_rule)
        assert ("lds_kernel" in gpu_ctx.last_kernel()) == (form == "all_staged")


def test_workgroup_boundary_and_sample_end(skl, gpu_ctx, shape):
    """Lengths of exactly one workgroup's window starts, +-1, +-k, in the form the plan gives them: 16 384-residue samples are
    staged, 4 096-residue samples share unstaged workgroups with their neighbours."""
    rng = np.random.default_rng(22)
    k = 7
    wg_staged = shape["wg_lds"] * shape["span_lds"]
    wg_unstaged = shape["wg_short"] * shape["short_span"](k)
    assert wg_unstaged < shape["long_min"] <= wg_staged - k
    seqs = [protein(rng, wg + d, separators=3) for wg in (wg_staged, wg_unstaged) for d in (0, 1, -1, k, -k, k - 1, 1 - k)]
    for end_rule in (False, True):
        check(skl, gpu_ctx, seqs, [k], 1024, end_rule=end_rule)
    assert "lds_kernel" in gpu_ctx.last_kernel() and "aahash_binmin_kernel" in gpu_ctx.last_kernel()


def test_end_rule(skl, gpu_ctx, form):
    """The reference's iterator seeds only where start < len - k.  Both settings; the residue before the last window valid or a
    separator; lengths k - 1, k, k + 1, which the reference panics on or gives its two windows for."""
    rng = np.random.default_rng(23)
    for k in (3, 5, 20):
        seqs = []
        for n in (k - 1, k, k + 1, k + 2, 3 * k, 100):
            s = protein(rng, n)
            seqs.append(s)
            if n > k:
                seqs.append(s[:n - k - 1] + b"*" + s[n - k:])      # the residue before the last window is a separator
                seqs.append(s[:n - 1] + b"*")                      # the sample ends in one, as without --concat-fasta
                seqs.append(s[:n - 2] + b"-" + s[n - 1:])          # the last window holds one
        ruled = check(skl, gpu_ctx, seqs, [k], 512, end_rule=True)
        every = check(skl, gpu_ctx, seqs, [k], 512, end_rule=False)
        filled = lambda a: (a != np.uint64(R.U64)).sum(axis=(1, 2))
        assert filled(ruled)[0] == 0 and filled(ruled)[1] == 0 and filled(every)[0] == 0 and filled(every)[1] == 1     # len k - 1, k
        assert filled(ruled)[2] == 2 and filled(every)[2] == 2                                                         # len k + 1
        assert filled(ruled)[3] == 0 and filled(every)[3] == 1      # k + 1 residues, the first a separator: only the window at len - k
        assert (filled(ruled) <= filled(every)).all() and (filled(ruled) < filled(every)).any()


def test_roll_periods(skl, gpu_ctx, shape, form):
    """k at and around the periods of the two halves of the split rotation, and past what the staged kernel takes."""
    seq = protein(np.random.default_rng(24), 400, separators=2)
    kmers = [31, 32, 33, 34, 62, 64, 66]
    check(skl, gpu_ctx, [seq], kmers, 1024)
    assert ("lds_kernel" in gpu_ctx.last_kernel()) == (form == "all_staged")
    beyond = shape["k_staged_max"] + 1
    check(skl, gpu_ctx, [seq], [shape["k_staged_max"], beyond], 1024)
    assert "lds_kernel" not in gpu_ctx.last_kernel()      # one k-mer length past the limit sends every sample to the unstaged form


@functools.lru_cache(maxsize=None)
def proteome():
    """20 000 residues in 60 records (a separator after each), a few invalid residues."""
    rng = np.random.default_rng(25)
    cuts = np.sort(rng.choice(np.arange(50, 19950), size=59, replace=False))
    seq = bytearray(protein(rng, 20000, separators=5))
    for c in cuts:
        seq[c] = ord("*")
    seq[-1] = ord("*")
    return bytes(seq)


@pytest.mark.parametrize("level", [1, 2, 3])
def test_levels(skl, gpu_ctx, level):
    check(skl, gpu_ctx, [proteome()], [5], 1024, level=level)
    assert "lds_kernel" in gpu_ctx.last_kernel()


def test_bins(skl, gpu_ctx, shape):
    """Bin minima in LDS up to lds_bins_max, in global memory beyond; a staged and two unstaged samples in one call."""
    rng = np.random.default_rng(26)
    seqs = [protein(rng, 300), proteome(), protein(rng, 70, separators=1)]
    for bins in (64, 1024, shape["lds_bins_max"], shape["lds_bins_max"] + 64, 100032):
        check(skl, gpu_ctx, seqs, [5], bins)


def test_short_empty_and_all_separator_samples_beside_a_long_one(skl, gpu_ctx, form):
    rng = np.random.default_rng(27)
    seqs = [b"", protein(rng, 2), b"*" * 40, proteome(), b"", b"X", protein(rng, 9), b"-" * 9000, protein(rng, 5)]
    for end_rule in (False, True):
        got = check(skl, gpu_ctx, seqs, [3, 5], 256, end_rule=end_rule)
        for s in (0, 1, 2, 4, 5, 7):
            assert (got[s] == np.uint64(R.U64)).all()


@functools.lru_cache(maxsize=None)
def short_samples():
    rng = np.random.default_rng(28)
    seqs = tuple(protein(rng, int(n), separators=int(n) // 40) for n in rng.integers(5, 71, size=3000))
    return seqs, want(seqs, [5], 64, end_rule=True)


@functools.lru_cache(maxsize=None)
def long_sample():
    seq = protein(np.random.default_rng(29), 200000, separators=50)
    return seq, want([seq], [5], 64, end_rule=True)


def test_many_short_samples(skl, gpu_ctx):
    """3 000 proteins of 5 to 70 residues: a dozen to a workgroup, no padding."""
    seqs, expect = short_samples()
    check(skl, gpu_ctx, seqs, [5], 64, end_rule=True, expect=expect)
    assert "lds_kernel" not in gpu_ctx.last_kernel()


def test_many_short_samples_around_a_long_one(skl, gpu_ctx):
    seqs, expect = short_samples()
    long_seq, long_expect = long_sample()
    mixed = seqs[:1500] + (long_seq,) + seqs[1500:]
    check(skl, gpu_ctx, mixed, [5], 64, end_rule=True, expect=np.concatenate([expect[:1500], long_expect, expect[1500:]]))
    assert "lds_kernel" in gpu_ctx.last_kernel() and "aahash_binmin_kernel" in gpu_ctx.last_kernel()


def test_batch_cut_inside_a_run_of_short_samples(skl, gpu_ctx, set_switch):
    """SKL_AA_BATCH_SIGN_BYTES lowered to 100 samples' worth of signs: thirty batches, cuts inside the run of short samples and
    either side of the long one, the same signs."""
    seqs, expect = short_samples()
    long_seq, long_expect = long_sample()
    mixed = seqs[:1450] + (long_seq,) + seqs[1450:]
    expect = np.concatenate([expect[:1450], long_expect, expect[1450:]])
    set_switch("SKL_AA_BATCH_SIGN_BYTES", 100 * 64 * 8)
    check(skl, gpu_ctx, mixed, [5], 64, end_rule=True, expect=expect)
    set_switch("SKL_AA_BATCH_SIGN_BYTES", 1)        # every sample a batch of its own
    check(skl, gpu_ctx, mixed[1400:1500], [5], 64, end_rule=True, expect=expect[1400:1500])


def test_refuses_what_it_cannot_index(skl, gpu_ctx):
    with pytest.raises(skl.SklError):
        skl.sketch_signs_aa(gpu_ctx, np.array([1, 2, 21, 3], dtype=np.uint8), [0, 4], [3], 64)
    with pytest.raises(skl.SklError):
        skl.sketch_signs_aa(gpu_ctx, np.array([1, 2, 3], dtype=np.uint8), [0, 3], [3], 64, level=4)
