"""skl_sketches_select / skl_sketches_concat: a new slab made on the device from resident ones must be the slab that
skl_sketches_create makes from the same samples taken in numpy -- its rows (bin-match counts, u32, exact), its pad rows and
lane slab (kNN and dense core/accessory calls), its completeness vector with everything derived from it (bit-identical
f32: both slabs install it the same way) and its own generation id (early-break plans).  Shapes: n around the lane-slab
group of 64 and the pad rows, row lengths from 7 to 1 120 16-byte words (8 to 256 lanes per row in the gather)."""
import numpy as np
import pytest

from sketchlib.rust_amd import synth

pytestmark = pytest.mark.gpu

KMERS = {1: [21], 3: [17, 21, 25], 5: [15, 19, 23, 27, 31]}
SHAPES = [(1, 1), (3, 2), (5, 32)]


def make_bins(n, nk, ss64, first_sample=0):
    """Clusters of relatives (counts that differ from pair to pair), two random samples in front."""
    r = synth.set_r(n, KMERS[nk], ss64, n_clusters=max(1, n // 8), first_sample=first_sample)
    r[:2] = synth.set_u(min(n, 2), nk, ss64, first_sample=first_sample)[:2]
    return np.ascontiguousarray(r)


def id_lists(n):
    ids = {"identity": np.arange(n), "reverse": np.arange(n)[::-1], "every second": np.arange(0, n, 2), "last": np.array([n - 1]),
           "repeat": np.array([0, n - 1, n // 2, n - 1, 0]), "longer than n": np.concatenate([np.arange(n), np.arange(n)[::-1], [n // 3]])}
    return {k: v.astype(np.uint32) for k, v in ids.items()}


@pytest.fixture(scope="module")
def source_bins():
    return {(n, nk, ss64): make_bins(n, nk, ss64) for n in (1, 63, 64, 65, 129) for nk, ss64 in SHAPES}


@pytest.mark.parametrize("nk,ss64", SHAPES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_select_exact(skl, gpu_ctx, source_bins, n, nk, ss64):
    bins = source_bins[n, nk, ss64]
    s = gpu_ctx.sketches(bins, n, KMERS[nk], ss64)
    before = skl.self_binmatch(gpu_ctx, s)
    for what, ids in id_lists(n).items():
        sel = s.select(ids)
        fresh = gpu_ctx.sketches(np.ascontiguousarray(bins[ids]), len(ids), KMERS[nk], ss64)
        assert sel.n == len(ids) == skl.load().skl_sketches_n_samples(sel._h)
        assert np.array_equal(skl.self_binmatch(gpu_ctx, sel), skl.self_binmatch(gpu_ctx, fresh)), what
        # (a single sample has no pair with itself: its row is checked against the source's samples)
        assert np.array_equal(skl.cross_binmatch(gpu_ctx, sel, s), skl.cross_binmatch(gpu_ctx, fresh, s)), what
        sel.close()
        fresh.close()
    assert np.array_equal(skl.self_binmatch(gpu_ctx, s), before)   # the source is untouched
    s.close()


def test_select_pad_rows_and_tiles(skl, gpu_ctx, source_bins):
    """kNN and dense core/accessory calls read the pad rows behind row n - 1 and the lane slab of the result."""
    n, nk, ss64 = 129, 5, 32
    bins = source_bins[n, nk, ss64]
    ids = np.concatenate([np.arange(128, 0, -2), [0]]).astype(np.uint32)   # 65 of 129, the source's last row first
    assert len(ids) == 65
    s = gpu_ctx.sketches(bins, n, KMERS[nk], ss64)
    sel = s.select(ids)
    fresh = gpu_ctx.sketches(np.ascontiguousarray(bins[ids]), 65, KMERS[nk], ss64)
    for p in (sel.set_k(), sel.set_k(23)):
        got, want = skl.self_dists_knn(gpu_ctx, sel, p, 3), skl.self_dists_knn(gpu_ctx, fresh, p, 3)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    assert np.array_equal(skl.self_dists_all(gpu_ctx, sel, sel.set_k()).view(np.uint32),
                          skl.self_dists_all(gpu_ctx, fresh, fresh.set_k()).view(np.uint32))
    for x in (s, sel, fresh):
        x.close()


def coreacc_bits(skl, ctx, s):
    return skl.self_dists_all(ctx, s, s.set_k()).view(np.uint32)


def test_select_with_completeness(skl, gpu_ctx):
    """0.81 x 0.81 is above the default cutoff of 0.64, 0.81 x 0.5 and 0.5 x 1.0 below it, 1.0 x 0.81 above."""
    n, nk, ss64 = 129, 3, 2
    bins = make_bins(n, nk, ss64)
    comp = np.where(np.arange(n) % 3 == 0, 0.5, 1.0)
    comp[7] = comp[64] = comp[128] = 0.81
    ids = np.concatenate([np.arange(n)[::-1], [7, 64, 0]]).astype(np.uint32)
    s = gpu_ctx.sketches(bins, n, KMERS[nk], ss64, comp)
    sel = s.select(ids)
    fresh = gpu_ctx.sketches(np.ascontiguousarray(bins[ids]), len(ids), KMERS[nk], ss64, comp[ids])
    plain = gpu_ctx.sketches(np.ascontiguousarray(bins[ids]), len(ids), KMERS[nk], ss64)
    assert np.array_equal(coreacc_bits(skl, gpu_ctx, sel), coreacc_bits(skl, gpu_ctx, fresh))
    assert not np.array_equal(coreacc_bits(skl, gpu_ctx, sel), coreacc_bits(skl, gpu_ctx, plain))   # (the vector did follow)
    for x in (s, sel, fresh, plain):
        x.close()


def test_select_unit_completeness_from_a_non_unit_vector(skl, gpu_ctx):
    """Sample 0 has completeness 0 (not in (0, 1]); the 256 others selected give a vector the lean early-break epilogue may
    take (nk = 5, 256 x 256 pairs: the early break applies): what is derived from the vector is the result's own."""
    n, nk, ss64 = 257, 5, 2
    bins = make_bins(n, nk, ss64)
    comp = np.where(np.arange(n) % 2 == 0, 0.9, 1.0)
    comp[0] = 0.0
    ids = np.arange(1, n).astype(np.uint32)
    s = gpu_ctx.sketches(bins, n, KMERS[nk], ss64, comp)
    sel = s.select(ids)
    fresh = gpu_ctx.sketches(np.ascontiguousarray(bins[ids]), len(ids), KMERS[nk], ss64, comp[ids])
    assert np.array_equal(coreacc_bits(skl, gpu_ctx, sel), coreacc_bits(skl, gpu_ctx, fresh))
    for x in (s, sel, fresh):
        x.close()


@pytest.mark.parametrize("n_a,n_b", [(1, 1), (63, 1), (64, 64), (65, 130)])
def test_concat(skl, gpu_ctx, n_a, n_b):
    nk, ss64 = 3, 2
    a_bins, b_bins, c_bins = make_bins(n_a, nk, ss64), make_bins(n_b, nk, ss64, first_sample=1000), make_bins(33, nk, ss64, first_sample=5)
    a, b, c = (gpu_ctx.sketches(x, len(x), KMERS[nk], ss64) for x in (a_bins, b_bins, c_bins))
    before = skl.cross_binmatch(gpu_ctx, a, c), skl.cross_binmatch(gpu_ctx, b, c)
    ab = skl.concat(a, b)
    fresh = gpu_ctx.sketches(np.ascontiguousarray(np.concatenate([a_bins, b_bins])), n_a + n_b, KMERS[nk], ss64)
    assert ab.n == n_a + n_b
    assert np.array_equal(skl.self_binmatch(gpu_ctx, ab), skl.self_binmatch(gpu_ctx, fresh))
    p = ab.set_k()
    assert np.array_equal(skl.cross_dists_all(gpu_ctx, ab, c, p).view(np.uint32), skl.cross_dists_all(gpu_ctx, fresh, c, p).view(np.uint32))
    assert np.array_equal(skl.cross_dists_all(gpu_ctx, c, ab, p).view(np.uint32), skl.cross_dists_all(gpu_ctx, c, fresh, p).view(np.uint32))
    # the inputs are still usable and unchanged
    assert np.array_equal(skl.cross_binmatch(gpu_ctx, a, c), before[0]) and np.array_equal(skl.cross_binmatch(gpu_ctx, b, c), before[1])
    for x in (a, b, c, ab, fresh):
        x.close()


def test_concat_completeness_and_errors(skl, gpu_ctx):
    nk, ss64 = 3, 2
    a_bins, b_bins = make_bins(65, nk, ss64), make_bins(40, nk, ss64, first_sample=1000)
    ca, cb = np.where(np.arange(65) % 2 == 0, 0.5, 1.0), np.full(40, 0.81)
    a = gpu_ctx.sketches(a_bins, 65, KMERS[nk], ss64, ca)
    b = gpu_ctx.sketches(b_bins, 40, KMERS[nk], ss64, cb)
    ab = skl.concat(a, b)
    fresh = gpu_ctx.sketches(np.ascontiguousarray(np.concatenate([a_bins, b_bins])), 105, KMERS[nk], ss64, np.concatenate([ca, cb]))
    assert np.array_equal(coreacc_bits(skl, gpu_ctx, ab), coreacc_bits(skl, gpu_ctx, fresh))
    b.set_completeness(None)   # one side only
    with pytest.raises(skl.SklError) as e:
        skl.concat(a, b)
    assert e.value.code == skl.ERR_INVALID_ARG
    other_size = gpu_ctx.sketches(make_bins(4, nk, 3), 4, KMERS[nk], 3)
    other_k = gpu_ctx.sketches(make_bins(4, nk, ss64), 4, [17, 21, 29], ss64)
    for other in (other_size, other_k):
        with pytest.raises(skl.SklError) as e:
            skl.concat(b, other)
        assert e.value.code == skl.ERR_INCOMPATIBLE
    gpu_ctx.synchronize()
    for x in (a, b, ab, fresh, other_size, other_k):
        x.close()


def test_plan_cache_follows_the_generation_id(skl, gpu_ctx):
    """nk = 5 and 256 x 256 pairs: core/accessory calls take a sampled early-break decision kept under the slabs' generation
    ids.  s, its reversal, s again: each equals its fresh counterpart, so no decision of one slab served another."""
    n, nk, ss64 = 256, 5, 2
    bins = make_bins(n, nk, ss64)
    rev = np.arange(n)[::-1].astype(np.uint32)
    s = gpu_ctx.sketches(bins, n, KMERS[nk], ss64)
    fresh_s = gpu_ctx.sketches(bins, n, KMERS[nk], ss64)
    fresh_rev = gpu_ctx.sketches(np.ascontiguousarray(bins[rev]), n, KMERS[nk], ss64)
    want_s, want_rev = coreacc_bits(skl, gpu_ctx, fresh_s), coreacc_bits(skl, gpu_ctx, fresh_rev)
    assert np.array_equal(coreacc_bits(skl, gpu_ctx, s), want_s)
    sel = s.select(rev)
    assert np.array_equal(coreacc_bits(skl, gpu_ctx, sel), want_rev)
    assert np.array_equal(coreacc_bits(skl, gpu_ctx, s), want_s)
    for x in (s, sel, fresh_s, fresh_rev):
        x.close()


def test_select_64_bit_offsets(skl, gpu_ctx):
    """A row slab past 4 GiB (n x 17 920 B > 2^32): the last 64 rows lie beyond what a 32-bit byte offset reaches.  Rows
    between the first and last 64 are zero, so a wrapped offset reads something else than the row it should."""
    torch = pytest.importorskip("torch")
    free, _ = torch.cuda.mem_get_info()
    if free < 16 << 30:
        pytest.skip(f"needs 16 GiB of free device memory for two 4.3 GB slabs, {free >> 30} GiB are free")
    nk, ss64 = 5, 32
    words = nk * ss64 * 14
    n = (1 << 32) // (words * 8) + 1000
    assert n * words * 8 > 1 << 32 and (n - 64) * words * 8 > 1 << 32
    dev = torch.device("cuda:0")
    t = torch.zeros((n, words), dtype=torch.int64, device=dev)
    ends = synth.set_u_device(128, nk, ss64, dev)
    t[:64] = ends[:64]
    t[n - 64:] = ends[64:]
    torch.cuda.synchronize()
    s = gpu_ctx.sketches(t, n, KMERS[nk], ss64)
    del t
    ids = np.concatenate([np.arange(64), np.arange(n - 64, n)]).astype(np.uint32)
    sel = s.select(ids)
    fresh = gpu_ctx.sketches(ends.contiguous(), 128, KMERS[nk], ss64)
    got, want = skl.self_binmatch(gpu_ctx, sel), skl.self_binmatch(gpu_ctx, fresh)
    assert np.array_equal(got, want)
    host = gpu_ctx.sketches(synth.set_u(128, nk, ss64), 128, KMERS[nk], ss64)   # (the same words, generated on the host)
    assert np.array_equal(got, skl.self_binmatch(gpu_ctx, host))
    for x in (s, sel, fresh, host):
        x.close()
    torch.cuda.empty_cache()


def test_argument_errors_launch_nothing(skl, gpu_ctx):
    n, nk, ss64 = 10, 3, 2
    bins = make_bins(n, nk, ss64)
    s = gpu_ctx.sketches(bins, n, KMERS[nk], ss64)
    for ids in ([], [n], [0, 3, n, 1], [0xFFFFFFFF]):
        with pytest.raises(skl.SklError) as e:
            s.select(np.array(ids, dtype=np.uint32))
        assert e.value.code == skl.ERR_INVALID_ARG
        gpu_ctx.synchronize()
    sel = s.select([9, 0])
    fresh = gpu_ctx.sketches(np.ascontiguousarray(bins[[9, 0]]), 2, KMERS[nk], ss64)
    assert np.array_equal(skl.self_binmatch(gpu_ctx, sel), skl.self_binmatch(gpu_ctx, fresh))
    for x in (s, sel, fresh):
        x.close()
