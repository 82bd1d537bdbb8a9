"""The column-window kNN at the shapes the drivers cut (multi_gpu.knn_window_cuts), in both forms, against the oracle.

* travelling heaps: skl_self_dists_knn_window, one set of heaps that every participant feeds its window in turn;
* decoupled: skl_self_dists_knn_window_logged against heaps each participant starts empty, its accept logs replayed in window
  order (skl_knn_heaps_replay) into one empty heap per row.
The participants run one after the other on the one device (exact: a participant never touches a row again after the band
that holds it).  The windows always come from knn_window_cuts.  The bar is the oracle's whole-row BinaryHeap replay
(TIES_RUST_HEAP): ids, order and both distances, compared as uint32; with a completeness vector the bar of the other
completeness kNN tests (ids exact, distances within 1e-6).  Then the regimes the decoupled form can be in -- tile pruning,
the forced early break below col_lo, a completeness vector, overflowing logs -- the replay's clamp, and the two drivers of
multi_gpu in-process."""
import numpy as np
import pytest

from sketchlib.rust_amd import multi_gpu, synth

pytestmark = pytest.mark.gpu

KMERS = [17, 21, 25, 29]


def _device():
    import torch

    return torch.device("cuda", 0)


def _sync(ctx):
    import torch

    torch.cuda.synchronize()
    ctx.synchronize()


def _data(n, kmers, ss64, seed=3):
    """Clusters of ~10 relatives (Set R), a tenth of the samples with no relative at all (Set U) and a few exact duplicates."""
    rng = np.random.default_rng(seed)
    bins = np.ascontiguousarray(synth.set_r(n, kmers, ss64, n_clusters=max(2, n // 10), seed=synth.SEED_R + seed))
    lone = rng.choice(n, max(1, n // 10), replace=False)
    bins[lone] = synth.set_u(len(lone), len(kmers), ss64, seed=synth.SEED_U + seed)
    for src, dst in rng.choice(n, (max(1, n // 40), 2)):
        bins[dst] = bins[src]
    return bins


def _key(g, oracle, dist, kmers):
    """-> (params, oracle args, coreacc, ani)."""
    if dist == "coreacc":
        return g.set_k(), (oracle.COREACC, 0, False), True, False
    k_idx = 1 if len(kmers) > 1 else 0
    return g.set_k(kmers[k_idx], dist == "ani"), (oracle.JACCARD, k_idx, dist == "ani"), False, dist == "ani"


def _windows(n, band_rows, world):
    """[(lo, hi, bands)] per participant: the bands that start below hi, ascending (what the drivers feed)."""
    cuts = multi_gpu.knn_window_cuts(n, band_rows, world)
    n_bands = (n + band_rows - 1) // band_rows
    return [(cuts[r], cuts[r + 1], [b for b in range(n_bands) if b * band_rows < cuts[r + 1]]) for r in range(world)]


def _replay_logs(skl, ctx, final, knn, lg, n):
    import torch

    m = max(1, int(lg["len"][:n].max()))
    rec, ids = lg["rec"][:n, :m].contiguous(), lg["id"][:n, :m].contiguous()
    lens = lg["len"][:n].contiguous()
    torch.cuda.synchronize()      # (torch cuts the logs on ITS stream; the session's context runs on a stream of its own)
    skl.knn_heaps_replay(ctx, final, 0, n, knn, rec, ids, lens)
    ctx.synchronize()


def _run(skl, ctx, g, p, knn, band_rows, world, form, coreacc, ani=False, cap=None, on_call=None):
    """All participants of the column-window pipeline one after the other -> (idx, d0, d1) as numpy arrays."""
    dev = _device()
    n = g.n
    cap = n if cap is None else cap          # (a row takes at most n - 1 candidates: the ample default never overflows)
    final = skl.knn_heaps_alloc(n, knn, coreacc, dev)
    _sync(ctx)
    for r, (lo, hi, bands) in enumerate(_windows(n, band_rows, world)):
        if form == "travelling":
            heaps, lg = final, None
        else:
            heaps, lg = skl.knn_heaps_alloc(n, knn, coreacc, dev), skl.knn_logs_alloc(n, cap, coreacc, dev)
            _sync(ctx)
        for band in bands:
            if lg is None:
                skl.self_dists_knn_window(ctx, g, p, knn, band_rows, band, lo, hi, heaps)
            else:
                skl.self_dists_knn_window_logged(ctx, g, p, knn, band_rows, band, lo, hi, heaps, lg)
            if on_call is not None:
                on_call(r, lo, hi, band, ctx.last_kernel())
        ctx.synchronize()
        if lg is not None:
            assert int(lg["len"].max()) <= cap, "the test's logs are meant to hold"
            assert int(lg["len"][hi:].sum()) == 0          # rows behind the window meet none of its pairs
            _replay_logs(skl, ctx, final, knn, lg, n)       # participant r's logs, in window order
    idx, d0, d1 = skl.knn_heaps_finalize(ctx, final, 0, n, knn, ani=ani)
    ctx.synchronize()
    return idx.cpu().numpy(), d0.cpu().numpy(), (d1.cpu().numpy() if d1 is not None else None)


def _assert_exact(got, exp, coreacc):
    idx, d0, d1 = got
    assert np.array_equal(idx.astype(np.uint64), exp["idx"]), np.argwhere(idx.astype(np.uint64) != exp["idx"])[:5]
    assert np.array_equal(d0.view(np.uint32), exp["d0"].view(np.uint32)), np.argwhere(d0 != exp["d0"])[:5]
    if coreacc:
        assert np.array_equal(d1.view(np.uint32), exp["d1"].view(np.uint32)), np.argwhere(d1 != exp["d1"])[:5]


# ---- 1. the ABI: empty windows are no-ops, everything else it refused it still refuses ----

@pytest.mark.parametrize("logged", [False, True])
def test_empty_window_launches_nothing_and_touches_nothing(skl, gpu_ctx, logged):
    """col_lo == col_hi (<= n, on a band boundary or not, n itself included) is SKL_OK with no launch and the heaps and logs as
    they were; a window past n, a reversed one and a non-empty one that starts inside a band are still refused."""
    import torch

    n, kmers, ss64, knn, band_rows = 118, KMERS, 4, 5, 64
    g = gpu_ctx.sketches(_data(n, kmers, ss64), n, kmers, ss64)
    p = g.set_k(21)
    dev = _device()
    heaps = skl.knn_heaps_alloc(n, knn, False, dev)
    lg = skl.knn_logs_alloc(n, 8, False, dev)
    gen = torch.Generator(device="cpu").manual_seed(7)

    def pattern(t, hi):      # random contents -- but lengths and ids in range, as any state a call may be handed
        t.copy_(torch.randint(0, hi, t.shape, generator=gen, dtype=torch.int64).to(torch.int32).view(t.dtype))

    pattern(heaps["h_key"], 0x3F800000)
    pattern(heaps["h_id"], n)
    pattern(heaps["h_len"], knn + 1)
    pattern(heaps["thr"], 2 ** 31 - 1)
    pattern(lg["rec"], 0x3F800000)
    pattern(lg["id"], n)
    pattern(lg["len"], 9)
    before = {k: v.clone() for k, v in list(heaps.items()) + [("rec", lg["rec"]), ("id", lg["id"]), ("len", lg["len"])] if v is not None}
    _sync(gpu_ctx)

    def call(band, lo, hi):
        if logged:
            skl.self_dists_knn_window_logged(gpu_ctx, g, p, knn, band_rows, band, lo, hi, heaps, lg)
        else:
            skl.self_dists_knn_window(gpu_ctx, g, p, knn, band_rows, band, lo, hi, heaps)

    gpu_ctx.timing_enable()
    try:
        gpu_ctx.timing_reset()
        for band, w in ((0, 0), (0, 64), (1, 64), (0, n), (1, n), (0, 37), (1, 100)):
            call(band, w, w)
        _sync(gpu_ctx)
        assert gpu_ctx.kernel_ms()[1] == 0
    finally:
        gpu_ctx.timing_enable(0)
    after = {k: v for k, v in list(heaps.items()) + [("rec", lg["rec"]), ("id", lg["id"]), ("len", lg["len"])] if v is not None}
    for k in before:
        assert torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)), k
    for band, lo, hi in ((0, 64, 0), (0, n + 1, n + 1), (0, 0, n + 1), (2, 64, 64), (0, 32, 64), (0, 0, 100)):
        with pytest.raises(skl.SklError) as e:
            call(band, lo, hi)
        assert e.value.code == skl.ERR_INVALID_ARG
    g.close()


# ---- 2a. shapes x key type x form ----

SHAPES = [   # (n, band_rows, world, knn)
    (118, 64, 3, 9),     # the second cut used to round to 128 and clamp to n = 118: a window [118, 118) cut inside a band
    (47, 16, 4, 7),      # the same with four participants
    (50, 64, 4, 5),      # n < band_rows: one band, empty windows in front of the last participant
    (128, 32, 3, 7),     # n an exact band multiple
    (125, 32, 7, 5),     # more participants than bands: empty windows in the middle
    (118, 64, 3, 1),     # knn = 1
    (62, 32, 3, 40),     # knn >= band_rows: no early break, lists never full after one band; every row short of relatives
]


@pytest.mark.parametrize("form", ["travelling", "decoupled"])
@pytest.mark.parametrize("dist", ["jaccard", "ani", "coreacc"])
@pytest.mark.parametrize("n,band_rows,world,knn", SHAPES)
def test_window_shapes(oracle, skl, gpu_ctx, n, band_rows, world, knn, dist, form):
    bins = _data(n, KMERS, 4, seed=n + world)
    o, g = oracle.Sketches(bins, n, KMERS, 4), gpu_ctx.sketches(bins, n, KMERS, 4)
    p, oargs, coreacc, ani = _key(g, oracle, dist, KMERS)
    exp = oracle.self_dists_knn(o, knn, *oargs, ties=oracle.TIES_RUST_HEAP, threads=8)
    _assert_exact(_run(skl, gpu_ctx, g, p, knn, band_rows, world, form, coreacc, ani), exp, coreacc)
    g.close()


_BIG = {}


@pytest.mark.parametrize("form", ["travelling", "decoupled"])
@pytest.mark.parametrize("world", [3, 4, 8])
def test_window_shapes_at_the_library_band_height(oracle, skl, gpu_ctx, monkeypatch, world, form):
    """n = 8 000 with the band height every participant agrees on (skl_knn_band_rows): the last band boundary below n lies far
    below it, so several participants get empty windows and the last one the rest."""
    monkeypatch.delenv("SKL_KNN_BAND_ROWS", raising=False)
    gpu_ctx.reload_env()
    n, kmers, ss64, knn = 8000, [21], 2, 10
    if not _BIG:
        bins = _data(n, kmers, ss64, seed=80)
        _BIG["bins"] = bins
        _BIG["exp"] = oracle.self_dists_knn(oracle.Sketches(bins, n, kmers, ss64), knn, oracle.JACCARD, 0, False,
                                            ties=oracle.TIES_RUST_HEAP, threads=8)
    g = gpu_ctx.sketches(_BIG["bins"], n, kmers, ss64)
    p = g.set_k(21)
    band_rows = skl.knn_band_rows(g, p, world)
    assert n % band_rows != 0
    got = _run(skl, gpu_ctx, g, p, knn, band_rows, world, form, False, cap=16 * knn + 64)
    _assert_exact(got, _BIG["exp"], False)
    g.close()


# ---- 2b. tile pruning under logs ----

@pytest.mark.parametrize("knn", [1, 3])
def test_pruning_under_logs(oracle, skl, gpu_ctx, monkeypatch, knn):
    """Single-k keys, the prunable 32 x 128 tiles.  The base set is the one tests/test_gpu_knn_prune.py prunes whole-matrix (240
    clusters of 6, sample s in cluster s % 240: a tile whose id distances miss every multiple of 240 holds no relative); on top,
    samples moved to random ids (their relatives then sit at arbitrary distances), exact duplicates and rows with no relative at
    all.  Heaps that start empty on a window prune against what they took there (the band's own rows below the window: not at
    all); the replayed lists are the oracle's -- and tiles really were left early, in both forms."""
    import torch

    n, kmers, ss64, band_rows, world = 1440, [17, 21, 25], 32, 64, 3
    t = synth.set_clustered_device(n, len(kmers), ss64, _device(), keep=0.94, n_clusters=240)
    bins = np.ascontiguousarray(t.cpu().numpy().view(np.uint64))
    del t
    torch.cuda.empty_cache()
    rng = np.random.default_rng(12)
    moved = rng.choice(n, 8, replace=False)
    bins[moved] = bins[rng.permutation(moved)]
    lone = rng.choice(n, 3, replace=False)
    bins[lone] = synth.set_u(3, len(kmers), ss64, seed=synth.SEED_U + 12)
    for src, dst in rng.choice(n, (4, 2)):
        bins[dst] = bins[src]
    monkeypatch.setenv("SKL_TILE32_MIN", "0")
    gpu_ctx.reload_env()
    o, g = oracle.Sketches(bins, n, kmers, ss64), gpu_ctx.sketches(bins, n, kmers, ss64)
    p = g.set_k(21)
    exp = oracle.self_dists_knn(o, knn, oracle.JACCARD, 1, False, ties=oracle.TIES_RUST_HEAP, threads=8)
    left_early = {}
    for form in ("decoupled", "travelling"):
        before = gpu_ctx.knn_prune_stats()
        got = _run(skl, gpu_ctx, g, p, knn, band_rows, world, form, False)
        after = gpu_ctx.knn_prune_stats()
        _assert_exact(got, exp, False)
        left_early[form] = (after[0] - before[0], after[1] - before[1])
    assert all(pruned > 0 for _tiles, pruned in left_early.values()), left_early
    g.close()


# ---- 2c. the early break below col_lo under logs ----

def _mixed(n, kmers, ss64, n_random, seed):
    u = synth.set_u(n_random, len(kmers), ss64, seed=synth.SEED_U + seed)
    r = synth.set_r(n - n_random, kmers, ss64, n_clusters=3, seed=synth.SEED_R + seed)
    return np.ascontiguousarray(np.concatenate([u, r], axis=0))


@pytest.mark.ab_library
@pytest.mark.parametrize("form", ["decoupled", "travelling"])
@pytest.mark.parametrize("lengths", [2, 3, 4])
@pytest.mark.parametrize("ss64", [64, 256])
def test_forced_early_break_below_col_lo(oracle, skl, gpu_ctx, set_switch, ss64, lengths, form):
    """Core/accessory keys, SKL_EARLY_BREAK = 2 / 3 / 4 (A/B build): the bands >= 1 take the early-break epilogue, also on the
    participants whose window starts above the band -- whose own rows, under logs, start EMPTY there (the flag that lets
    (1, 1) pairs mark nothing covers the turned rows only; the own rows' test is their own threshold).  Lists = the oracle's."""
    kmers, n, knn, band_rows, world = [15, 19, 23, 27, 31], 330, 7, 64, 3
    bins = _mixed(n, kmers, ss64, n_random=n - 30, seed=31)
    o, g = oracle.Sketches(bins, n, kmers, ss64), gpu_ctx.sketches(bins, n, kmers, ss64)
    set_switch("SKL_EARLY_BREAK", lengths)
    below = []

    def on_call(r, lo, hi, band, name):
        if lo > 0 and band >= 1 and (band + 1) * band_rows <= lo:
            below.append(name)

    got = _run(skl, gpu_ctx, g, g.set_k(), knn, band_rows, world, form, True, on_call=on_call)
    exp = oracle.self_dists_knn(o, knn, oracle.COREACC, 0, False, ties=oracle.TIES_RUST_HEAP, threads=8)
    _assert_exact(got, exp, True)
    assert below and all("early break: %d of 5" % lengths in name for name in below), below[:2]
    g.close()


# ---- 2d. a completeness vector ----

@pytest.mark.parametrize("form", ["travelling", "decoupled"])
@pytest.mark.parametrize("dist", ["jaccard", "coreacc"])
def test_completeness_vector(oracle, skl, gpu_ctx, form, dist):
    """Completeness in (0, 1], some exactly 1: ids exact, distances within 1e-6 of the oracle."""
    n, ss64, knn, band_rows, world = 300, 8, 6, 48, 3
    bins = _data(n, KMERS, ss64, seed=41)
    comp = np.random.default_rng(5).uniform(0.45, 1.0, n)
    comp[::5] = 1.0
    o, g = oracle.Sketches(bins, n, KMERS, ss64, completeness=comp), gpu_ctx.sketches(bins, n, KMERS, ss64, completeness=comp)
    p, oargs, coreacc, _ani = _key(g, oracle, dist, KMERS)
    idx, d0, d1 = _run(skl, gpu_ctx, g, p, knn, band_rows, world, form, coreacc)
    exp = oracle.self_dists_knn(o, knn, *oargs, ties=oracle.TIES_RUST_HEAP, threads=8)
    assert np.array_equal(idx.astype(np.uint64), exp["idx"]), np.argwhere(idx.astype(np.uint64) != exp["idx"])[:5]
    np.testing.assert_allclose(d0, exp["d0"], atol=1e-6, rtol=0)
    if coreacc:
        np.testing.assert_allclose(d1, exp["d1"], atol=1e-6, rtol=0)
    assert (comp < 1.0).sum() > n // 2
    g.close()


# ---- 2e. logs that overflow ----

@pytest.mark.parametrize("coreacc", [False, True])
@pytest.mark.parametrize("knn,cap", [(20, 24), (300, 310)], ids=["one-wave", "workgroup"])
def test_log_capacity(oracle, skl, gpu_ctx, knn, cap, coreacc):
    """A log shorter than what the busiest row takes: every row's length counts on past the capacity and equals the ample run's,
    the first `cap` records and ids are the ample run's prefix bit for bit, the heaps are the same, and the row after the last
    one -- a sentinel -- is untouched.  The one-wave heap form (knn <= 256) and the one-workgroup form."""
    import torch

    n, ss64, band_rows, world = 700, 16, 64, 3
    kmers = [15, 19, 23, 27, 31]
    bins = synth.set_r(n, kmers, ss64, n_clusters=4)
    bins[40] = bins[7]
    bins[400] = bins[7]
    g = gpu_ctx.sketches(bins, n, kmers, ss64)
    p = g.set_k() if coreacc else g.set_k(23)
    dev = _device()
    over = 0
    for lo, hi, bands in _windows(n, band_rows, world):
        runs = []
        for c in (n, cap):
            heaps, lg = skl.knn_heaps_alloc(n, knn, coreacc, dev), skl.knn_logs_alloc(n + 1, c, coreacc, dev)
            lg["rec"][n].fill_(float("nan"))
            lg["id"][n].fill_(-0x21524111)          # 0xDEADBEEF
            lg["len"][n] = 0x5A5A5A5A
            _sync(gpu_ctx)
            for band in bands:
                skl.self_dists_knn_window_logged(gpu_ctx, g, p, knn, band_rows, band, lo, hi, heaps, lg)
            _sync(gpu_ctx)
            runs.append((heaps, lg))
        (h_a, ample), (h_s, small) = runs
        assert int(ample["len"][:n].max()) < n
        assert torch.equal(small["len"][:n], ample["len"][:n])
        assert torch.equal(small["rec"][:n].view(torch.int32), ample["rec"][:n, :cap].view(torch.int32))
        assert torch.equal(small["id"][:n], ample["id"][:n, :cap])
        for k in h_a:
            if h_a[k] is not None:
                assert torch.equal(h_a[k].view(torch.int32), h_s[k].view(torch.int32)), k
        for lg in (ample, small):
            assert torch.isnan(lg["rec"][n]).all() and bool((lg["id"][n] == -0x21524111).all()) and int(lg["len"][n]) == 0x5A5A5A5A
        over += int((small["len"][:n] > cap).sum())
    assert over > 0, "some row's log is meant to overflow"
    g.close()


# ---- 2f. the replay's contract ----

@pytest.mark.parametrize("knn", [5, 300])
def test_replay_clamps_lengths_to_the_capacity(skl, gpu_ctx, knn):
    """skl_knn_heaps_replay reads min(lens[row], cap) entries of a row: lengths past the capacity replay like lengths equal to
    it; rows of length zero leave their heaps as they are (empty ones empty)."""
    import torch

    n, kmers, ss64, band_rows = 700, [15, 19, 23, 27, 31], 16, 64
    bins = synth.set_r(n, kmers, ss64, n_clusters=4)
    g = gpu_ctx.sketches(bins, n, kmers, ss64)
    p = g.set_k(23)
    dev = _device()
    heaps, lg = skl.knn_heaps_alloc(n, knn, False, dev), skl.knn_logs_alloc(n, n, False, dev)
    _sync(gpu_ctx)
    for band in range((n + band_rows - 1) // band_rows):
        skl.self_dists_knn_window_logged(gpu_ctx, g, p, knn, band_rows, band, 0, n, heaps, lg)
    _sync(gpu_ctx)
    lens = lg["len"].clone()
    cap = (int(lens.min()) + int(lens.max())) // 2
    assert int((lens > cap).sum()) > 0 and int(((lens > 0) & (lens < cap)).sum()) > 0
    rec, ids = lg["rec"][:, :cap].contiguous(), lg["id"][:, :cap].contiguous()
    clamped = torch.minimum(lens, torch.full_like(lens, cap))
    huge = torch.where(lens > cap, torch.full_like(lens, 2 ** 31 - 1), lens)
    out = []
    for ln in (lens.contiguous(), clamped.contiguous(), huge.contiguous()):
        h = skl.knn_heaps_alloc(n, knn, False, dev)
        _sync(gpu_ctx)
        skl.knn_heaps_replay(gpu_ctx, h, 0, n, knn, rec, ids, ln)
        _sync(gpu_ctx)
        out.append(h)
    for h in out[1:]:
        for k in ("h_key", "h_id", "h_len", "thr"):
            assert torch.equal(out[0][k].view(torch.int32), h[k].view(torch.int32)), k
    assert int(out[1]["h_len"].max()) > 0
    # zero-length rows: empty heaps stay empty, filled ones stay as they are
    empty = skl.knn_heaps_alloc(n, knn, False, dev)
    zero = torch.zeros_like(lens)
    filled = {k: (v.clone() if v is not None else None) for k, v in out[1].items()}
    _sync(gpu_ctx)
    skl.knn_heaps_replay(gpu_ctx, empty, 0, n, knn, rec, ids, zero)
    skl.knn_heaps_replay(gpu_ctx, out[1], 0, n, knn, rec, ids, zero)
    _sync(gpu_ctx)
    assert int(empty["h_len"].abs().sum()) == 0 and bool((empty["thr"] == -1).all())
    for k in ("h_key", "h_id", "h_len", "thr"):
        assert torch.equal(filled[k].view(torch.int32), out[1][k].view(torch.int32)), k
    g.close()


# ---- 2g. the drivers in-process ----

@pytest.mark.parametrize("band_rows", [None, 48])
@pytest.mark.parametrize("dist", ["jaccard", "coreacc"])
def test_drivers_in_process_with_one_rank(oracle, skl, dist, band_rows):
    """multi_gpu.self_knn_once_reference and self_knn_once_reference_decoupled with world 1 and no process group, on the library's
    own calls and a context on torch's stream (as scripts/bench_knn_multi.py makes it): the oracle's lists; a log of 2 entries
    cannot hold what a heap of 7 takes, and the decoupled driver says so with None."""
    import torch

    n, ss64, knn = 300, 8, 7
    bins = _data(n, KMERS, ss64, seed=51)
    dev = _device()
    ctx = skl.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    try:
        o, g = oracle.Sketches(bins, n, KMERS, ss64), ctx.sketches(bins, n, KMERS, ss64)
        p, oargs, coreacc, _ani = _key(g, oracle, dist, KMERS)
        exp = oracle.self_dists_knn(o, knn, *oargs, ties=oracle.TIES_RUST_HEAP, threads=8)
        res = multi_gpu.self_knn_once_reference(ctx, g, p, knn, 0, 1, None, dev, band_rows=band_rows)
        assert res[:2] == (0, n)
        _assert_exact(tuple(t.cpu().numpy() if t is not None else None for t in res[2:]), exp, coreacc)
        res = multi_gpu.self_knn_once_reference_decoupled(ctx, g, p, knn, 0, 1, None, dev, band_rows=band_rows)
        assert res is not None and res[:2] == (0, n)
        _assert_exact(tuple(t.cpu().numpy() if t is not None else None for t in res[2:]), exp, coreacc)
        assert multi_gpu.self_knn_once_reference_decoupled(ctx, g, p, knn, 0, 1, None, dev, band_rows=band_rows, log_cap=2) is None
        g.close()
    finally:
        torch.cuda.synchronize()
        ctx.close()
