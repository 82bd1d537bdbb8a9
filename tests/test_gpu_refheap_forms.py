"""The heap-replay kernels (csrc/topk.hip) in both forms -- one wave per row (SKL_REFHEAP_WAVE=1, the default up to 256
neighbours) and one workgroup per row (SKL_REFHEAP_WAVE=0; what more than 256 neighbours take anyway) -- at the shapes
where what the forms share can go wrong: knn around the form boundary, rows around the trip sizes of the two feeds
(64 x 4 and 256 x 4 records), a heap that stays open to the last candidate, the accept log, ragged one-shot rows.  Each
form must give the oracle's TIES_RUST_HEAP lists exactly: ids, order and distances, every row."""
import numpy as np
import pytest

from sketchlib.rust_amd import synth
from test_gpu_precluster import as_pairs, candidates, oracle_pairs

pytestmark = [pytest.mark.gpu, pytest.mark.ab_library]

WAVE = ["1", "0"]
_SHARED = {}


def shared(key, make):
    """Inputs and the oracle's lists of one case: computed once, used by both forms, never written to."""
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


def self_case(oracle, bins, n, kmers, ss64, knn, coreacc):
    o = oracle.Sketches(bins, n, kmers, ss64)
    oargs = (oracle.COREACC, 0, False) if coreacc else (oracle.JACCARD, len(kmers) // 2, False)
    return bins, oracle.self_dists_knn(o, knn, *oargs, ties=oracle.TIES_RUST_HEAP, threads=8)


def oracle_candidate_counts(oracle, bins, skq, kmers, ss64):
    """How many candidates the oracle lists for each row: its precluster lists at knn = n - 1 hold every candidate of a row,
    and behind them the padding (row, 1.0) -- a row is never its own candidate."""
    n = skq.shape[0]
    full = oracle.self_dists_knn_precluster(oracle.Sketches(bins, n, kmers, ss64), skq, n - 1, 0, False, ties=oracle.TIES_RUST_HEAP, threads=8)
    return (full["idx"] != np.arange(n)[:, None]).sum(axis=1)


def check_self(skl, ctx, bins, exp, n, kmers, ss64, knn, coreacc):
    g = ctx.sketches(bins, n, kmers, ss64)
    idx, d0, d1 = skl.self_dists_knn(ctx, g, g.set_k() if coreacc else g.set_k(kmers[len(kmers) // 2]), knn)
    g.close()
    assert np.array_equal(idx, exp["idx"]), np.argwhere(idx != exp["idx"])[:5]
    assert np.array_equal(d0.view(np.uint32), exp["d0"].view(np.uint32))
    if coreacc:
        assert np.array_equal(d1.view(np.uint32), exp["d1"].view(np.uint32))


@pytest.mark.parametrize("wave", WAVE)
@pytest.mark.parametrize("coreacc", [False, True])
@pytest.mark.parametrize("knn", [1, 255, 256, 257])
def test_knn_at_the_form_boundary(oracle, skl, gpu_ctx, set_switch, knn, coreacc, wave):
    """256 neighbours are the most one wave per row holds, 257 run one workgroup per row whatever the switch says.  Bands of
    37 rows: every pair once, each band's turned merges (one mark per 32 records) and own merge (per 64)."""
    kmers, ss64, n = [17, 21, 25, 29], 4, 600
    bins, exp = shared(("boundary", knn, coreacc),
                       lambda: self_case(oracle, synth.set_r(n, kmers, ss64, n_clusters=40), n, kmers, ss64, knn, coreacc))
    set_switch("SKL_KNN_BAND_ROWS", 37)
    set_switch("SKL_REFHEAP_WAVE", wave)
    gpu_ctx.set_knn_ties(skl.TIES_REFERENCE)
    check_self(skl, gpu_ctx, bins, exp, n, kmers, ss64, knn, coreacc)


@pytest.mark.parametrize("wave", WAVE)
@pytest.mark.parametrize("band", [None, 37])
@pytest.mark.parametrize("n", [65, 257, 1025, 1100])
def test_row_lengths_around_the_trip_sizes(oracle, skl, gpu_ctx, set_switch, n, band, wave):
    """Rows of n records: one more than 64, than 64 x 4 and than 256 x 4, and 1 100 -- never a whole trip of either feed,
    the last mark word partly used.  Without a band height the rows go through the one-shot kernels (row by row, a whole row
    at once), in bands of 37 through the resumable ones."""
    kmers, ss64, knn = [21], 2, 7
    bins, exp = shared(("lengths", n), lambda: self_case(oracle, synth.set_r(n, kmers, ss64, n_clusters=9), n, kmers, ss64, knn, False))
    set_switch("SKL_KNN_BAND_ROWS", band)
    set_switch("SKL_REFHEAP_WAVE", wave)
    gpu_ctx.set_knn_ties(skl.TIES_REFERENCE)
    check_self(skl, gpu_ctx, bins, exp, n, kmers, ss64, knn, False)


@pytest.mark.parametrize("wave", WAVE)
@pytest.mark.parametrize("band", [None, 7])
def test_a_heap_that_stays_open_while_every_key_ties(oracle, skl, gpu_ctx, set_switch, band, wave):
    """Copies of one sketch.  Neither the library nor the reference takes more neighbours than the other n - 1 samples
    (skl_self_dists_knn rejects knn > n - 1), so the self kNN of n = 40 runs at knn = 39: the heap is open up to the row's
    last candidate and every trip drains at once (one-shot without a band height, resumable in bands of 7).  knn = 50 is
    the next test's."""
    kmers, ss64, n = [21], 4, 40
    bins = shared("tied bins", lambda: np.tile(synth.set_u(1, 1, ss64), (60, 1)))
    _, exp = shared("tied 39", lambda: self_case(oracle, bins[:n], n, kmers, ss64, n - 1, False))
    set_switch("SKL_KNN_BAND_ROWS", band)
    set_switch("SKL_REFHEAP_WAVE", wave)
    gpu_ctx.set_knn_ties(skl.TIES_REFERENCE)
    check_self(skl, gpu_ctx, bins[:n], exp, n, kmers, ss64, n - 1, False)


@pytest.mark.parametrize("wave", WAVE)
def test_an_open_heap_of_50_over_40_tied_samples(oracle, skl, gpu_ctx, set_switch, wave):
    """n = 40, knn = 50, every key tied, through the entry point that takes it: the candidate lists.  40 of 60 copies of one
    sketch list each other: 39 tied candidates a row, a heap that never fills, padding behind it; 20 rows list nothing."""
    kmers, ss64, n, knn = [21], 4, 40, 50
    bins = shared("tied bins", lambda: np.tile(synth.set_u(1, 1, ss64), (60, 1)))
    skq = (1000 + np.arange(60 * 3)).reshape(60, 3).astype(np.uint16)
    skq[:n] = 0                                      # one index sketch for 40 rows
    offs, cols = candidates(skq)
    assert np.array_equal(oracle_candidate_counts(oracle, bins, skq, kmers, ss64), [n - 1] * n + [0] * (60 - n))
    assert np.array_equal(np.diff(offs.astype(np.int64)), [n - 1] * n + [0] * (60 - n))
    exp = shared("tied 50", lambda: oracle.self_dists_knn_precluster(oracle.Sketches(bins, 60, kmers, ss64), skq, knn, 0, False,
                                                                     ties=oracle.TIES_RUST_HEAP, threads=8))
    set_switch("SKL_REFHEAP_WAVE", wave)
    gpu_ctx.set_knn_ties(skl.TIES_REFERENCE)
    g = gpu_ctx.sketches(bins, 60, kmers, ss64)
    idx, d0 = skl.self_dists_knn_candidates(gpu_ctx, g, g.set_k(21), knn, offs, cols)
    g.close()
    assert as_pairs(idx, d0) == oracle_pairs(exp)


@pytest.mark.parametrize("wave", WAVE)
@pytest.mark.parametrize("coreacc", [False, True])
def test_the_accept_log_of_two_windows_replayed(oracle, skl, gpu_ctx, set_switch, coreacc, wave):
    """skl_self_dists_knn_window_logged over two column windows, each against heaps that start empty, then
    skl_knn_heaps_replay of the two logs in window order (explicit candidate ids, a length per row) and the finalize step."""
    import torch
    from sketchlib.rust_amd import multi_gpu

    kmers, ss64, n, knn, band_rows, cap = [17, 21, 25, 29], 4, 300, 9, 64, 128

    def make():
        bins = synth.set_r(n, kmers, ss64, n_clusters=4)
        bins[40] = bins[7]
        bins[199] = bins[7]
        bins[200] = bins[7]
        return self_case(oracle, bins, n, kmers, ss64, knn, coreacc)

    bins, exp = shared(("log", coreacc), make)
    set_switch("SKL_REFHEAP_WAVE", wave)
    g = gpu_ctx.sketches(bins, n, kmers, ss64)
    p = g.set_k() if coreacc else g.set_k(kmers[len(kmers) // 2])
    dev = torch.device("cuda", 0)
    cuts = multi_gpu.knn_window_cuts(n, band_rows, 2)
    logs = []
    for r in range(2):
        heaps = skl.knn_heaps_alloc(n, knn, coreacc, dev)
        lg = skl.knn_logs_alloc(n, cap, coreacc, dev)
        for band in range((n + band_rows - 1) // band_rows):
            if band * band_rows >= cuts[r + 1]:
                break
            skl.self_dists_knn_window_logged(gpu_ctx, g, p, knn, band_rows, band, cuts[r], cuts[r + 1], heaps, lg)
        gpu_ctx.synchronize()
        assert int(lg["len"].max()) <= cap, "the test's logs are meant to hold"
        logs.append(lg)
    final = skl.knn_heaps_alloc(n, knn, coreacc, dev)
    for lg in logs:
        m = max(1, int(lg["len"].max()))
        rec, ids = lg["rec"][:, :m].contiguous(), lg["id"][:, :m].contiguous()
        torch.cuda.synchronize()      # (torch cuts the logs on ITS stream; the context runs on a stream of its own)
        skl.knn_heaps_replay(gpu_ctx, final, 0, n, knn, rec, ids, lg["len"])
        gpu_ctx.synchronize()
    idx, d0, d1 = skl.knn_heaps_finalize(gpu_ctx, final, 0, n, knn)
    gpu_ctx.synchronize()
    g.close()
    assert np.array_equal(idx.cpu().numpy().astype(np.uint64), exp["idx"]), np.argwhere(idx.cpu().numpy() != exp["idx"])[:5]
    assert np.array_equal(d0.cpu().numpy().view(np.uint32), exp["d0"].view(np.uint32))
    if coreacc:
        assert np.array_equal(d1.cpu().numpy().view(np.uint32), exp["d1"].view(np.uint32))


@pytest.mark.parametrize("wave", WAVE)
@pytest.mark.parametrize("knn", [10, 256])
def test_the_ragged_one_shot(oracle, skl, gpu_ctx, set_switch, knn, wave):
    """The precluster entry point: rows without a candidate (all padding), with fewer than knn (padded behind them) and
    with more than 256 (more than one trip of the wave feed), a third of the database one sketch (rows of ties)."""
    kmers, ss64, n = [17, 21, 25, 29], 2, 400

    def make():
        bins = synth.set_r(n, kmers, ss64, n_clusters=9)
        bins[::3] = bins[0]
        skq = (1000 + np.arange(n * 4)).reshape(n, 4).astype(np.uint16)     # no two rows share a bin ...
        skq[:300, 0] = 7                                                     # ... but these 300 (299 candidates each)
        skq[300:304, 1] = 9                                                  # ... and these 4 (3 each)
        exp = oracle.self_dists_knn_precluster(oracle.Sketches(bins, n, kmers, ss64), skq, knn, 1, False, ties=oracle.TIES_RUST_HEAP,
                                               threads=8)
        return bins, skq, exp, oracle_candidate_counts(oracle, bins, skq, kmers, ss64)

    bins, skq, exp, lens = shared(("ragged", knn), make)
    assert (lens == 0).any() and ((lens > 0) & (lens < knn)).any() and (lens > 256).any()
    offs, cols = candidates(skq)
    assert np.array_equal(np.diff(offs.astype(np.int64)), lens)      # the lists handed to the library are the oracle's, row by row
    set_switch("SKL_REFHEAP_WAVE", wave)
    gpu_ctx.set_knn_ties(skl.TIES_REFERENCE)
    g = gpu_ctx.sketches(bins, n, kmers, ss64)
    idx, d0 = skl.self_dists_knn_candidates(gpu_ctx, g, g.set_k(21), knn, offs, cols)
    g.close()
    assert as_pairs(idx, d0) == oracle_pairs(exp)
