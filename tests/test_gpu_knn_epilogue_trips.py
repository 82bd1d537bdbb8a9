"""The kNN bands' early-break epilogue (coreacc_epilogue_knn_kernel) at the edges of its trips.  The kernel's form follows the
sketch size -- <1> up to 32 chunks, <2> up to 64, <0> beyond -- and a wave reads a slice in trips of 64 half chunks (32 chunks):
16 chunks half fill the single trip, 32 fill it, 33 put two half chunks into a second one, 64 fill two, 65 is the smallest
size of the any-size form.  Every case completes pairs (relatives among random sketches, two of five lengths counted), in
the row-major order and, at 33 chunks, in the column-group-major one: ids, order and both distances are the oracle's."""
import numpy as np
import pytest

from helpers import mixed

pytestmark = pytest.mark.gpu

KMERS = [15, 19, 23, 27, 31]
N, N_RANDOM, KNN, BAND_ROWS = 330, 300, 7, 64
CASES = [(16, 0), (32, 0), (33, 0), (64, 0), (65, 0), (33, 2)]


@pytest.mark.ab_library
@pytest.mark.parametrize("ss64,order", CASES)
def test_knn_band_epilogue_trip_boundaries(oracle, skl, gpu_ctx, set_switch, ss64, order):
    bins = mixed(N, KMERS, ss64, n_random=N_RANDOM, n_clusters=3, seed=29)
    o, g = oracle.Sketches(bins, N, KMERS, ss64), gpu_ctx.sketches(bins, N, KMERS, ss64)
    exp = oracle.self_dists_knn(o, KNN, oracle.COREACC, ties=oracle.TIES_CANONICAL, threads=8)
    # (the data does what the test is about: some neighbour passed a completed length and took the fit with extended counts)
    assert ((exp["d0"] != 1.0) | (exp["d1"] != 1.0)).any()
    set_switch("SKL_KNN_BAND_ROWS", BAND_ROWS)
    set_switch("SKL_KNN_EPI_BLOCKED", order)
    set_switch("SKL_EARLY_BREAK", 2)
    before = gpu_ctx.early_break_stats()
    idx, d0, d1 = skl.self_dists_knn(gpu_ctx, g, g.set_k(), KNN)
    after = gpu_ctx.early_break_stats()
    g.close()
    assert "early break: 2 of 5" in gpu_ctx.last_kernel(), gpu_ctx.last_kernel()
    assert after[0] > before[0] and after[1] > before[1], (before, after)   # pairs went through the epilogue, and some were completed
    assert np.array_equal(idx, exp["idx"]), np.argwhere(idx != exp["idx"])[:5]
    assert np.array_equal(d0.view(np.uint32), exp["d0"].view(np.uint32)) and np.array_equal(d1.view(np.uint32), exp["d1"].view(np.uint32))
