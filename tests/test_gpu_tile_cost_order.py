"""Tiles dealt by cost (csrc/work_map.hpp plan_tile_numbering_by_cost / lookup_tile_by_cost_at): a self-mode k-sliced counts
launch of 16 x 128 tiles gives every XCD a share of its full tiles and then a share of its half tiles, instead of one
contiguous share of all of them.  tests/test_work_map_cost_cpu.py checks the map on the CPU; here the kernel runs in that order.

Every case compares the whole output with the oracle bit for bit, with SKL_TILE_COST_ORDER=1 (wherever the form allows) and =0.
Five k-mer lengths, 4 096 bins.  n = 65: one column group; 129, 193, 257, 413, 900: an odd number of 64-column blocks (the last
group's tiles are all half tiles); 193, 257, 413: an odd number of groups; 257: the first size at which the early break is
decided; 413, 520, 900: more than one round of workgroups.  Set U gives early-break launches (2 of 5 lengths counted), Set R
with a few clusters counts all five.  A launch takes the order unless its early break was decided block by block (those tiles
go to the XCDs in turns) or the library is told of a single XCD; every case asserts the marker in last_kernel() accordingly."""
import numpy as np
import pytest

from sketchlib.rust_amd import synth

pytestmark = pytest.mark.gpu

KMERS = [15, 19, 23, 27, 31]
SS64 = 64
MARK = "[tiles dealt by cost, half tiles last]"
SIZES = [65, 129, 193, 257, 413, 520, 900]

_REF = {}


def _case(oracle, data, n):
    """(bins, expected core/accessory matrix, expected bin-match counts), once per (data set, n), read-only."""
    if (data, n) not in _REF:
        bins = synth.set_u(n, len(KMERS), SS64) if data == "U" else synth.set_r(n, KMERS, SS64, n_clusters=max(3, n // 60))
        o = oracle.Sketches(bins, n, KMERS, SS64)
        dists = oracle.self_dists_all(o, threads=8)
        same = oracle.self_binmatch(o, threads=8)
        dists.setflags(write=False)
        same.setflags(write=False)
        _REF[(data, n)] = (bins, dists, same)
    return _REF[(data, n)]


def _order(gpu_ctx, monkeypatch, order, xcds=None):
    monkeypatch.setenv("SKL_TILE_COST_ORDER", order)
    if xcds is not None:
        monkeypatch.setenv("SKL_XCDS", str(xcds))
    gpu_ctx.reload_env()


def _marker(gpu_ctx, order, xcds=8):
    name = gpu_ctx.last_kernel()
    assert "pair_kernel_kslice<R=16, JL=2, COUNTS, k-sliced" in name, name
    takes = order == "1" and xcds > 1 and "block by block" not in name
    assert (MARK in name) == takes, name
    return takes


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("order", ["1", "0"])
@pytest.mark.parametrize("data", ["U", "R"])
@pytest.mark.parametrize("n", SIZES)
def test_all_pairs_rows_and_counts(oracle, skl, gpu_ctx, monkeypatch, n, data, order):
    bins, dists, same = _case(oracle, data, n)
    _order(gpu_ctx, monkeypatch, order)
    g = gpu_ctx.sketches(bins, n, KMERS, SS64)
    got = skl.self_dists_all(gpu_ctx, g, g.set_k())
    _marker(gpu_ctx, order)
    assert np.array_equal(_bits(got), _bits(dists))
    if n - 50 > 37:   # a band in the middle of the triangle (n = 65 has none)
        r0, r1 = 37, n - 50
        lo, cnt = skl.self_pairs(n, 0, r0), skl.self_pairs(n, r0, r1)
        part = skl.self_dists_rows(gpu_ctx, g, g.set_k(), r0, r1)
        _marker(gpu_ctx, order)
        assert part.shape[0] == cnt and np.array_equal(_bits(part), _bits(dists[lo:lo + cnt]))
    counts = skl.self_binmatch(gpu_ctx, g)
    assert _marker(gpu_ctx, order) == (order == "1")
    assert np.array_equal(counts, same)
    g.close()


@pytest.mark.parametrize("xcds", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [193, 520])
def test_fewer_xcds(oracle, skl, gpu_ctx, monkeypatch, n, xcds):
    """SKL_XCDS = 1 / 2 / 4 / 8: the shares of 1 (the present order: nothing to deal), 2, 4 and 8 XCDs."""
    bins, dists, same = _case(oracle, "U", n)
    _order(gpu_ctx, monkeypatch, "1", xcds)
    g = gpu_ctx.sketches(bins, n, KMERS, SS64)
    got = skl.self_dists_all(gpu_ctx, g, g.set_k())
    assert _marker(gpu_ctx, "1", xcds) == (xcds > 1)
    assert np.array_equal(_bits(got), _bits(dists))
    counts = skl.self_binmatch(gpu_ctx, g)
    assert _marker(gpu_ctx, "1", xcds) == (xcds > 1)
    assert np.array_equal(counts, same)
    g.close()


def test_both_orders_agree_byte_for_byte(oracle, skl, gpu_ctx, monkeypatch):
    bins, dists, _ = _case(oracle, "U", 900)
    g = gpu_ctx.sketches(bins, 900, KMERS, SS64)
    out = {}
    for order in ("0", "1"):
        _order(gpu_ctx, monkeypatch, order)
        out[order] = skl.self_dists_all(gpu_ctx, g, g.set_k())
        assert _marker(gpu_ctx, order) == (order == "1")
    assert out["0"].tobytes() == out["1"].tobytes()
    g.close()
