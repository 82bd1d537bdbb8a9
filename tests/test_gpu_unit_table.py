"""The unit table (csrc/unit_table.hpp): a k-sliced launch of the chunk-split kernel reads what each of its workgroups computes
-- tile, k-mer length, chunk range, half-tile case, flags -- from one 16-byte descriptor per workgroup that the host built once
for the launch's shape, instead of decoding its workgroup index at the kernel's head.  tests/test_unit_table_cpu.py checks the
table against the decode on the CPU; here the kernel runs from it.

Every case runs with the table forced on wherever the form allows (skl_ctx_set_unit_table(ctx, 1), "1" below) and with the decode
in the kernel (0) and compares the whole output with the oracle bit for bit; skl_ctx_unit_table() must say which path the last
pair launch took: the table exactly when the launch was a k-sliced one (", k-sliced" in last_kernel(); the all-k form and the
small-launch fallback have no table).
Five k-mer lengths, 4 096 bins unless a case says otherwise.  Sizes: 2 and 17 below one tile; 65 one column group; 129, 193, 257,
413, 900 an odd number of 64-column blocks; 257 the first size with an early-break decision; 413 and 900 more than one round of
workgroups.  Set U gives early-break launches (2 of 5 lengths counted, tail-sliced), Set R counts all five."""
import numpy as np
import pytest

from sketchlib.rust_amd import synth

pytestmark = pytest.mark.gpu

KMERS = [15, 19, 23, 27, 31]
SS64 = 64
SIZES = [2, 17, 65, 129, 193, 257, 413, 900]

_REF = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _case(oracle, data, n, ss64=SS64):
    """(bins, oracle handle, core/accessory matrix, bin-match counts), once per (data set, n, sketch size), read-only."""
    key = (data, n, ss64)
    if key not in _REF:
        bins = synth.set_u(n, len(KMERS), ss64) if data == "U" else synth.set_r(n, KMERS, ss64, n_clusters=max(3, n // 60))
        o = oracle.Sketches(bins, n, KMERS, ss64)
        dists, same = _frozen(oracle.self_dists_all(o, threads=8), oracle.self_binmatch(o, threads=8))
        _REF[key] = (bins, o, dists, same)
    return _REF[key]


@pytest.fixture(autouse=True)
def _by_rule_afterwards(gpu_ctx):
    """The session's context goes back to the library's rule after every test here."""
    yield
    gpu_ctx.set_unit_table(-1)


def _table(gpu_ctx, monkeypatch, table, **switches):
    for name, value in switches.items():
        monkeypatch.setenv(name, str(value))
    gpu_ctx.reload_env()
    gpu_ctx.set_unit_table(int(table))


def _path(gpu_ctx, table):
    """The accessor says which path the last pair launch took; returns whether it read a table."""
    name = gpu_ctx.last_kernel()
    used = gpu_ctx.unit_table()[0]
    assert used == (table == "1" and ", k-sliced" in name and "segments of" not in name), (table, used, name)
    return used


@pytest.mark.parametrize("table", ["1", "0"])
@pytest.mark.parametrize("data", ["U", "R"])
@pytest.mark.parametrize("n", SIZES)
def test_all_pairs_a_row_band_cross_and_counts(oracle, skl, gpu_ctx, monkeypatch, n, data, table):
    bins, o, dists, same = _case(oracle, data, n)
    _table(gpu_ctx, monkeypatch, table)
    g = gpu_ctx.sketches(bins, n, KMERS, SS64)
    got = skl.self_dists_all(gpu_ctx, g, g.set_k())
    used = _path(gpu_ctx, table)
    assert np.array_equal(_bits(got), _bits(dists))
    if n - 50 > 37:   # a band in the middle of the triangle
        r0, r1 = 37, n - 50
        lo, cnt = skl.self_pairs(n, 0, r0), skl.self_pairs(n, r0, r1)
        part = skl.self_dists_rows(gpu_ctx, g, g.set_k(), r0, r1)
        _path(gpu_ctx, table)
        assert part.shape[0] == cnt and np.array_equal(_bits(part), _bits(dists[lo:lo + cnt]))
    counts = skl.self_binmatch(gpu_ctx, g)
    used |= _path(gpu_ctx, table)
    assert np.array_equal(counts, same)
    if n >= 17:   # cross mode, nA != nB: the first third of the samples against all of them
        na = n // 3 + 1
        key = ("cross", data, n)
        if key not in _REF:
            _REF[key] = _frozen(oracle.cross_dists_all(oracle.Sketches(bins[:na], na, KMERS, SS64), o, oracle.COREACC, threads=8))[0]
        g_a = gpu_ctx.sketches(bins[:na], na, KMERS, SS64)
        cross = skl.cross_dists_all(gpu_ctx, g_a, g, g.set_k())
        used |= _path(gpu_ctx, table)
        assert np.array_equal(_bits(cross), _bits(_REF[key]))
        g_a.close()
    if n >= 65:
        assert used == (table == "1")   # (from one column group on some launch of the case is k-sliced)
    g.close()


@pytest.mark.parametrize("table", ["1", "0"])
@pytest.mark.parametrize("n,ss64,sliced", [(200, 64, True), (1300, 64, False), (1300, 32, False)])
def test_single_k_and_a_sketch_of_32_chunks(oracle, skl, gpu_ctx, monkeypatch, n, ss64, sliced, table):
    """Single-k Jaccard at 200 samples (counts in tail slices + an epilogue) and at 1 300 (the single-k form itself, not sliced);
    2 048 bins at 1 300 samples: core/accessory counts launches that are not tail-sliced -- whole units, wave priority by round.
    (The library's rule slices the last round of every launch below 0.9 rounds of workgroups, single-k up to ~1 900 samples:
    the cases that are not sliced run with SKL_TAIL_SLICES=0.)"""
    bins, o, dists, _ = _case(oracle, "U", n, ss64)
    _table(gpu_ctx, monkeypatch, table, **({} if sliced else {"SKL_TAIL_SLICES": 0}))
    g = gpu_ctx.sketches(bins, n, KMERS, ss64)
    key = ("jaccard", n, ss64)
    if key not in _REF:
        _REF[key] = _frozen(oracle.self_dists_all(o, oracle.JACCARD, 2, threads=8))[0]
    got = skl.self_dists_all(gpu_ctx, g, g.set_k(KMERS[2]))
    assert _path(gpu_ctx, table) == (table == "1")
    assert ("chunk slices per unit" in gpu_ctx.last_kernel()) == sliced, gpu_ctx.last_kernel()
    assert np.array_equal(_bits(got), _bits(_REF[key]))
    if ss64 == 32:
        got = skl.self_dists_all(gpu_ctx, g, g.set_k())
        assert _path(gpu_ctx, table) == (table == "1")
        assert "chunk slices per unit" not in gpu_ctx.last_kernel(), gpu_ctx.last_kernel()
        assert np.array_equal(_bits(got), _bits(dists))
    g.close()


@pytest.mark.parametrize("table", ["1", "0"])
def test_a_plan_decided_block_by_block(oracle, skl, gpu_ctx, monkeypatch, table):
    """A database that is half one species: the early break is decided per block of 256 x 256 sample ids, the tiles go to the XCDs in
    turns, and a (tile, k index) whose block wants fewer lengths is `none` in the table as it returns at once in the kernel."""
    key = ("species",)
    if key not in _REF:
        bins = np.ascontiguousarray(np.concatenate([synth.set_r(512, KMERS, 16, n_clusters=1, seed=synth.SEED_R + 31),
                                                    synth.set_u(512, len(KMERS), 16, seed=synth.SEED_U + 132)], axis=0))
        o = oracle.Sketches(bins, 1024, KMERS, 16)
        _REF[key] = (bins,) + _frozen(oracle.self_dists_all(o, threads=8))
    bins, dists = _REF[key]
    _table(gpu_ctx, monkeypatch, table)
    g = gpu_ctx.sketches(bins, 1024, KMERS, 16)
    got = skl.self_dists_all(gpu_ctx, g, g.set_k())
    assert gpu_ctx.early_break_blocks()["mixed"] and "block by block" in gpu_ctx.last_kernel(), gpu_ctx.last_kernel()
    assert _path(gpu_ctx, table) == (table == "1")
    assert np.array_equal(_bits(got), _bits(dists))
    g.close()


@pytest.mark.parametrize("order", ["0", "1"])
@pytest.mark.parametrize("xcds", [1, 2, 4])
@pytest.mark.parametrize("n", [193, 413])
def test_fewer_xcds_and_both_tile_orders(oracle, skl, gpu_ctx, monkeypatch, n, xcds, order):
    bins, _, dists, same = _case(oracle, "U", n)
    g = gpu_ctx.sketches(bins, n, KMERS, SS64)
    for table in ("1", "0"):
        _table(gpu_ctx, monkeypatch, table, SKL_XCDS=xcds, SKL_TILE_COST_ORDER=order)
        got = skl.self_dists_all(gpu_ctx, g, g.set_k())
        assert _path(gpu_ctx, table) == (table == "1")
        assert ("[tiles dealt by cost, half tiles last]" in gpu_ctx.last_kernel()) == (order == "1" and xcds > 1)
        assert np.array_equal(_bits(got), _bits(dists))
        counts = skl.self_binmatch(gpu_ctx, g)
        assert _path(gpu_ctx, table) == (table == "1")
        assert np.array_equal(counts, same)
    g.close()


def test_cache_hit_miss_and_eviction(oracle, skl, gpu_ctx, monkeypatch):
    """Five launches of different shapes in one context, then the first shape again: the context keeps four tables, so the first
    shape's was evicted and is built anew; a shape repeated at once is a hit.  All against the oracle.  The library's default
    (skl_ctx_set_unit_table(ctx, -1)): the dense calls' launches take the table."""
    gpu_ctx.set_unit_table(-1)
    n = 413
    bins, _, dists, _ = _case(oracle, "U", n)
    g = gpu_ctx.sketches(bins, n, KMERS, SS64)

    def band(r0, r1):
        lo, cnt = skl.self_pairs(n, 0, r0), skl.self_pairs(n, r0, r1)
        _, hits, builds = gpu_ctx.unit_table()
        part = skl.self_dists_rows(gpu_ctx, g, g.set_k(), r0, r1)
        used, hits2, builds2 = gpu_ctx.unit_table()
        assert used, gpu_ctx.last_kernel()
        assert np.array_equal(_bits(part), _bits(dists[lo:lo + cnt]))
        return hits2 - hits, builds2 - builds

    shapes = [(0, n), (16, n - 20), (37, n - 50), (64, 300), (100, 400)]
    assert band(*shapes[0]) in ((0, 1), (1, 0))                         # (the session's context may have met the shape before)
    assert band(*shapes[0]) == (1, 0)                                   # the same shape: a hit
    for s in shapes[1:]:
        band(*s)
    for s in shapes[1:]:
        assert band(*s) == (1, 0)                                       # the last four shapes: all kept
    assert band(*shapes[0]) == (0, 1)                                   # the first one was evicted: built anew
    assert band(*shapes[4]) == (1, 0) and band(*shapes[0]) == (1, 0)
    g.close()
