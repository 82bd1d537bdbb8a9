"""skl_self_dists_hist / skl_cross_dists_hist (csrc/hist.hip, csrc/capi_hist.cpp): the histogram of the f32 values a dense
call stores, on a grid the caller gives, built on the GPU behind each dense band.

The expected histogram never comes from this library: it is the ORACLE's dense array (tests/test_gpu_dists_within.py: Space)
binned by np_hist() below, a numpy float32 restatement of the header's cell rule.  Without a completeness vector the stored
values are the oracle's bit for bit and the bar is identical counts, `outside` and `nan`.  With one, values may differ by up to
1e-6, so the grid is one where no oracle value changes its cell or its in/out status when moved by +-2e-6 in f32 (asserted on
the CPU before the GPU call), and the bar is identical counts again.

Chunk size and the LDS limit come from the native check of csrc/hist_plan.hpp (tests/test_hist_plan_cpu.py).  No whole self call
has exactly one chunk of pairs, so "one chunk, and one more" are row 0 of n = chunk + 1 and n = chunk + 2 samples.

NaN stored values cannot be produced through the public inputs (tests/test_gpu_dists_within.py documents this), so the rule
"a NaN is counted in outside[1]" rests on the native check; here nan == 0 is asserted wherever the oracle holds none."""
import ctypes as C

import numpy as np
import pytest

from sketchlib.rust_amd import synth
from test_gpu_dists_within import KMERS, SS64, caps_of, clustered, space
from test_hist_plan_cpu import consts as _plan_consts

pytestmark = pytest.mark.gpu

SENT = 0xDEADBEEFDEADBEEF
G8 = (0, 1, 8, 0, 1, 8)
G1 = (0, 1, 1, 0, 1, 1)
NARROW = (0, 0.1, 16, 0, 0.5, 4)


def consts():
    """(threads, chunk, LDS cells, cell limit, ...) from a plain (unsanitized) build of tests/native/hist_check.cpp."""
    return _plan_consts(sanitize=False)


def axes_of(grid, ncols):
    return [tuple(grid[:3])] + ([tuple(grid[3:6])] if ncols == 2 else [])


def axis_cells(v, lo, hi, n):
    """The header's cell rule for one column of f32 values -> (cell as int64, inside as bool); NaNs are the caller's."""
    lo, hi = np.float32(lo), np.float32(hi)
    scale = np.float32(np.float64(n) / (np.float64(hi) - np.float64(lo)))
    with np.errstate(invalid="ignore", over="ignore"):
        inside = ~((v < lo) | (v > hi)) & ~np.isnan(v)
        x = (np.where(inside, v, lo).astype(np.float32) - lo) * scale          # one f32 subtract, one f32 multiply
    assert x.dtype == np.float32
    c = np.minimum(np.minimum(x, np.float32(n)).astype(np.int64), n - 1)       # truncation, the last cell closed at hi
    return c, inside


def np_hist(d, grid):
    """-> (counts uint64 [n0] or [n0, n1], outside, nan) of f32 values d [positions, ncols]."""
    ncols = d.shape[1]
    axes = axes_of(grid, ncols)
    nan = np.isnan(d).any(axis=1)
    inside = np.ones(d.shape[0], dtype=bool)
    cell = np.zeros(d.shape[0], dtype=np.int64)
    for x, (lo, hi, n) in enumerate(axes):
        c, ok = axis_cells(d[:, x], lo, hi, n)
        inside &= ok | np.isnan(d[:, x])
        cell = cell * n + c
    keep = inside & ~nan
    cells = int(np.prod([a[2] for a in axes]))
    counts = np.bincount(cell[keep], minlength=cells).astype(np.uint64)
    return counts.reshape([a[2] for a in axes]), int((~inside & ~nan).sum()), int(nan.sum())


def expected(sp, grid, kmer=None, ani=False, r0=0, r1=None):
    if sp.n_cols == 0 or (not sp.query and sp.n < 2):
        ncols = 2 if kmer is None else 1
        return np.zeros([a[2] for a in axes_of(grid, ncols)], dtype=np.uint64), 0, 0
    a, b = sp.start(r0), sp.start(sp.n if r1 is None else r1)
    return np_hist(sp.dense(kmer, ani)[a:b], grid)


class Slabs:
    """The device slabs of a Space for the length of a `with`."""

    def __init__(self, sp, kmer=None, ani=False):
        self.sp, self.kmer, self.ani = sp, kmer, ani

    def __enter__(self):
        sp = self.sp
        self.g = sp.ctx.sketches(sp.bins, sp.n, sp.kmers, sp.ss64, completeness=sp.comp)
        self.q = sp.ctx.sketches(sp.query[0], sp.query[1], sp.kmers, sp.ss64, completeness=sp.query[2]) if sp.query else None
        self.p = self.g.set_k(self.kmer, self.ani, cutoff=sp.cutoff)
        return self

    def __exit__(self, *exc):
        self.g.close()
        if self.q is not None:
            self.q.close()


def run(sp, grid, kmer=None, ani=False, r0=0, r1=None, counts=None):
    with Slabs(sp, kmer, ani) as s:
        return sp.skl.dists_hist(sp.ctx, s.g, s.p, grid, r0, r1, query=s.q, counts=counts)


def raw(sp, s, grid, counts, outside, r0=0, r1=None, flags=0, on_device=0):
    """The C call as it is.  grid: a HistGrid, or None; counts / outside: numpy uint64 arrays, an address, or None."""
    lib = sp.skl.load()
    addr = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a      # noqa: E731
    r1 = sp.n if r1 is None else r1
    gp = C.byref(grid) if grid is not None else None
    if s.q is None:
        return lib.skl_self_dists_hist(sp.ctx._h, s.g._h, C.byref(s.p), r0, r1, gp, addr(counts), on_device, flags, addr(outside))
    return lib.skl_cross_dists_hist(sp.ctx._h, s.g._h, s.q._h, C.byref(s.p), r0, r1, gp, addr(counts), on_device, flags, addr(outside))


def check(sp, grid, kmer=None, ani=False, r0=0, r1=None, kernel=None):
    """The fresh call gives the oracle's histogram; -> (counts, outside, nan) as expected."""
    want, w_out, w_nan = expected(sp, grid, kmer, ani, r0, r1)
    got, g_out, g_nan = run(sp, grid, kmer, ani, r0, r1)
    pairs = sp.start(sp.n if r1 is None else r1) - sp.start(r0) if (sp.query or sp.n >= 2) else 0
    print(f"n={sp.n} cols={sp.n_cols} kmer={kmer} ani={ani} grid={grid} rows=({r0}, {r1}): {pairs} pairs, {int((want > 0).sum())} of {want.size} cells occupied, "
          f"largest {int(want.max())}, outside {w_out}, nan {w_nan}; got outside {g_out}, nan {g_nan}, sum {int(got.sum())}")
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert int(want.sum()) + w_out + w_nan == pairs                          # (the test's own arithmetic)
    assert np.array_equal(got, want) and g_out == w_out and g_nan == w_nan
    assert w_nan == 0
    name = sp.ctx.last_kernel()
    if pairs:
        which = kernel or ("hist_lds_kernel" if want.size <= consts()[2] else "hist_global_kernel")
        assert "skl::" + which in name and name.index("kernel") < name.index("skl::hist_"), name      # the dense kernel is named first
        assert ("hist_lds_kernel" in name) != ("hist_global_kernel" in name), name
    return want, w_out, w_nan


@pytest.fixture()
def sp65(oracle, skl, gpu_ctx):
    return space(oracle, skl, gpu_ctx, "sp65", clustered(65, 4))


def chunk_space(oracle, skl, gpu_ctx, extra):
    n = consts()[1] + extra
    return space(oracle, skl, gpu_ctx, ("chunk", n), clustered(n, 40))


def contended_space(oracle, skl, gpu_ctx):
    """tests/test_gpu_dists_within.py's clustered2200: 2 100 unrelated samples, then 100 copies of one."""
    def make():
        a = synth.set_r(2100, KMERS, SS64, n_clusters=2100)
        b = np.repeat(synth.set_r(1, KMERS, SS64, n_clusters=1, seed=synth.SEED_R + 5), 100, axis=0)
        return np.concatenate([a, b]), 2200, KMERS, SS64

    return space(oracle, skl, gpu_ctx, "clustered2200", make)


# ---- 1. small ----

@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_small(oracle, skl, gpu_ctx, n):
    sp = space(oracle, skl, gpu_ctx, ("small", n), clustered(n, 1 if n < 4 else 4))
    for grid in (G8, G1, NARROW):
        want, out, _nan = check(sp, grid)
        if n == 1:
            assert not want.any() and out == 0
    if n == 1:
        return
    for r0, r1 in ((0, 0), (n - 1, n - 1), (n, n), (n - 1, n)):       # empty ranges (the last row of a triangle holds no pair)
        want, out, _nan = check(sp, G8, r0=r0, r1=r1)
        assert not want.any() and out == 0
    if n == 65:
        d = sp.dense()
        assert int((d[:, 0] == np.float32(1.0)).sum()) == 1585
        want, out, _nan = expected(sp, NARROW)
        assert out >= 1585 and (want > 0).sum() > 1               # the pairs at a core distance of 1.0 are off the narrow grid


# ---- 2. one chunk and one more ----

@pytest.mark.parametrize("extra", [1, 2])
def test_one_chunk_and_one_more(oracle, skl, gpu_ctx, extra):
    chunk = consts()[1]
    sp = chunk_space(oracle, skl, gpu_ctx, extra)
    assert sp.start(1) - sp.start(0) == chunk + extra - 1
    for grid in (G8, NARROW):
        want, out, _nan = check(sp, grid, r0=0, r1=1)
        assert int(want.sum()) + out == chunk + extra - 1
    check(sp, G8, r0=sp.n - 3, r1=sp.n - 1)                       # the triangle's last two rows: 2 + 1 pairs
    check(sp, (0, 1, 64), kmer=21, r0=0, r1=1)                    # one column: four positions a load
    if extra == 2:
        want, _out, _nan = check(sp, G8)                          # the whole call: 1 026 chunks, every workgroup strides
        assert (want > 0).sum() > 2


# ---- 3. contended counters ----

def test_contended_counters(oracle, skl, gpu_ctx):
    sp = contended_space(oracle, skl, gpu_ctx)
    pairs = sp.i.size
    want, out, _nan = expected(sp, G8)
    assert out == 0 and int(want.max()) > 0.9 * pairs             # one cell holds nearly everything: (1, 1)
    assert int(want[0, 0]) >= 4950                                # the copies, at (0, 0)
    check(sp, G8)
    want, out, _nan = check(sp, G1)                               # every lane of every wave hits the one counter
    assert int(want[0, 0]) == pairs
    check(sp, (0, 1, 129, 0, 1, 128))                             # the same spikes through the global kernel
    check(sp, (0, 1, 1), kmer=21)


# ---- 4. both kernels at the boundary ----

@pytest.mark.parametrize("which", ["sp65", "chunk2"])
def test_both_kernels_at_the_boundary(oracle, skl, gpu_ctx, which):
    lds_cells, max_cells = consts()[2:4]
    assert lds_cells == 128 * 128 and max_cells == 1024 * 1024
    sp = space(oracle, skl, gpu_ctx, "sp65", clustered(65, 4)) if which == "sp65" else chunk_space(oracle, skl, gpu_ctx, 2)
    check(sp, (0, 1, 128, 0, 1, 128), kernel="hist_lds_kernel")
    check(sp, (0, 1, 128, 0, 1, 129), kernel="hist_global_kernel")
    check(sp, (0, 1, 129, 0, 1, 128), kernel="hist_global_kernel")
    check(sp, (0, 1, 1024, 0, 1, 1024), kernel="hist_global_kernel")
    check(sp, (0, 1, lds_cells), kmer=21, kernel="hist_lds_kernel")
    check(sp, (0, 1, lds_cells + 1), kmer=21, kernel="hist_global_kernel")
    check(sp, (0, 1, max_cells), kmer=21, kernel="hist_global_kernel")


# ---- 5. ends of the grid ----

def test_ends_of_the_grid(sp65):
    d = sp65.dense()
    stored = caps_of(sp65)[1]
    lowest = float(d[:, 0].min())
    assert lowest < stored and (d[:, 0] == np.float32(stored)).any()
    # [lowest stored value, a stored value]: both ends are counted, in the first and the last cell
    grid = (lowest, stored, 5, float(d[:, 1].min()), float(d[:, 1].max()), 3)
    want, out, _nan = check(sp65, grid)
    at_lo, at_hi = d[:, 0] == np.float32(lowest), d[:, 0] == np.float32(stored)
    assert int(want[0].sum()) >= int(at_lo.sum()) > 0 and int(want[-1].sum()) >= int(at_hi.sum()) > 0
    assert out == int((d[:, 0] > np.float32(stored)).sum()) > 0
    # one f32 step inside either end puts exactly those pairs outside
    inner = (float(np.nextafter(np.float32(lowest), np.float32(2))), float(np.nextafter(np.float32(stored), np.float32(-1)))) + grid[2:]
    _want, out_inner, _nan = check(sp65, inner)
    assert out_inner == out + int(at_lo.sum()) + int(at_hi.sum())
    # a grid strictly inside the data in both columns counts the rest in outside
    q = lambda x, s: float(np.quantile(d[:, x].astype(np.float64), s))      # noqa: E731
    inside = (q(0, 0.05), q(0, 0.2), 6, q(1, 0.05), q(1, 0.2), 7)      # (three quarters of the pairs are stored as (1, 1))
    assert d[:, 0].min() < inside[0] < inside[1] < d[:, 0].max() and d[:, 1].min() < inside[3] < inside[4] < d[:, 1].max()
    want, out, _nan = check(sp65, inside)
    assert out > 0 and want.sum() > 0


# ---- 6. one stored column ----

def test_single_k_and_ani(oracle, skl, gpu_ctx):
    sp = space(oracle, skl, gpu_ctx, "sp63", clustered(63, 4, seed=2))
    assert sp.i.size % 4 == 1                                     # the last 16-byte load holds one value
    for ani in (False, True):
        v = sp.dense(21, ani)[:, 0]
        for grid in ((0, 1, 8), (0, 1, 1), (float(v.min()), float(v.max()), 100), (0.2, 0.9, 7)):
            want, _out, _nan = check(sp, grid, kmer=21, ani=ani)
            assert want.ndim == 1
        for r0, r1 in ((0, 1), (5, 6), (60, 62)):                 # bands of 62, 57 and 3 values
            check(sp, (0, 1, 8), kmer=21, ani=ani, r0=r0, r1=r1)
    # the grid is on STORED values: unrelated pairs are stored as a distance of 1 and as an identity of 0
    d, a = sp.dense(21, False)[:, 0], sp.dense(21, True)[:, 0]
    hd, ha = np_hist(d[:, None], (0, 1, 8))[0], np_hist(a[:, None], (0, 1, 8))[0]
    assert hd[-1] > hd.sum() // 2 and hd[0] == 0 and ha[0] > ha.sum() // 2 and ha[-1] > 0
    # garbage in lo1 / hi1 / n1 is ignored with one column
    want, w_out, _nan = expected(sp, (0.2, 0.9, 7), kmer=21)
    with Slabs(sp, 21) as s:
        for garbage in ((float("nan"), float("-inf"), 0), (5.0, -5.0, 0xFFFFFFFF), (0.0, 0.0, 123456)):
            g = skl.HistGrid(0.2, 0.9, garbage[0], garbage[1], 7, garbage[2])
            counts = np.full(8, SENT, dtype=np.uint64)
            outside = np.full(2, SENT, dtype=np.uint64)
            assert raw(sp, s, g, counts, outside) == skl.OK
            assert np.array_equal(counts[:7], want) and counts[7] == SENT and outside.tolist() == [w_out, 0]


# ---- 7. cross ----

def test_cross(oracle, skl, gpu_ctx):
    nr, nq = 65, 7

    def make():
        ref = synth.set_r(nr, KMERS, SS64, n_clusters=4)
        qry = np.concatenate([ref[[7]], synth.set_r(nq - 1, KMERS, SS64, n_clusters=4, first_sample=1000)])
        return ref, nr, KMERS, SS64, None, (qry, nq, None)

    sp = space(oracle, skl, gpu_ctx, ("hist cross", nq), make)
    d = sp.dense()
    assert d.shape[0] == nr * nq and (d[7 * nq] == 0).all()       # (7, 0): a copy
    want, out, _nan = check(sp, G8)
    assert out == 0 and int(want.sum()) == nr * nq and int(want[0, 0]) >= 1
    check(sp, NARROW)
    check(sp, (0, 1, 128, 0, 1, 129))
    for r0, r1 in ((11, 29), (0, 1), (64, 65), (17, 17), (65, 65)):
        want, out, _nan = check(sp, G8, r0=r0, r1=r1)
        assert int(want.sum()) + out == (r1 - r0) * nq
    check(sp, (0, 1, 16), kmer=25, r0=3, r1=40)
    check(sp, (0.5, 1, 16), kmer=25, ani=True)
    with pytest.raises(skl.SklError) as e:
        run(sp, G8, r0=5, r1=nr + 1)
    assert e.value.code == skl.ERR_INVALID_ARG


# ---- 8. row ranges and ACCUMULATE ----

RANGES = ((0, 7), (7, 8), (8, 40), (40, 65))


@pytest.mark.parametrize("grid", [G8, (0, 1, 128, 0, 1, 129)])
def test_row_ranges_and_accumulate(sp65, grid):
    skl = sp65.skl
    whole, w_out, _nan = check(sp65, grid)
    cells = whole.size
    # fresh calls, summed in numpy
    parts = [check(sp65, grid, r0=r0, r1=r1) for r0, r1 in RANGES]
    assert np.array_equal(sum(p[0] for p in parts), whole) and sum(p[1] for p in parts) == w_out
    # chained with SKL_HIST_ACCUMULATE into a host array: the same object comes back; outside and nan are each call's own
    counts = np.zeros(whole.shape, dtype=np.uint64)
    outs = []
    for r0, r1 in RANGES:
        back, out, nan = run(sp65, grid, r0=r0, r1=r1, counts=counts)
        assert back is counts and nan == 0
        outs.append(out)
    assert np.array_equal(counts, whole) and outs == [p[1] for p in parts]
    # ... and into a device tensor, with a sentinel element behind the counts
    import torch

    t = torch.zeros(cells + 1, dtype=torch.int64, device="cuda:0")
    t[cells] = -7
    torch.cuda.synchronize()
    for r0, r1 in RANGES:
        back, out, nan = run(sp65, grid, r0=r0, r1=r1, counts=t)
        assert back is t
    got = t.cpu().numpy()
    assert np.array_equal(got[:cells].view(np.uint64).reshape(whole.shape), whole) and got[cells] == -7
    # the C call: outside is accumulated too under the flag; without it a pre-filled array (host or device) is overwritten
    with Slabs(sp65) as s:
        g = skl.HistGrid(grid[0], grid[1], grid[3], grid[4], grid[2], grid[5])
        counts = np.append(np.full(cells, 5, dtype=np.uint64), np.uint64(SENT))
        outside = np.array([1000, 2000], dtype=np.uint64)
        for r0, r1 in RANGES:
            assert raw(sp65, s, g, counts, outside, r0, r1, flags=skl.HIST_ACCUMULATE) == skl.OK
        assert np.array_equal(counts[:cells], whole.reshape(-1) + np.uint64(5)) and counts[cells] == SENT
        assert outside.tolist() == [1000 + w_out, 2000]
        assert raw(sp65, s, g, counts, outside, 8, 40) == skl.OK
        assert np.array_equal(counts[:cells], parts[2][0].reshape(-1)) and counts[cells] == SENT and outside.tolist() == [parts[2][1], 0]
        t.fill_(9)
        torch.cuda.synchronize()
        assert raw(sp65, s, g, t.data_ptr(), outside, 8, 40, on_device=1) == skl.OK
        got = t.cpu().numpy()
        assert np.array_equal(got[:cells].view(np.uint64), parts[2][0].reshape(-1)) and got[cells] == 9
        # an empty range: zeroed without the flag, kept with it
        assert raw(sp65, s, g, t.data_ptr(), outside, 20, 20, flags=skl.HIST_ACCUMULATE, on_device=1) == skl.OK
        assert np.array_equal(t.cpu().numpy(), got)
        assert raw(sp65, s, g, t.data_ptr(), outside, 20, 20, on_device=1) == skl.OK
        got = t.cpu().numpy()
        assert not got[:cells].any() and got[cells] == 9 and outside.tolist() == [0, 0]


# ---- 9. several bands ----

@pytest.mark.parametrize("band", [64, 1])
def test_bands(sp65, set_switch, band):
    one_band = {grid: check(sp65, grid) for grid in (G8, NARROW, (0, 1, 128, 0, 1, 129))}
    assert " bands)" not in sp65.ctx.last_kernel()
    set_switch("SKL_PAIRS_BAND", band)
    for grid, (whole, w_out, _nan) in one_band.items():
        want, out, _nan = check(sp65, grid)
        assert " bands)" in sp65.ctx.last_kernel()
        assert np.array_equal(want, whole) and out == w_out
    check(sp65, G8, r0=3, r1=50)
    check(sp65, (0, 1, 8), kmer=21)
    counts = np.zeros((8, 8), dtype=np.uint64)
    for r0, r1 in RANGES:
        run(sp65, G8, r0=r0, r1=r1, counts=counts)
    assert np.array_equal(counts, one_band[G8][0])
    set_switch("SKL_PAIRS_BAND", None)
    check(sp65, G8)
    assert " bands)" not in sp65.ctx.last_kernel()


# ---- 10. completeness vector ----

def steady(d, grid):
    """No value of d changes its cell, or whether it is on the grid, when moved by +-2e-6 in f32."""
    for x, (lo, hi, n) in enumerate(axes_of(grid, d.shape[1])):
        v = d[:, x]
        c, ok = axis_cells(v, lo, hi, n)
        for delta in (-2e-6, 2e-6):
            c2, ok2 = axis_cells((v.astype(np.float64) + delta).astype(np.float32), lo, hi, n)
            if not (np.array_equal(ok, ok2) and np.array_equal(c[ok], c2[ok])):
                return False
    return True


@pytest.mark.parametrize("mode", ["jaccard", "ani", "coreacc"])
def test_with_a_completeness_vector(oracle, skl, gpu_ctx, mode):
    def make():
        bins, n, kmers, ss64 = clustered(65, 4)()
        return bins, n, kmers, ss64, np.linspace(0.75, 1.0, n)

    sp = space(oracle, skl, gpu_ctx, "sp65comp", make)
    kmer, ani = (None, False) if mode == "coreacc" else (21, mode == "ani")
    d = sp.dense(kmer, ani)
    assert not np.array_equal(d, space(oracle, skl, gpu_ctx, "sp65", clustered(65, 4)).dense(kmer, ani))     # the vector changes the values
    grids = [(-0.05, 1.05, n0) + ((-0.05, 1.05, n0) if kmer is None else ()) for n0 in (7, 9, 13)]
    ok = [g for g in grids if steady(d, g)]
    assert ok, "no grid of 7, 9 or 13 cells is steady under +-2e-6"
    want, out, _nan = check(sp, ok[0], kmer=kmer, ani=ani)
    assert out == 0 and (want > 0).sum() > 1
    check(sp, ok[0], kmer=kmer, ani=ani, r0=11, r1=29)


# ---- 11. refused inputs ----

def test_refused_inputs(sp65):
    skl = sp65.skl
    nan, inf = float("nan"), float("inf")
    good = (0.0, 1.0, 0.0, 1.0, 8, 8)                             # (lo0, hi0, lo1, hi1, n0, n1): the struct's order
    bad_grids = [
        (0.0, 1.0, 0.0, 1.0, 0, 8), (0.0, 1.0, 0.0, 1.0, 8, 0),
        (nan, 1.0, 0.0, 1.0, 8, 8), (0.0, nan, 0.0, 1.0, 8, 8), (0.0, 1.0, nan, 1.0, 8, 8), (0.0, 1.0, 0.0, nan, 8, 8),
        (-inf, 1.0, 0.0, 1.0, 8, 8), (0.0, inf, 0.0, 1.0, 8, 8), (0.0, 1.0, -inf, 1.0, 8, 8), (0.0, 1.0, 0.0, inf, 8, 8),
        (0.0, 1e39, 0.0, 1.0, 8, 8),                              # infinite once rounded to float
        (1.0, 1.0, 0.0, 1.0, 8, 8), (1.0, 0.0, 0.0, 1.0, 8, 8), (0.0, 1.0, 0.5, 0.5, 8, 8), (0.0, 1.0, 0.5, 0.25, 8, 8),
        (1.0, 1.0 + 1e-12, 0.0, 1.0, 8, 8), (0.0, 1.0, 0.5, 0.5 + 1e-12, 8, 8),      # hi <= lo after rounding to float
        (0.0, 1.0, 0.0, 1.0, 1025, 1024), (0.0, 1.0, 0.0, 1.0, 1 << 20, 2), (0.0, 1.0, 0.0, 1.0, 0xFFFFFFFF, 0xFFFFFFFF),
    ]
    with Slabs(sp65) as s, Slabs(sp65, 21) as s1:
        def refused(slabs, grid, counts="own", outside="own", **kw):
            c = np.full(64 + 1, SENT, dtype=np.uint64)
            o = np.full(2, SENT, dtype=np.uint64)
            rc = raw(sp65, slabs, grid, c if isinstance(counts, str) else counts, o if isinstance(outside, str) else outside, **kw)
            assert rc == skl.ERR_INVALID_ARG, (rc, grid and [getattr(grid, f) for f, _t in grid._fields_], kw)
            assert (c == SENT).all() and (o == SENT).all()
            assert skl.load().skl_last_error()

        for fields in bad_grids:
            refused(s, skl.HistGrid(*fields))
        for fields in bad_grids[:1] + [f for f in bad_grids if f[0] != 0.0 or f[1] != 1.0] + [(0.0, 1.0, 0.0, 0.0, (1 << 20) + 1, 1)]:
            refused(s1, skl.HistGrid(*fields))                    # one column: the first column's refusals, and the cell limit
        ok = skl.HistGrid(*good)
        refused(s, None)
        refused(s, ok, counts=None)
        refused(s, ok, outside=None)
        for flags in (2, 3, 4, -1):
            refused(s, ok, flags=flags)
        refused(s, ok, r0=0, r1=sp65.n + 1)
        refused(s, ok, r0=66, r1=66)
        refused(s, ok, r0=9, r1=8)
        # and the same grid is served once nothing is wrong with the call
        c = np.full(65, SENT, dtype=np.uint64)
        o = np.full(2, SENT, dtype=np.uint64)
        assert raw(sp65, s, ok, c, o) == skl.OK
        want, w_out, _nan = expected(sp65, G8)
        assert np.array_equal(c[:64], want.reshape(-1)) and c[64] == SENT and o.tolist() == [w_out, 0]


# ---- 12. Python ----

def test_python_calls(sp65):
    skl, ctx = sp65.skl, sp65.ctx
    n = sp65.n
    with Slabs(sp65) as s:
        counts, outside, nan = skl.dists_hist(ctx, s.g, s.p, NARROW)
        assert isinstance(counts, np.ndarray) and counts.dtype == np.uint64 and counts.shape == (16, 4)
        assert type(outside) is int and type(nan) is int and nan == 0
        assert int(counts.sum()) + outside + nan == n * (n - 1) // 2
        counts, outside, nan = skl.dists_hist(ctx, s.g, s.p, NARROW, 5, 30)
        assert int(counts.sum()) + outside + nan == skl.self_pairs(n, 5, 30)
        with pytest.raises(ValueError):
            skl.dists_hist(ctx, s.g, s.p, (0, 1, 8))              # core/accessory wants both columns
        with pytest.raises(ValueError):
            skl.dists_hist(ctx, s.g, s.p, G8, counts=np.zeros(63, dtype=np.uint64))
        with pytest.raises(skl.SklError) as e:
            skl.dists_hist(ctx, s.g, s.p, (0, 1, 0, 0, 1, 8))
        assert e.value.code == skl.ERR_INVALID_ARG
        # cross: the slab against itself holds every pair twice and the diagonal (at 0, 0)
        both, out2, _nan = skl.dists_hist(ctx, s.g, s.p, G8, query=s.g)
        once, out1, _nan = skl.dists_hist(ctx, s.g, s.p, G8)
        diag = np.zeros((8, 8), dtype=np.uint64)
        diag[0, 0] = n
        assert np.array_equal(both, 2 * once + diag) and out2 == 2 * out1
        # consistency with count_within: a cap in an empty cell between occupied ones splits the first column's cells
        grid = (0, 1, 64, -1, 2, 1)
        want, w_out, _nan = expected(sp65, grid)
        first = want[:, 0]
        occupied = np.flatnonzero(first)
        assert w_out == 0 and occupied.size > 2
        gaps = [c for c in range(occupied[0] + 1, occupied[-1]) if first[c] == 0]
        assert gaps, "the oracle's first column occupies one run of cells"
        c = gaps[len(gaps) // 2]
        cap = (c + 0.5) / 64
        assert axis_cells(np.array([cap], dtype=np.float32), 0, 1, 64)[0][0] == c      # the cap lies in the empty cell: the rule is monotone
        counts, outside, _nan = skl.dists_hist(ctx, s.g, s.p, grid)
        below = int(counts[:c].sum())
        assert 0 < below < int(counts.sum()) and outside == 0
        assert skl.count_within(ctx, s.g, s.p, cap) == below
    with Slabs(sp65, 21) as s:
        counts, outside, nan = skl.dists_hist(ctx, s.g, s.p, (0, 0.5, 32))
        assert counts.shape == (32,) and int(counts.sum()) + outside + nan == n * (n - 1) // 2
        with pytest.raises(ValueError):
            skl.dists_hist(ctx, s.g, s.p, G8)
