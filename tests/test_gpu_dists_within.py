"""skl_self_dists_within / skl_cross_dists_within (csrc/within.hip, csrc/capi_within.cpp): all pairs of a dense call within a
distance cap, compacted on the GPU in the dense call's own order.

The expected result is the ORACLE's dense array filtered in numpy f32 with the predicate the header states -- never this
library's own dense output.  Without a completeness vector the bar is the project's: identical index lists and
bit-identical values.  With one, values may differ by <= 1e-6, so every cap is the midpoint of a gap of at least 4e-6 in the
oracle's sorted first-column values (asserted on the CPU before the GPU call): no pair can then legitimately flip, and the bar
is identical index lists with |delta| <= 1e-6 on the values.

Chunk size and scan width come from the native check of csrc/within_plan.hpp (tests/test_within_plan_cpu.py).  No whole self
call has exactly one chunk of pairs (2 048 is not a triangular number), so "exactly one chunk, and one more" are row 0 of
n = chunk + 1 and of n = chunk + 2 samples: the band the kernels see is what counts.

NaN: tests/test_gpu_edges.py takes the reference's NaN semantics from a completeness of 0 under cutoff 0; the same inputs are
rebuilt here.  The NaN of those inputs lives inside the fit and the stored values come out as plain numbers (the oracle's
array holds no NaN there), so the test shows that the filter sees what the dense call stores; that a NaN VALUE in either
column never passes is checked on arrays that hold one by the native check."""
import numpy as np
import pytest

from sketchlib.rust_amd import synth
from test_within_plan_cpu import consts as _plan_consts

pytestmark = pytest.mark.gpu


def consts():
    """csrc/within_plan.hpp's constants from a plain (unsanitized) build of tests/native/within_check.cpp."""
    return _plan_consts(sanitize=False)


KERNELS = ("within_count_kernel", "within_scan_kernel")
SENT_ID, SENT_D = 0xDEADBEEF, np.float32(-7.0)
INF = float("inf")


def keep_mask(d, cap, cap2=INF, ani=False):
    """The header's predicate on f32 values [positions, ncols]."""
    with np.errstate(invalid="ignore"):
        k = (d[:, 0] >= np.float32(1.0 - cap)) if ani else (d[:, 0] <= np.float32(cap))
        if d.shape[1] == 2 and not np.isinf(cap2):
            k = k & (d[:, 1] <= np.float32(cap2))
    return k


def gap_cap(values, share):
    """A cap no value lies within 2e-6 of: the midpoint of the gap of >= 4e-6 in the sorted values nearest to quantile `share`."""
    v = np.unique(values[np.isfinite(values)].astype(np.float64))
    gaps = np.flatnonzero(np.diff(v) >= 4e-6)
    assert gaps.size, "no gap of 4e-6 between the oracle's values"
    g = gaps[np.argmin(np.abs(gaps - share * (v.size - 1)))]
    cap = 0.5 * (v[g] + v[g + 1])
    assert v[g] + 1.9e-6 <= float(np.float32(cap)) <= v[g + 1] - 1.9e-6
    return cap


class Space:
    """A pair space on both sides: the oracle's dense values with their (i, j), and the device slabs."""

    def __init__(self, oracle, skl, ctx, bins, n, kmers, ss64, comp=None, query=None, cutoff=0.64):
        self.oracle, self.skl, self.ctx = oracle, skl, ctx
        self.bins, self.n, self.kmers, self.ss64, self.comp, self.cutoff = bins, n, list(kmers), ss64, comp, cutoff
        self.query = query                      # (bins, n, comp) of the query side, or None: self mode
        self.n_cols = query[1] if query else n
        if query:
            self.i, self.j = [x.astype(np.uint32) for x in np.divmod(np.arange(n * query[1]), query[1])]
        else:
            self.i, self.j = [x.astype(np.uint32) for x in np.triu_indices(n, 1)]
        self._dense = {}

    def start(self, r):
        """Position of the first pair of row r."""
        if self.query:
            return r * self.n_cols
        r = min(r, max(self.n - 1, 0))
        return r * self.n - r * (r + 1) // 2

    def dense(self, kmer=None, ani=False):
        key = (kmer, ani)
        if key not in self._dense:
            O = self.oracle
            o = O.Sketches(self.bins, self.n, self.kmers, self.ss64, self.comp)
            mode = (O.COREACC, 0, False) if kmer is None else (O.JACCARD, self.kmers.index(kmer), ani)
            if self.query:
                q = O.Sketches(self.query[0], self.query[1], self.kmers, self.ss64, self.query[2])
                d = O.cross_dists_all(o, q, *mode, cutoff=self.cutoff, threads=8)
            else:
                d = O.self_dists_all(o, *mode, cutoff=self.cutoff, threads=8)
            d = np.ascontiguousarray(d, dtype=np.float32).reshape(self.i.size, -1)
            d.setflags(write=False)
            self._dense[key] = d
        return self._dense[key]

    def expected(self, cap, cap2=INF, kmer=None, ani=False, r0=0, r1=None):
        a, b = self.start(r0), self.start(self.n if r1 is None else r1)
        d = self.dense(kmer, ani)[a:b]
        k = keep_mask(d, cap, cap2, ani)
        return self.i[a:b][k], self.j[a:b][k], d[k]

    def run(self, cap, cap2=INF, kmer=None, ani=False, r0=0, r1=None, capacity=0, device=False):
        """-> (n_found, i, j, d): the outputs hold capacity + 1 records, sentinel-filled before the call."""
        skl, ctx = self.skl, self.ctx
        g = ctx.sketches(self.bins, self.n, self.kmers, self.ss64, completeness=self.comp)
        q = ctx.sketches(self.query[0], self.query[1], self.kmers, self.ss64, completeness=self.query[2]) if self.query else None
        try:
            p = g.set_k(kmer, ani, cutoff=self.cutoff)
            nc = skl.ncols(p)
            if capacity == 0:
                return skl.dists_within_into(ctx, g, p, cap, cap2, r0, r1, None, 0, q), None, None, None
            if device:
                import torch

                oi = torch.full((capacity + 1,), SENT_ID - (1 << 32), dtype=torch.int32, device="cuda:0")
                oj = oi.clone()
                od = torch.full((capacity + 1, nc), float(SENT_D), dtype=torch.float32, device="cuda:0")
                torch.cuda.synchronize()
                found = skl.dists_within_into(ctx, g, p, cap, cap2, r0, r1, (oi, oj, od), capacity, q)
                return found, oi.cpu().numpy().view(np.uint32), oj.cpu().numpy().view(np.uint32), od.cpu().numpy()
            oi = np.full(capacity + 1, SENT_ID, dtype=np.uint32)
            oj = oi.copy()
            od = np.full((capacity + 1, nc), SENT_D, dtype=np.float32)
            return skl.dists_within_into(ctx, g, p, cap, cap2, r0, r1, (oi, oj, od), capacity, q), oi, oj, od
        finally:
            g.close()
            if q is not None:
                q.close()

    def check(self, cap, cap2=INF, kmer=None, ani=False, r0=0, r1=None, capacity=None, device=False):
        """Count-only agrees with the oracle's count; the sized call gives the oracle's list; nothing beyond it is touched."""
        ei, ej, ed = self.expected(cap, cap2, kmer, ani, r0, r1)
        n_exp = ei.size
        assert self.run(cap, cap2, kmer, ani, r0, r1)[0] == n_exp
        launched = self.start(self.n if r1 is None else r1) > self.start(r0)      # (an empty pair space launches nothing and names nothing)
        name = self.ctx.last_kernel()
        assert not launched or (all(k in name for k in KERNELS) and "within_scatter_kernel" not in name and "count only" in name), name
        capacity = n_exp if capacity is None else capacity
        if capacity == 0:
            return n_exp
        found, gi, gj, gd = self.run(cap, cap2, kmer, ani, r0, r1, capacity, device)
        name = self.ctx.last_kernel()
        assert not launched or (all(k in name for k in KERNELS + ("within_scatter_kernel",)) and name.index("kernel") < name.index("within_count")), name
        assert found == n_exp, (found, n_exp)
        w = min(capacity, n_exp)
        print(f"n={self.n} cols={self.n_cols} kmer={kmer} ani={ani} cap=({cap}, {cap2}) rows=({r0}, {r1}): {n_exp} pairs, {w} written")
        assert np.array_equal(gi[:w], ei[:w]) and np.array_equal(gj[:w], ej[:w])
        if self.comp is not None or (self.query and self.query[2] is not None):
            assert w == 0 or float(np.max(np.abs(gd[:w].astype(np.float64) - ed[:w]))) <= 1e-6
        else:
            assert gd[:w].tobytes() == ed[:w].tobytes()
        assert (gi[w:] == SENT_ID).all() and (gj[w:] == SENT_ID).all() and (gd[w:] == SENT_D).all()     # the element after the prefix is untouched
        return n_exp


KMERS, SS64 = [17, 21, 25, 29], 8
_spaces = {}


def space(oracle, skl, ctx, key, make):
    if key not in _spaces:
        _spaces[key] = Space(oracle, skl, ctx, *make())
    _spaces[key].ctx = ctx
    return _spaces[key]


def clustered(n, n_clusters, seed=0):
    return lambda: (synth.set_r(n, KMERS, SS64, n_clusters=n_clusters, seed=synth.SEED_R + seed), n, KMERS, SS64)


def caps_of(sp, kmer=None, ani=False):
    """(below every value, a stored value, above every value) of the first column, as distances."""
    v = sp.dense(kmer, ani)[:, 0].astype(np.float64)
    v = 1.0 - v if ani else v
    inner = np.sort(v[(v > v.min()) & (v < v.max())])
    stored = float(inner[inner.size // 3]) if inner.size else float(v.min())
    below = float(v.min()) / 2 if v.min() > 0 else None      # (identical samples: no cap lies below a distance of 0)
    return below, stored, 2.0


@pytest.fixture()
def sp65(oracle, skl, gpu_ctx):
    return space(oracle, skl, gpu_ctx, "sp65", clustered(65, 4))


# ---- self, core/accessory: sizes ----

@pytest.mark.parametrize("n", [2, 3, 65])
def test_self_coreacc_small(oracle, skl, gpu_ctx, n):
    sp = space(oracle, skl, gpu_ctx, ("small", n), clustered(n, 1 if n < 4 else 4))
    below, stored, above = caps_of(sp)
    assert below is not None and sp.check(below) == 0 # nothing found: nothing written
    assert sp.check(above) == n * (n - 1) // 2        # the dense listing itself
    got = sp.check(stored)                            # a cap equal to a stored value keeps it
    assert 0 < got <= n * (n - 1) // 2
    assert (sp.dense()[:, 0] == np.float32(stored)).any()


@pytest.mark.parametrize("extra", [1, 2])
def test_one_chunk_and_one_more(oracle, skl, gpu_ctx, extra):
    chunk = consts()[0]
    n = chunk + extra                                 # row 0 holds chunk (+ 1) pairs
    sp = space(oracle, skl, gpu_ctx, ("chunk", n), clustered(n, 40))
    assert sp.start(1) - sp.start(0) == chunk + extra - 1
    _below, stored, above = caps_of(sp)
    assert sp.check(above, r0=0, r1=1) == chunk + extra - 1
    assert 0 < sp.check(stored, r0=0, r1=1) < chunk
    last = sp.check(above, r0=n - 3, r1=n - 1)        # the triangle's last two rows: 2 + 1 pairs
    assert last == 3


def test_more_chunks_than_one_scan_step_mostly_empty(oracle, skl, gpu_ctx):
    """2 100 unrelated samples, then 100 copies of one sample: the last 4 950 positions (the copies' own rows) are at distance 0
    and all pass a cap of 0 -- full chunks -- and nearly every chunk before them counts 0; 1 182 chunks against a scan step
    of 1 024."""
    chunk, _span, step = consts()[:3]

    def make():
        a = synth.set_r(2100, KMERS, SS64, n_clusters=2100)
        b = np.repeat(synth.set_r(1, KMERS, SS64, n_clusters=1, seed=synth.SEED_R + 5), 100, axis=0)
        return np.concatenate([a, b]), 2200, KMERS, SS64

    sp = space(oracle, skl, gpu_ctx, "clustered2200", make)
    pairs = sp.i.size
    assert -(-pairs // chunk) > step
    d = sp.dense()
    k = keep_mask(d, 0.0)
    per_chunk = np.add.reduceat(k.astype(np.int64), np.arange(0, pairs, chunk))
    assert (per_chunk == 0).mean() > 0.9 and (per_chunk == chunk).sum() >= 2 and k[-4950:].all()
    assert sp.check(0.0) == int(k.sum())
    sp.check(0.0, device=True)
    assert sp.check(0.5, cap2=0.5) >= 4950            # both columns tested
    sp.check(2.0, capacity=5000)                      # every chunk full, the first 5 000 records written


# ---- row ranges ----

def test_row_ranges(sp65):
    n = sp65.n
    _below, stored, above = caps_of(sp65)
    for cap in (stored, above):
        for r0, r1 in ((0, 1), (n - 2, n - 1), (n - 2, n), (13, 37), (20, 20), (n, n), (0, 0)):
            sp65.check(cap, r0=r0, r1=r1)
        # consecutive ranges, concatenated, are the whole call
        whole = sp65.expected(cap)
        parts = []
        for r0, r1 in ((0, 7), (7, 8), (8, 40), (40, n)):
            m = sp65.check(cap, r0=r0, r1=r1)
            parts.append(sp65.run(cap, r0=r0, r1=r1, capacity=max(m, 1))[1:])
            parts[-1] = [x[:m] for x in parts[-1]]
        for x in range(3):
            assert np.array_equal(np.concatenate([p[x] for p in parts]), whole[x])
    with pytest.raises(sp65.skl.SklError) as e:
        sp65.run(stored, r0=5, r1=n + 1)
    assert e.value.code == sp65.skl.ERR_INVALID_ARG


# ---- several bands ----

@pytest.mark.parametrize("band", [100, 64, 1])
def test_bands(sp65, set_switch, band):
    """SKL_PAIRS_BAND cuts the call into bands of whole rows of at most that many pairs (1: a row a band).  With the cap above
    every value each band edge has a survivor on either side."""
    _below, stored, above = caps_of(sp65)
    set_switch("SKL_PAIRS_BAND", band)
    for cap in (above, stored):
        for device in (False, True):
            sp65.check(cap, device=device)
            assert " bands)" in sp65.ctx.last_kernel()
        m = sp65.check(cap, capacity=0)
        sp65.check(cap, capacity=m - 1)               # the cut falls inside a band
        sp65.check(cap, capacity=m // 2, device=True)
        sp65.check(cap, r0=3, r1=50)
    sp65.check(stored, kmer=21)
    set_switch("SKL_PAIRS_BAND", None)
    sp65.check(above)
    assert " bands)" not in sp65.ctx.last_kernel()


# ---- caps ----

def test_caps(sp65):
    skl = sp65.skl
    below, stored, above = caps_of(sp65)
    d = sp65.dense()
    assert below is not None and sp65.check(below, capacity=10) == 0        # 0 found: the sentinel-filled outputs stay as they are
    assert sp65.check(above) == d.shape[0]
    assert sp65.check(0.0) == int((d[:, 0] == 0).sum())
    acc = float(np.median(d[keep_mask(d, stored), 1]))
    both = sp65.check(stored, cap2=acc)
    assert 0 < both < sp65.check(stored)              # the second cap cuts a subset
    assert sp65.check(stored, cap2=-1.0) == 0         # a cap nothing meets is a cap, not an error
    for bad in ((float("nan"), INF), (0.1, float("nan")), (-1e-9, INF), (-1.0, 0.5)):
        for capacity in (0, 4):
            with pytest.raises(skl.SklError) as e:
                sp65.run(*bad, capacity=capacity)
            assert e.value.code == skl.ERR_INVALID_ARG
    # outputs missing although records are asked for
    g = sp65.ctx.sketches(sp65.bins, sp65.n, sp65.kmers, sp65.ss64)
    with pytest.raises(skl.SklError) as e:
        skl.dists_within_into(sp65.ctx, g, g.set_k(), stored, out=None, capacity=4)
    assert e.value.code == skl.ERR_INVALID_ARG
    g.close()


# ---- capacity ----

@pytest.mark.parametrize("device", [False, True])
def test_capacity(sp65, device):
    _below, stored, _above = caps_of(sp65)
    m = sp65.check(stored, capacity=0)
    assert m > 3
    sp65.check(stored, capacity=m, device=device)
    sp65.check(stored, capacity=m - 1, device=device)     # the prefix, and the element after it untouched
    sp65.check(stored, capacity=1, device=device)
    sp65.check(stored, capacity=100 * m, device=device)


# ---- modes ----

def test_single_k_odd_pair_count(oracle, skl, gpu_ctx):
    """One column: four values per 16-byte load; 63 samples give 1 953 pairs, so the last load holds one."""
    sp = space(oracle, skl, gpu_ctx, "sp63", clustered(63, 4, seed=2))
    assert sp.i.size % 4 == 1
    below, stored, above = caps_of(sp, kmer=21)
    assert below is not None and sp.check(below, kmer=21) == 0
    assert sp.check(above, kmer=21) == sp.i.size
    assert 0 < sp.check(stored, kmer=21, device=True) < sp.i.size
    sp.check(stored, cap2=0.0, kmer=21)               # the second cap is ignored with one column
    for r0, r1 in ((0, 1), (5, 6), (60, 62)):         # bands of 62, 57 and 3 values
        sp.check(above, kmer=21, r0=r0, r1=r1)


def test_ani_turns_the_test_round(oracle, skl, gpu_ctx):
    sp = space(oracle, skl, gpu_ctx, "sp63", clustered(63, 4, seed=2))
    below, stored, above = caps_of(sp, kmer=21, ani=True)
    d = sp.dense(21, True)[:, 0]
    # the bound is 1 - cap, formed in double and rounded once: the stored identity itself is kept
    assert (d == np.float32(1.0 - stored)).any()
    m = sp.check(stored, kmer=21, ani=True)
    assert m == int((d >= np.float32(1.0 - stored)).sum()) and 0 < m < d.size
    assert sp.check(above, kmer=21, ani=True) == d.size
    assert below is not None and sp.check(below, kmer=21, ani=True) == 0
    # close pairs have a HIGH identity: the distance-mode list of the same cap is another one
    assert sp.check(0.02, kmer=21, ani=True, device=True) == int((d >= np.float32(0.98)).sum())


@pytest.mark.parametrize("kmer", [None, 21])
def test_with_a_completeness_vector(oracle, skl, gpu_ctx, kmer):
    def make():
        bins, n, kmers, ss64 = clustered(65, 4)()
        return bins, n, kmers, ss64, np.linspace(0.75, 1.0, n)

    sp = space(oracle, skl, gpu_ctx, "sp65comp", make)
    v = sp.dense(kmer)[:, 0]
    for share in (0.05, 0.3, 0.9):
        cap = gap_cap(v, share)
        m = sp.check(cap, kmer=kmer, device=share == 0.3)
        assert 0 < m < v.size
    sp.check(gap_cap(v, 0.3), kmer=kmer, r0=11, r1=29, capacity=17)


def test_nan_semantics_inputs(oracle, skl, gpu_ctx):
    """The inputs tests/test_gpu_edges.py takes the reference's NaN semantics from: a completeness of 0 under cutoff 0."""
    def make():
        kmers, ss64, n = [17, 21, 25], 8, 12
        comp = np.ones(n)
        comp[3] = 0.0
        return synth.set_r(n, kmers, ss64, n_clusters=2), n, kmers, ss64, comp, None, 0.0

    sp = space(oracle, skl, gpu_ctx, "nan12", make)
    d = sp.dense()
    row3 = (sp.i == 3) | (sp.j == 3)
    nan = np.isnan(d).any(axis=1)
    print(f"{int(nan.sum())} of {d.shape[0]} oracle pairs hold a NaN; pairs of sample 3: {np.unique(d[row3], axis=0)}")
    for share in (0.2, 0.6):
        cap = gap_cap(d[:, 0], share)
        sp.check(cap)
        gi, gj = sp.run(cap, capacity=d.shape[0])[1:3]
        listed = set(zip(gi.tolist(), gj.tolist()))
        assert not any((int(a), int(b)) in listed for a, b in zip(sp.i[nan], sp.j[nan]))      # a NaN never passes
    assert sp.check(2.0) == int((~np.isnan(d[:, 0])).sum())


# ---- cross ----

@pytest.mark.parametrize("nq", [1, 63, 64, 65])
def test_cross(oracle, skl, gpu_ctx, nq):
    nr = 40

    def make():
        ref = synth.set_r(nr, KMERS, SS64, n_clusters=5)
        qry = np.concatenate([ref[[7]], synth.set_r(nq - 1, KMERS, SS64, n_clusters=5, first_sample=1000)]) if nq > 1 else ref[[7]]
        return ref, nr, KMERS, SS64, None, (qry, nq, None)

    sp = space(oracle, skl, gpu_ctx, ("cross", nq), make)
    d = sp.dense()
    assert d.shape[0] == nr * nq and (d[7 * nq] == 0).all()        # (7, 0): a copy
    inner = np.sort(d[(d[:, 0] > 0) & (d[:, 0] < 1), 0])
    stored = float(inner[inner.size // 2])
    assert sp.check(2.0) == nr * nq
    assert sp.check(0.0) >= 1
    m = sp.check(stored, device=True)
    assert 0 < m < nr * nq
    acc = float(np.median(d[keep_mask(d, stored), 1]))
    assert 0 < sp.check(stored, cap2=acc) < m                      # a cap on both columns
    sp.check(stored, r0=11, r1=29)                                 # a reference range in the middle
    sp.check(2.0, r0=11, r1=29, capacity=100)
    sp.check(stored, r0=17, r1=17)
    sp.check(stored, kmer=25, r0=3, r1=40)
    sp.check(0.3, kmer=25, ani=True)


def test_cross_bands(oracle, skl, gpu_ctx, set_switch):
    nr, nq = 40, 65

    def make():
        ref = synth.set_r(nr, KMERS, SS64, n_clusters=5)
        qry = np.concatenate([ref[[7]], synth.set_r(nq - 1, KMERS, SS64, n_clusters=5, first_sample=1000)])
        return ref, nr, KMERS, SS64, None, (qry, nq, None)

    sp = space(oracle, skl, gpu_ctx, ("cross", nq), make)
    set_switch("SKL_PAIRS_BAND", 3 * nq + 1)          # three reference rows a band
    sp.check(2.0)
    assert "14 bands" in sp.ctx.last_kernel()
    d = sp.dense()
    sp.check(float(np.median(d[d[:, 0] < 1, 0])), device=True)


# ---- Python ----

def test_python_calls(sp65):
    skl, ctx = sp65.skl, sp65.ctx
    _below, stored, above = caps_of(sp65)
    g = ctx.sketches(sp65.bins, sp65.n, sp65.kmers, sp65.ss64)
    p = g.set_k()
    ei, ej, ed = sp65.expected(stored)
    assert skl.count_within(ctx, g, p, stored) == ei.size
    for capacity in (None, ei.size, 3, 10 * ei.size):          # 3: the arrays overflow and the call repeats with the exact size
        i, j, d = skl.self_dists_within(ctx, g, p, stored, capacity=capacity)
        assert i.dtype == np.uint32 and j.dtype == np.uint32 and d.dtype == np.float32 and d.shape == (ei.size, 2)
        assert np.array_equal(i, ei) and np.array_equal(j, ej) and d.tobytes() == ed.tobytes()
    ei, ej, ed = sp65.expected(stored, 0.2, r0=5, r1=30)
    i, j, d = skl.self_dists_within(ctx, g, p, stored, 0.2, 5, 30)
    assert np.array_equal(i, ei) and np.array_equal(j, ej) and d.tobytes() == ed.tobytes()
    assert skl.count_within(ctx, g, p, stored, 0.2, 5, 30) == ei.size
    i, j, d = skl.self_dists_within(ctx, g, g.set_k(21), 1e-9)
    assert i.size == 0 and j.size == 0 and d.shape == (0, 1)
    # cross: the slab against itself lists every pair twice and the diagonal
    i, j, d = skl.cross_dists_within(ctx, g, g, p, stored)
    assert i.size == 2 * sp65.expected(stored)[0].size + sp65.n and skl.count_within(ctx, g, p, stored, query=g) == i.size
    up = i < j
    assert np.array_equal(i[up], sp65.expected(stored)[0]) and np.array_equal(j[up], sp65.expected(stored)[1])
    g.close()
