"""skl_self_dists_pairs / skl_cross_dists_pairs (csrc/pair_list.hip): the distances of an explicit list of sample pairs.

Expected values are the oracle's dense results indexed at the listed pair (reversed entries at the same pair, `a == b`
entries from oracle.core_acc_pair / the diagonal of a cross call).  The bar is the project's own: without a
completeness correction bit-identical f32, with one |delta| <= 1e-6."""
import numpy as np
import pytest

from sketchlib.rust_amd import synth

pytestmark = pytest.mark.gpu

KERNEL = "pair_list_kernel"


def cond(i, j, n):
    """Condensed index of the pair {i, j}, i != j (distance_matrix.rs:11-14)."""
    i, j = np.minimum(i, j).astype(np.int64), np.maximum(i, j).astype(np.int64)
    return n * i - (i * (i + 1)) // 2 + j - 1 - i


class Db:
    """A synthetic database on both sides: oracle view and device slab, with or without completeness."""

    def __init__(self, oracle, skl, ctx, bins, n, kmers, ss64):
        self.oracle, self.skl, self.ctx = oracle, skl, ctx
        self.bins, self.n, self.kmers, self.ss64 = bins, n, list(kmers), ss64
        self.comp = np.linspace(0.75, 1.0, n)
        self._dense = {}

    def oview(self, comp):
        return self.oracle.Sketches(self.bins, self.n, self.kmers, self.ss64, self.comp if comp else None)

    def gview(self, comp):
        return self.ctx.sketches(self.bins, self.n, self.kmers, self.ss64, completeness=self.comp if comp else None)

    def dense(self, kmer, ani, comp):
        """oracle.self_dists_all for this mode, computed once."""
        key = (kmer, ani, comp)
        if key not in self._dense:
            o = self.oview(comp)
            if kmer is None:
                d = self.oracle.self_dists_all(o, threads=8)
            else:
                d = self.oracle.self_dists_all(o, self.oracle.JACCARD, self.kmers.index(kmer), ani, threads=8)
            d.setflags(write=False)
            self._dense[key] = d
        return self._dense[key]

    def diagonal(self, idx, kmer, ani, comp):
        """The oracle's value of (i, i) for the samples idx."""
        o = self.oview(comp)
        if kmer is None:
            return np.array([self.oracle.core_acc_pair(o, o, int(i), int(i)) for i in idx], dtype=np.float32)
        sub = self.oracle.Sketches(self.bins.reshape(self.n, -1)[idx], len(idx), self.kmers, self.ss64,
                                   self.comp[idx] if comp else None)
        d = self.oracle.cross_dists_all(sub, sub, self.oracle.JACCARD, self.kmers.index(kmer), ani)
        return d[np.arange(len(idx)), np.arange(len(idx))]

    def expected(self, a, b, kmer, ani, comp):
        a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
        d = self.dense(kmer, ani, comp)
        out = np.zeros((a.size, d.shape[1]), dtype=np.float32)
        off = a != b
        out[off] = d[cond(a[off], b[off], self.n)]
        if (~off).any():
            out[~off] = self.diagonal(a[~off], kmer, ani, comp)
        return out

    def run(self, a, b, kmer, ani, comp, out=None):
        g = self.gview(comp)
        try:
            return self.skl.self_dists_pairs(self.ctx, g, g.set_k(kmer, ani), a, b, out=out)
        finally:
            g.close()

    def check(self, a, b, kmer=None, ani=False, comp=False):
        got = self.run(a, b, kmer, ani, comp)
        assert KERNEL in self.ctx.last_kernel()
        exp = self.expected(a, b, kmer, ani, comp)
        assert got.shape == exp.shape and not np.isnan(got).any()
        if comp:
            err = float(np.max(np.abs(got.astype(np.float64) - exp)))
            print(f"n_pairs={len(a)} kmer={kmer} ani={ani} comp: max |delta| = {err:.3g}")
            assert err <= 1e-6
        else:
            bad = np.flatnonzero((got != exp).any(axis=1))
            print(f"n_pairs={len(a)} kmer={kmer} ani={ani}: {bad.size} entries differ")
            assert np.array_equal(got, exp), (bad[:5], got[bad[:5]], exp[bad[:5]])
        return got


def all_pairs(n):
    i, j = np.triu_indices(n, 1)
    return i.astype(np.uint32), j.astype(np.uint32)


_dbs = {}


def make_db(oracle, skl, ctx, n, kmers, ss64, n_clusters):
    key = (n, tuple(kmers), ss64, n_clusters)
    if key not in _dbs:
        _dbs[key] = Db(oracle, skl, ctx, synth.set_r(n, kmers, ss64, n_clusters=n_clusters), n, kmers, ss64)
    _dbs[key].ctx = ctx
    return _dbs[key]


@pytest.fixture()
def db300(oracle, skl, gpu_ctx):
    return make_db(oracle, skl, gpu_ctx, 300, [17, 21, 25, 29], 16, 7)


def case1_list(n):
    """All pairs shuffled, every pair reversed, 200 repeats and 20 entries with a == b, in one shuffled list."""
    rng = np.random.default_rng(5)
    i, j = all_pairs(n)
    rep = rng.integers(0, i.size, 200)
    same = rng.integers(0, n, 20).astype(np.uint32)
    a = np.concatenate([i, j, i[rep], same])
    b = np.concatenate([j, i, j[rep], same])
    order = rng.permutation(a.size)
    return a[order], b[order]


# ---- 1: every pair, every order ----

@pytest.mark.parametrize("kmer,ani,comp", [(None, False, False), (None, False, True), (21, False, False), (21, False, True),
                                           (21, True, False), (21, True, True)])
def test_every_pair_every_order(db300, kmer, ani, comp):
    a, b = case1_list(db300.n)
    got = db300.check(a, b, kmer, ani, comp)
    if kmer is None:
        plain = (got == 1.0).all(axis=1).mean()
        assert 0.5 < plain < 0.95, plain          # both arms of the fit: (1, 1) and fitted pairs
        if not comp:
            o = db300.oview(False)
            # reversed and a == b entries against the one-pair oracle
            for x in list(np.flatnonzero(a > b)[:100]) + list(np.flatnonzero(a == b)):
                assert tuple(got[x]) == db300.oracle.core_acc_pair(o, o, int(a[x]), int(b[x])), (x, a[x], b[x])
            assert (got[a == b] == 0.0).all()


# ---- 2: run shapes ----

def test_run_shapes(db300):
    n = db300.n
    rng = np.random.default_rng(6)
    a, b = [], []
    for row, length in enumerate([1, 2, 63, 64, 65, 129, 299]):
        r = 3 + 11 * row
        others = np.array([x for x in range(n) if x != r], dtype=np.uint32)
        a.append(np.full(length, r, dtype=np.uint32))
        b.append(others[:length] if length == 299 else rng.choice(others, length, replace=False))
    a, b = np.concatenate(a), np.concatenate(b)
    db300.check(a, b)
    db300.check(a, b, kmer=25)
    # one foreign pair in the middle of a long run
    cut = int(np.flatnonzero(a == 3 + 11 * 6)[0]) + 150
    a2 = np.concatenate([a[:cut], [7], a[cut:]]).astype(np.uint32)
    b2 = np.concatenate([b[:cut], [250], b[cut:]]).astype(np.uint32)
    got = db300.check(a2, b2)
    assert np.array_equal(np.delete(got, cut, axis=0), db300.run(a, b, None, False, False))
    # a single entry: one work item shorter than a wave, one workgroup with three idle waves
    db300.check(a[:1], b[:1])


# ---- 3: sketch sizes ----

@pytest.mark.parametrize("n,ss64,clusters", [(120, s, 6) for s in (1, 3, 16, 32, 33, 64, 96, 157, 170)] + [(40, 1100, 4)])
def test_sketch_sizes(oracle, skl, gpu_ctx, n, ss64, clusters):
    db = make_db(oracle, skl, gpu_ctx, n, [17, 21, 25], ss64, clusters)
    i, j = all_pairs(n)
    order = np.random.default_rng(ss64).permutation(i.size)
    for a, b in ((i, j), (i[order], j[order])):
        db.check(a, b)               # three lengths: one flat run, kept up to 3 trips (32 chunks), stepped beyond
        db.check(a, b, kmer=21)      # one length: kept up to 96 chunks, stepped beyond
    db.check(i, j, comp=True)
    _dbs.pop((n, (17, 21, 25), ss64, clusters))   # (the large ones are not needed again)


# ---- 4: many lengths, few lengths ----

def test_many_lengths(oracle, skl, gpu_ctx):
    db = make_db(oracle, skl, gpu_ctx, 150, list(range(13, 28, 2)), 8, 5)    # nk = 8 > MAX_FUSED_K: counts + fit kernel
    i, j = all_pairs(150)
    order = np.random.default_rng(8).permutation(i.size)
    db.check(i, j)
    assert "pair_list_fit_kernel" in gpu_ctx.last_kernel()
    db.check(i[order], j[order])
    db.check(i, j, comp=True)
    db.check(i[order], j[order], kmer=19, ani=True)


def test_two_lengths_is_the_degenerate_arm(oracle, skl, gpu_ctx):
    db = make_db(oracle, skl, gpu_ctx, 150, [17, 21], 8, 5)
    i, j = all_pairs(150)
    got = db.check(i, j)
    assert (got == 1.0).all()        # a fit needs three points (jaccard.rs:117)


@pytest.mark.parametrize("kmers,ss64", [([15, 19, 23, 27, 31], 16), ([17, 21], 64), ([15, 19, 23, 27, 31, 35], 40)])
def test_other_kept_and_reread_forms(oracle, skl, gpu_ctx, kmers, ss64):
    """More record shapes: 5 x 16 chunks (three flat trips kept), 2 x 64 and 6 x 40 chunks (stepped, the row re-read)."""
    db = make_db(oracle, skl, gpu_ctx, 90, kmers, ss64, 5)
    i, j = all_pairs(90)
    order = np.random.default_rng(9).permutation(i.size)
    db.check(i, j)
    db.check(i[order], j[order], comp=True)


def test_one_length_coreacc_is_the_existing_error(oracle, skl, gpu_ctx):
    bins = synth.set_r(10, [21], 4, n_clusters=2)
    g = gpu_ctx.sketches(bins, 10, [21], 4)
    with pytest.raises(skl.SklError) as e:
        skl.self_dists_pairs(gpu_ctx, g, g.set_k(), [0, 1], [1, 2])
    assert e.value.code == skl.ERR_KMER_COUNT and "at least two k-mer lengths" in e.value.message
    with pytest.raises(skl.SklError) as e2:
        skl.self_dists_all(gpu_ctx, g, g.set_k())
    assert e2.value.message == e.value.message
    g.close()


# ---- 5: cross ----

@pytest.mark.parametrize("ref_comp,query_comp", [(False, False), (True, True), (True, False), (False, True)])
def test_cross(oracle, skl, gpu_ctx, ref_comp, query_comp):
    kmers, ss64, nr, nq = [17, 21, 25, 29], 16, 150, 100
    ref = synth.set_r(nr, kmers, ss64, n_clusters=7)
    qry = np.concatenate([synth.set_r(90, kmers, ss64, n_clusters=7, seed=synth.SEED_R + 3), ref[[3, 10, 17, 24, 31, 38, 45, 52, 59, 149]]])
    rc = np.linspace(0.75, 1.0, nr) if ref_comp else None
    qc = np.linspace(1.0, 0.7, nq) if query_comp else None
    o_r, o_q = oracle.Sketches(ref, nr, kmers, ss64, rc), oracle.Sketches(qry, nq, kmers, ss64, qc)
    g_r, g_q = gpu_ctx.sketches(ref, nr, kmers, ss64, completeness=rc), gpu_ctx.sketches(qry, nq, kmers, ss64, completeness=qc)
    rng = np.random.default_rng(12)
    a, b = np.divmod(rng.permutation(nr * nq)[:9000], nq)                     # shuffled
    ga, gb = np.divmod(np.sort(rng.permutation(nr * nq)[:9000]), nq)          # grouped by reference
    both = ref_comp and query_comp                                            # the correction needs both vectors (jaccard.rs:36)
    for kmer, ani in ((None, False), (21, False), (21, True)):
        if kmer is None:
            exp = oracle.cross_dists_all(o_r, o_q, threads=8)
        else:
            exp = oracle.cross_dists_all(o_r, o_q, oracle.JACCARD, kmers.index(kmer), ani, threads=8)
        for x, y in ((a, b), (ga, gb)):
            got = skl.cross_dists_pairs(gpu_ctx, g_r, g_q, g_r.set_k(kmer, ani), x, y)
            assert KERNEL in gpu_ctx.last_kernel()
            if both:
                err = float(np.max(np.abs(got.astype(np.float64) - exp[x, y])))
                print(f"cross kmer={kmer} ani={ani} comp: max |delta| = {err:.3g}")
                assert err <= 1e-6
            else:
                assert np.array_equal(got, exp[x, y])
    if not both and (ref_comp or query_comp):   # one vector alone changes nothing
        plain_r, plain_q = gpu_ctx.sketches(ref, nr, kmers, ss64), gpu_ctx.sketches(qry, nq, kmers, ss64)
        assert np.array_equal(skl.cross_dists_pairs(gpu_ctx, g_r, g_q, g_r.set_k(), a, b),
                              skl.cross_dists_pairs(gpu_ctx, plain_r, plain_q, plain_r.set_k(), a, b))
        plain_r.close()
        plain_q.close()
    # copies of reference samples among the queries: distance zero
    got = skl.cross_dists_pairs(gpu_ctx, g_r, g_q, g_r.set_k(21), [3, 149], [90, 99])
    assert (got == 0.0).all()
    g_r.close()
    g_q.close()


# ---- 6: bands ----

@pytest.mark.parametrize("band", ["1000", "64"])
def test_bands(db300, set_switch, band):
    a, b = case1_list(db300.n)
    whole = {(k, c): db300.run(a, b, k, False, c) for k in (None, 21) for c in (False, True)}
    set_switch("SKL_PAIRS_BAND", band)
    for (k, c), exp in whole.items():
        assert np.array_equal(db300.run(a, b, k, False, c), exp), (k, c)
    # a grouped list: runs cut by band boundaries
    i, j = all_pairs(db300.n)
    set_switch("SKL_PAIRS_BAND", None)
    exp = db300.run(i[:20000], j[:20000], None, False, False)
    set_switch("SKL_PAIRS_BAND", band)
    assert np.array_equal(db300.run(i[:20000], j[:20000], None, False, False), exp)


# ---- 7: edges ----

def test_edges(db300, skl, gpu_ctx):
    import torch

    n = db300.n
    g = db300.gview(False)
    p = g.set_k()
    a, b = case1_list(n)
    a, b = a[:5000].copy(), b[:5000].copy()
    # an index equal to n: invalid argument naming the entry, nothing written
    for side in (0, 1):
        bad = [a.copy(), b.copy()]
        bad[side][4321] = n
        out = np.full((a.size, 2), -7.0, dtype=np.float32)
        with pytest.raises(skl.SklError) as e:
            skl.self_dists_pairs(gpu_ctx, g, p, bad[0], bad[1], out=out)
        assert e.value.code == skl.ERR_INVALID_ARG and "pair 4321" in e.value.message and str(n) in e.value.message
        assert (out == -7.0).all()
    # an empty list
    got = skl.self_dists_pairs(gpu_ctx, g, p, [], [])
    assert got.shape == (0, 2) and got.dtype == np.float32
    assert skl.self_dists_pairs(gpu_ctx, g, g.set_k(21), [], []).shape == (0, 1)
    # device output
    host = skl.self_dists_pairs(gpu_ctx, g, p, a, b)
    dev = torch.full((a.size, 2), -7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    skl.self_dists_pairs(gpu_ctx, g, p, a, b, out=dev)
    gpu_ctx.synchronize()
    assert np.array_equal(dev.cpu().numpy(), host)
    dev1 = torch.zeros((a.size, 1), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    skl.self_dists_pairs(gpu_ctx, g, g.set_k(25, True), a, b, out=dev1)
    gpu_ctx.synchronize()
    assert np.array_equal(dev1.cpu().numpy(), skl.self_dists_pairs(gpu_ctx, g, g.set_k(25, True), a, b))
    g.close()
