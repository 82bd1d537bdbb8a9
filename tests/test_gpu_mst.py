"""skl_self_mst / skl_clusters_from_edges (csrc/mst.hip, csrc/capi_mst.cpp): the minimum spanning forest of the distance graph by
Boruvka rounds over dense bands on the GPU, and the clusters a list of edges connects.

The expected trees never come from this library: they are Kruskal in numpy (kruskal()) over the ORACLE's dense array -- the
edges sorted by np.lexsort on (j, i, w), applied in blocks, pairs already in one component skipped -- which is the unique minimum
spanning forest under the header's edge order.  Without a completeness vector the stored values are the oracle's bit for bit,
so the bar is identical i, j and w arrays, identical labels and counts.  With one, stored values may differ in the last bit, so
the bar is structural: cuts at gap_cap midpoints (asserted on the CPU) give the oracle's components, and every weight is the
dense call's own value for its pair.  Every raw call writes into arrays with a sentinel behind the n - 1 records and the n
labels."""
import ctypes as C
import math

import numpy as np
import pytest

from sketchlib.rust_amd import synth
from test_gpu_clusters_within import assert_nontrivial, components
from test_gpu_clusters_within import expected as expected_clusters
from test_gpu_dists_within import INF, KMERS, SS64, caps_of, clustered, gap_cap, space

pytestmark = pytest.mark.gpu

SENT, SENT_W = 0xDEADBEEF, np.float32(-7.0)
BLOCK = 4096


def kruskal(n, i, j, w, cap=INF):
    """The minimum spanning forest of n samples under the edges (i, j, w) with w not NaN and <= (f32) cap, by the edge order
    (w, i, j) -> (i, j, w) in that order.  The sorted edges are taken block by block: those whose ends already carry one label
    are dropped at once, the others are applied one after the other, the higher label rewritten to the lower."""
    with np.errstate(invalid="ignore"):
        ok = w <= np.float32(cap)
    i, j, w = i[ok].astype(np.int64), j[ok].astype(np.int64), w[ok]
    order = np.lexsort((j, i, w))                                    # (-0.0 and +0.0 compare equal: the tie falls to i, j)
    i, j, w = i[order], j[order], w[order]
    lab = np.arange(n)
    taken = []
    for k in range(0, i.size, BLOCK):
        if len(taken) >= n - 1:
            break
        bi, bj = i[k:k + BLOCK], j[k:k + BLOCK]
        for e in np.flatnonzero(lab[bi] != lab[bj]):
            a, b = lab[bi[e]], lab[bj[e]]
            if a == b:
                continue
            lab[lab == max(a, b)] = min(a, b)
            taken.append(k + e)
    taken = np.asarray(taken, dtype=np.int64)
    return i[taken].astype(np.uint32), j[taken].astype(np.uint32), w[taken]


def raw(sp, column=0, cap=INF, kmer=None, ani=False, want_labels=True):
    """-> (rc, i, j, w, labels, n_edges, rounds): the outputs hold n records (n - 1 and a sentinel) and n + 1 labels."""
    skl, ctx, n = sp.skl, sp.ctx, sp.n
    g = ctx.sketches(sp.bins, n, sp.kmers, sp.ss64, completeness=sp.comp)
    try:
        p = g.set_k(kmer, ani, cutoff=sp.cutoff)
        oi, oj = np.full(n, SENT, dtype=np.uint32), np.full(n, SENT, dtype=np.uint32)
        ow = np.full(n, SENT_W, dtype=np.float32)
        lab = np.full(n + 1, SENT, dtype=np.uint32)
        found, rounds = C.c_uint64(77), C.c_uint32(77)
        rc = skl.load().skl_self_mst(ctx._h, g._h, C.byref(p), column, cap, oi.ctypes.data, oj.ctypes.data, ow.ctypes.data,
                                     lab.ctypes.data if want_labels else None, C.byref(found), C.byref(rounds))
        return rc, oi, oj, ow, lab, int(found.value), int(rounds.value)
    finally:
        g.close()


def check(sp, column=0, cap=INF, kmer=None):
    """The call gives Kruskal's forest over the oracle's values, bit for bit, with its labels; nothing beyond is touched."""
    n = sp.n
    d = sp.dense(kmer)[:, column] if n >= 2 else np.zeros(0, dtype=np.float32)
    ei, ej, ew = kruskal(n, sp.i, sp.j, d, cap)
    want_lab = components(n, ei, ej)
    rc, gi, gj, gw, lab, found, rounds = raw(sp, column, cap, kmer)
    assert rc == sp.skl.OK, sp.skl.load().skl_last_error()
    print(f"n={n} kmer={kmer} column={column} cap={cap}: {ei.size} edges expected, {found} found in {rounds} rounds")
    assert found == ei.size == n - int((want_lab == np.arange(n)).sum())
    assert np.array_equal(gi[:found], ei) and np.array_equal(gj[:found], ej)
    assert gw[:found].tobytes() == (ew + np.float32(0.0)).tobytes()           # (a stored -0.0f is reported as +0.0f)
    assert (gi[:found] < gj[:found]).all()
    assert (gi[found:] == SENT).all() and (gj[found:] == SENT).all() and (gw[found:] == SENT_W).all()
    assert np.array_equal(lab[:n], want_lab) and lab[n] == SENT
    assert rounds <= math.ceil(math.log2(n)) if n > 1 else rounds == 0
    assert (rounds == 0) == (found == 0)
    if n >= 2:
        name = sp.ctx.last_kernel()
        assert "mst_min_edge_kernel" in name and name.index("kernel") < name.index("mst_min_edge_kernel"), name   # the dense kernel is named first
        assert f"{rounds} rounds" in name
    return gi[:found], gj[:found], gw[:found], lab[:n], rounds


# ---- 1. small ----

@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_small(oracle, skl, gpu_ctx, n):
    """n = 65 is 2 080 pairs: one chunk and a little more, and every wave span crosses rows."""
    sp = space(oracle, skl, gpu_ctx, ("mst small", n), clustered(n, 4))
    for column, kmer in ((0, None), (1, None), (0, 21)):
        gi, _gj, _gw, lab, rounds = check(sp, column, INF, kmer)
        if n == 1:
            assert gi.size == 0 and lab.tolist() == [0] and rounds == 0
        else:
            assert gi.size == n - 1 and not lab.any()                # no cap, no NaN: one tree


# ---- 2. many chunks, several bands a round ----

@pytest.mark.parametrize("band", [1, 64])
def test_bands(oracle, skl, gpu_ctx, set_switch, band):
    sp = space(oracle, skl, gpu_ctx, ("mst", 300), clustered(300, 12))
    set_switch("SKL_PAIRS_BAND", band)
    for column, kmer in ((0, None), (1, None), (0, 25)):
        *_x, rounds = check(sp, column, INF, kmer)
        assert " bands a round" in sp.ctx.last_kernel() and " 1 bands" not in sp.ctx.last_kernel()
        assert 2 <= rounds <= math.ceil(math.log2(300))              # a within-cluster round and a between-cluster round at least
    set_switch("SKL_PAIRS_BAND", None)
    check(sp)
    assert " 1 bands a round" in sp.ctx.last_kernel()


def test_many_chunks(oracle, skl, gpu_ctx, set_switch):
    """2 100 samples: rows wider than a chunk, 2.2 M pairs, and with SKL_PAIRS_BAND = 64 a band per row."""
    sp = space(oracle, skl, gpu_ctx, ("mst", 2100), clustered(2100, 40))
    set_switch("SKL_PAIRS_BAND", 64)
    *_x, rounds = check(sp)
    assert 2 <= rounds <= math.ceil(math.log2(2100))
    set_switch("SKL_PAIRS_BAND", None)
    check(sp, 1)


# ---- 3. ties ----

def test_ties(oracle, skl, gpu_ctx):
    n = 70
    one = synth.set_r(1, KMERS, SS64, n_clusters=1)
    sp = space(oracle, skl, gpu_ctx, ("mst identical", n), lambda: (np.repeat(one, n, axis=0), n, KMERS, SS64))
    for column, kmer in ((0, None), (1, None), (0, 21)):
        assert not sp.dense(kmer)[:, column].any()                   # every pair at 0
        gi, gj, gw, lab, rounds = check(sp, column, INF, kmer)
        assert not gi.any() and np.array_equal(gj, np.arange(1, n)) and not gw.any() and rounds == 1      # the star at 0
        check(sp, column, 0.0, kmer)
    # unrelated samples -- sample s holds the value s + 1 in every bin, so no two share one: every single-k pair is stored as 1
    def unrelated():
        vals = np.broadcast_to(np.arange(1, n + 1, dtype=np.uint16)[:, None, None], (n, len(KMERS), SS64 * 64))
        return synth.bitslice(np.ascontiguousarray(vals)).reshape(n, -1), n, KMERS, SS64

    sp = space(oracle, skl, gpu_ctx, ("mst unrelated", n), unrelated)
    assert (sp.dense(29)[:, 0] == np.float32(1.0)).all()
    gi, gj, gw, lab, rounds = check(sp, 0, INF, 29)
    assert not gi.any() and np.array_equal(gj, np.arange(1, n)) and (gw == np.float32(1.0)).all() and rounds == 1
    below_one = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    gi, _gj, _gw, lab, rounds = check(sp, 0, below_one, 29)
    assert gi.size == 0 and np.array_equal(lab, np.arange(n)) and rounds == 0
    check(sp, 0, 1.0, 29)                                            # a cap equal to the stored value keeps it

    # duplicates at non-adjacent indices: weight-0 edges among the clusters' own
    def make():
        bins, m, kmers, ss64 = clustered(65, 4)()
        bins = bins.copy()
        bins[40] = bins[3]
        bins[57] = bins[3]
        bins[20] = bins[50]
        bins[64] = bins[0]
        return bins, m, kmers, ss64

    sp = space(oracle, skl, gpu_ctx, "mst duplicates", make)
    for column, kmer in ((0, None), (1, None), (0, 17)):
        d = sp.dense(kmer)[:, column]
        assert int((d == 0).sum()) >= 5
        gi, gj, gw, _lab, _rounds = check(sp, column, INF, kmer)
        zero = gw == 0                                               # the duplicates merge first: (40, 57) would close a cycle
        assert zero.sum() >= 4 and zero[:int(zero.sum())].all()
        assert {(3, 40), (3, 57), (20, 50), (0, 64)} <= set(zip(gi[zero].tolist(), gj[zero].tolist()))


# ---- 4. a forest under a cap ----

def test_forest_under_a_cap(oracle, skl, gpu_ctx):
    sp = space(oracle, skl, gpu_ctx, "sp65", clustered(65, 4))
    below, stored, above = caps_of(sp)
    d = sp.dense()
    quantile = float(np.quantile(d[:, 0].astype(np.float64), 0.1))
    for cap, nontrivial in ((below, False), (stored, True), (quantile, True), (0.5, True), (above, False)):
        want, n_want = expected_clusters(sp, cap)                    # the oracle's components, as the cluster tests build them
        if nontrivial:
            assert_nontrivial(want)
        gi, _gj, _gw, lab, _rounds = check(sp, 0, cap)
        assert np.array_equal(lab, want) and gi.size == sp.n - n_want
    # the accessory column under a cap of its own
    cap1 = float(np.quantile(d[:, 1].astype(np.float64), 0.1))
    gi, gj, _gw, lab, _rounds = check(sp, 1, cap1)
    with np.errstate(invalid="ignore"):
        k = d[:, 1] <= np.float32(cap1)
    want = components(sp.n, sp.i[k], sp.j[k])
    assert_nontrivial(want)
    assert np.array_equal(lab, want)


# ---- 5. cuts ----

def test_cuts(oracle, skl, gpu_ctx):
    sp = space(oracle, skl, gpu_ctx, "sp65", clustered(65, 4))
    gi, gj, gw, _lab, _rounds = check(sp)
    v = sp.dense()[:, 0]
    counts = []
    for share in (0.05, 0.3, 0.9):
        t = gap_cap(v, share)
        want, n_want = expected_clusters(sp, t)
        k = gw <= np.float32(t)
        assert np.array_equal(k, np.arange(gw.size) < int(k.sum()))  # a prefix
        lab, count = skl.clusters_from_edges(gpu_ctx, gi[k], gj[k], sp.n)
        assert lab.dtype == np.uint32 and np.array_equal(lab, want) and count == n_want
        assert "mst_edges_union_kernel" in gpu_ctx.last_kernel()
        counts.append(count)
    assert counts[0] > counts[2] > 0
    # no edge: the identity; every edge: the tree's one component; edges in any order and repeated
    lab, count = skl.clusters_from_edges(gpu_ctx, gi[:0], gj[:0], sp.n)
    assert np.array_equal(lab, np.arange(sp.n)) and count == sp.n
    perm = np.random.default_rng(1).permutation(np.concatenate([np.arange(gi.size), np.arange(gi.size)]))
    lab, count = skl.clusters_from_edges(gpu_ctx, gj[perm], gi[perm], sp.n)
    assert not lab.any() and count == 1
    lab, count = skl.clusters_from_edges(gpu_ctx, [], [], 0)
    assert lab.size == 0 and count == 0


# ---- 6. completeness vector ----

@pytest.mark.parametrize("kmer", [None, 21])
def test_with_a_completeness_vector(oracle, skl, gpu_ctx, kmer):
    def make():
        bins, n, kmers, ss64 = clustered(65, 4)()
        return bins, n, kmers, ss64, np.linspace(0.75, 1.0, n)

    sp = space(oracle, skl, gpu_ctx, "sp65comp", make)
    n = sp.n
    rc, gi, gj, gw, lab, found, rounds = raw(sp, 0, INF, kmer)
    assert rc == skl.OK and found == n - 1 and not lab[:n].any() and lab[n] == SENT and 1 <= rounds <= 7
    gi, gj, gw = gi[:found], gj[:found], gw[:found]
    assert (gi < gj).all() and (np.diff(gw) >= 0).all()
    v = sp.dense(kmer)[:, 0]
    counts = []
    for share in (0.05, 0.3, 0.9):
        t = gap_cap(v, share)                                        # (asserts the gap on the CPU)
        want, n_want = expected_clusters(sp, t, kmer=kmer)
        k = gw <= np.float32(t)
        got, count = skl.clusters_from_edges(gpu_ctx, gi[k], gj[k], n)
        assert np.array_equal(got, want) and count == n_want
        counts.append(count)
    assert counts[0] > counts[2]
    # every weight is the dense call's own value for its pair
    g = gpu_ctx.sketches(sp.bins, n, sp.kmers, sp.ss64, completeness=sp.comp)
    own = skl.self_dists_all(gpu_ctx, g, g.set_k(kmer, False, cutoff=sp.cutoff)).reshape(sp.i.size, -1)[:, 0]
    g.close()
    at = np.array([sp.start(int(a)) + int(b) - int(a) - 1 for a, b in zip(gi, gj)])
    assert gw.tobytes() == (own[at] + np.float32(0.0)).tobytes()
    assert float(np.max(np.abs(own.astype(np.float64) - v))) <= 1e-6


# ---- 7. NaN inputs ----

def test_nan_semantics_inputs(oracle, skl, gpu_ctx):
    """The inputs of tests/test_gpu_clusters_within.py::test_nan_semantics_inputs (a completeness of 0 under cutoff 0).  Whatever
    the dense call stores for the pairs of sample 3 decides: a pair that holds a NaN is never an edge, and the forest is Kruskal's
    with those pairs removed (kruskal() drops them with the same comparison).  A completeness vector is involved, so the weights
    are compared with the dense call's own."""
    def make():
        kmers, ss64, n = [17, 21, 25], 8, 12
        comp = np.ones(n)
        comp[3] = 0.0
        return synth.set_r(n, kmers, ss64, n_clusters=2), n, kmers, ss64, comp, None, 0.0

    sp = space(oracle, skl, gpu_ctx, "nan12", make)
    n = sp.n
    g = gpu_ctx.sketches(sp.bins, n, sp.kmers, sp.ss64, completeness=sp.comp)
    own = skl.self_dists_all(gpu_ctx, g, g.set_k(None, False, cutoff=sp.cutoff)).reshape(sp.i.size, -1)
    g.close()
    d = sp.dense()
    assert np.array_equal(np.isnan(own), np.isnan(d))
    for column in (0, 1):
        ei, ej, ew = kruskal(n, sp.i, sp.j, own[:, column])
        oi, oj, _ow = kruskal(n, sp.i, sp.j, d[:, column])
        rc, gi, gj, gw, lab, found, rounds = raw(sp, column)
        assert rc == skl.OK and found == ei.size
        nan = np.isnan(own[:, column])
        print(f"column {column}: {int(nan.sum())} NaN pairs, {found} edges, {rounds} rounds")
        assert np.array_equal(gi[:found], ei) and np.array_equal(gj[:found], ej) and gw[:found].tobytes() == (ew + np.float32(0.0)).tobytes()
        assert np.array_equal(lab[:n], components(n, oi, oj))        # the oracle's values connect the same samples
        nan_pairs = set(zip(sp.i[nan].tolist(), sp.j[nan].tolist()))
        assert not nan_pairs & set(zip(gi[:found].tolist(), gj[:found].tolist()))
        if nan[(sp.i == 3) | (sp.j == 3)].all():
            assert lab[3] == 3
        assert (gi[found:] == SENT).all() and lab[n] == SENT


# ---- 8. errors ----

def test_refused_inputs(oracle, skl, gpu_ctx):
    sp = space(oracle, skl, gpu_ctx, "sp65", clustered(65, 4))
    n = sp.n

    def untouched(res):
        rc, gi, gj, gw, lab, found, rounds = res
        assert rc == skl.ERR_INVALID_ARG, rc
        assert (gi == SENT).all() and (gj == SENT).all() and (gw == SENT_W).all() and (lab == SENT).all()
        assert found == 0 and rounds == 0

    untouched(raw(sp, 0, INF, 21, ani=True))                         # the tree is defined on distances
    untouched(raw(sp, 1, INF, 21))                                   # column 1 of one stored column
    for column in (2, -1):
        untouched(raw(sp, column))
    for cap in (float("nan"), -1e-9, -1.0):
        untouched(raw(sp, 0, cap))
    L = skl.load()
    g = gpu_ctx.sketches(sp.bins, n, sp.kmers, sp.ss64)
    p = g.set_k()
    oi, oj = np.full(n, SENT, dtype=np.uint32), np.full(n, SENT, dtype=np.uint32)
    ow = np.full(n, SENT_W, dtype=np.float32)
    found, rounds = C.c_uint64(77), C.c_uint32(77)
    full = [oi.ctypes.data, oj.ctypes.data, ow.ctypes.data, None, C.byref(found), C.byref(rounds)]
    for missing in (0, 1, 2, 4, 5):
        args = list(full)
        args[missing] = None
        assert L.skl_self_mst(gpu_ctx._h, g._h, C.byref(p), 0, INF, *args) == skl.ERR_INVALID_ARG
        assert (oi == SENT).all() and (oj == SENT).all() and (ow == SENT_W).all()
    assert L.skl_self_mst(gpu_ctx._h, g._h, C.byref(p), 0, INF, *full) == skl.OK and found.value == n - 1      # labels may be NULL
    g.close()
    # skl_clusters_from_edges: an index equal to n, on either side, is refused before anything follows it
    ei, ej = np.array([0, 5, 7], dtype=np.uint32), np.array([1, n, 2], dtype=np.uint32)
    lab = np.full(n + 1, SENT, dtype=np.uint32)
    count = C.c_uint64(77)
    for a, b in ((ei, ej), (ej, ei)):
        assert L.skl_clusters_from_edges(gpu_ctx._h, a.ctypes.data, b.ctypes.data, 3, n, lab.ctypes.data, C.byref(count)) == skl.ERR_INVALID_ARG
        assert (lab == SENT).all() and count.value == 0
    with pytest.raises(skl.SklError) as e:
        skl.clusters_from_edges(gpu_ctx, ei, ej, n)
    assert e.value.code == skl.ERR_INVALID_ARG
    assert L.skl_clusters_from_edges(gpu_ctx._h, ei.ctypes.data, ej.ctypes.data, 3, n, None, C.byref(count)) == skl.ERR_INVALID_ARG
    assert L.skl_clusters_from_edges(gpu_ctx._h, ei.ctypes.data, ej.ctypes.data, 3, n, lab.ctypes.data, None) == skl.ERR_INVALID_ARG
    assert L.skl_clusters_from_edges(gpu_ctx._h, None, ej.ctypes.data, 3, n, lab.ctypes.data, C.byref(count)) == skl.ERR_INVALID_ARG
    assert (lab == SENT).all()
    assert L.skl_clusters_from_edges(gpu_ctx._h, ei.ctypes.data, ej.ctypes.data, 3, n + 1, lab.ctypes.data, C.byref(count)) == skl.OK
    assert count.value == n + 1 - 3 and lab[1] == 0 and lab[n] == 5 and lab[7] == 2


# ---- 9. Python, and the launch names ----

def test_python_calls_and_launch_names(oracle, skl, gpu_ctx):
    sp = space(oracle, skl, gpu_ctx, "sp65", clustered(65, 4))
    n = sp.n
    ei, ej, ew = kruskal(n, sp.i, sp.j, sp.dense()[:, 0], 0.5)
    g = gpu_ctx.sketches(sp.bins, n, sp.kmers, sp.ss64)
    p = g.set_k()
    i, j, w, rounds = skl.mst(gpu_ctx, g, p, max_dist=0.5)
    assert i.dtype == np.uint32 and j.dtype == np.uint32 and w.dtype == np.float32 and isinstance(rounds, int)
    assert np.array_equal(i, ei) and np.array_equal(j, ej) and w.tobytes() == (ew + np.float32(0.0)).tobytes()
    name = gpu_ctx.last_kernel()
    assert name.index("kernel") < name.index("skl::mst_min_edge_kernel") < name.index("skl::mst_offer_min_kernel") < name.index("skl::mst_hook_kernel")
    assert f"{rounds} rounds" in name and "1 bands a round" in name
    i, j, w, rounds, lab = skl.mst(gpu_ctx, g, p, column=1, labels=True)
    e1 = kruskal(n, sp.i, sp.j, sp.dense()[:, 1])
    assert np.array_equal(i, e1[0]) and np.array_equal(j, e1[1]) and lab.dtype == np.uint32 and lab.shape == (n,) and not lab.any()
    # the slab is still usable, and the cluster call at the same cap agrees with the forest's labels
    *_x, lab = skl.mst(gpu_ctx, g, p, max_dist=0.5, labels=True)
    labels, count = skl.clusters_within(gpu_ctx, g, p, 0.5)
    assert np.array_equal(lab, labels) and count == n - ei.size
    g.close()
