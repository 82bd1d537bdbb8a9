"""skl_self_clusters_within / skl_clusters_merge (csrc/cluster.hip, csrc/capi_clusters.cpp): single-linkage clusters under a
distance cap, one label per sample, by a lock-free union-find on the GPU behind each dense band.

The expected labels never come from this library: they are the connected components of the graph whose edges are the ORACLE's
dense array filtered in numpy f32 with the header's predicate (tests/test_gpu_dists_within.py: Space, keep_mask), found by a
small union-find in array form here (components()), label = lowest index.  The bar is identical label arrays and an identical
cluster count: without a completeness vector the stored values are the oracle's bit for bit; with one, every cap is a
gap_cap midpoint (asserted on the CPU before the GPU call), so no pair can legitimately flip.  Where a case says so, the test
asserts before the GPU call that the expected structure is not trivial: more than one cluster, fewer than n, one of three or
more samples."""
import ctypes as C

import numpy as np
import pytest

from sketchlib.rust_amd import synth
from test_gpu_dists_within import INF, KMERS, SS64, caps_of, clustered, consts, gap_cap, space

pytestmark = pytest.mark.gpu

SENT = 0xDEADBEEF


def components(n, i, j):
    """Connected components of n samples under edges (i[k], j[k]), label = lowest index: a union-find in array form.  Every
    round hooks each edge's two current labels (and its two samples) under the lower of the two, then follows the labels to
    their ends; at the fixed point both ends of every edge carry one label, a label is a member of its component no higher
    than the sample, and so it is the component's lowest index."""
    lab = np.arange(n, dtype=np.int64)
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    while i.size:
        li, lj = lab[i], lab[j]
        live = li != lj                                              # (of ALL edges, every round: labels that agree now may part again)
        if not live.any():
            break
        li, lj = li[live], lj[live]
        lo = np.minimum(li, lj)
        for at in (li, lj, i[live], j[live]):
            np.minimum.at(lab, at, lo)
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    return lab.astype(np.uint32)


def sizes_of(lab):
    return np.sort(np.bincount(lab)[np.unique(lab)])[::-1]


def assert_nontrivial(lab):
    s = sizes_of(lab)
    assert 1 < s.size < lab.size and s[0] >= 3, s


def expected(sp, cap, cap2=INF, kmer=None, ani=False, r0=0, r1=None, start=None):
    """-> (labels, n_clusters) from the oracle; start: a partition the call continues from (its links are edges too)."""
    if sp.n < 2:
        ei = ej = np.zeros(0, dtype=np.int64)
    else:
        ei, ej, _d = sp.expected(cap, cap2, kmer, ani, r0, r1)
    if start is not None:
        ei, ej = np.concatenate([ei, np.arange(sp.n)]), np.concatenate([ej, np.asarray(start[:sp.n], dtype=np.int64)])
    lab = components(sp.n, ei, ej)
    return lab, int((lab == np.arange(sp.n)).sum())


def run(sp, cap, cap2=INF, kmer=None, ani=False, r0=0, r1=None, labels=None, device=False):
    """-> (labels as numpy [n or n + 1 with the sentinel], n_clusters).  labels: None (fresh) or a numpy array to continue from;
    device: the array goes through a device tensor."""
    skl, ctx = sp.skl, sp.ctx
    g = ctx.sketches(sp.bins, sp.n, sp.kmers, sp.ss64, completeness=sp.comp)
    try:
        p = g.set_k(kmer, ani, cutoff=sp.cutoff)
        if labels is not None and device:
            import torch

            t = torch.from_numpy(labels.view(np.int32).copy()).to("cuda:0")
            torch.cuda.synchronize()
            out, count = skl.clusters_within(ctx, g, p, cap, cap2, r0, r1, labels=t)
            assert out is t
            return t.cpu().numpy().view(np.uint32), count
        return skl.clusters_within(ctx, g, p, cap, cap2, r0, r1, labels=None if labels is None else labels.copy())
    finally:
        g.close()


def check(sp, cap, cap2=INF, kmer=None, ani=False, r0=0, r1=None, nontrivial=False, continuing=False):
    """The fresh call (and, `continuing`, the call continued from the identity on either side, sentinel behind the labels)
    gives the oracle's labels and count."""
    want, n_want = expected(sp, cap, cap2, kmer, ani, r0, r1)
    if nontrivial:
        assert_nontrivial(want)
    got, n_got = run(sp, cap, cap2, kmer, ani, r0, r1)
    s = sizes_of(want)
    print(f"n={sp.n} kmer={kmer} ani={ani} cap=({cap}, {cap2}) rows=({r0}, {r1}): {n_want} clusters, largest {s[0]}, {int((s == 1).sum())} singletons; got {n_got}")
    assert got.dtype == np.uint32 and got.shape == (sp.n,)
    assert np.array_equal(got, want) and n_got == n_want
    assert np.array_equal(got[got], got)
    name = sp.ctx.last_kernel()
    pairs = sp.n >= 2 and sp.start(sp.n if r1 is None else r1) > sp.start(r0)
    assert "cluster_flatten_kernel" in name and "cluster_count_kernel" in name and (("cluster_union_kernel" in name) == pairs), name
    assert not pairs or name.index("kernel") < name.index("cluster_union"), name          # the dense kernel is named first
    if continuing:
        for device in (False, True):
            start = np.append(np.arange(sp.n, dtype=np.uint32), np.uint32(SENT))
            got, n_got = run(sp, cap, cap2, kmer, ani, r0, r1, labels=start, device=device)
            assert np.array_equal(got[:-1], want) and n_got == n_want and got[-1] == SENT
    return want, n_want


@pytest.fixture()
def sp65(oracle, skl, gpu_ctx):
    return space(oracle, skl, gpu_ctx, "sp65", clustered(65, 4))


# ---- 1. small ----

@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_small(oracle, skl, gpu_ctx, n):
    sp = space(oracle, skl, gpu_ctx, ("small", n), clustered(n, 1 if n < 4 else 4))
    if n == 1:
        for cap in (0.0, 0.5, 2.0):
            want, count = check(sp, cap, continuing=True)
            assert want.tolist() == [0] and count == 1
        return
    below, _stored, above = caps_of(sp)
    assert below is not None
    want, count = check(sp, below, continuing=True)                 # a cap below every value: the identity
    assert np.array_equal(want, np.arange(n)) and count == n
    want, count = check(sp, above, continuing=True)                 # a cap above every value: one cluster
    assert not want.any() and count == 1
    if n < 65:
        return
    d = sp.dense()
    assert ((d[:, 0] <= np.float32(0.1)) | (d[:, 0] == np.float32(1.0))).all()          # nothing anywhere near the cap of 0.5 (the close values end at 0.066)
    want, count = check(sp, 0.5, nontrivial=True, continuing=True)  # set_r's own clusters: sample s belongs to s % 4
    assert count == 4 and np.array_equal(want, np.arange(n) % 4)
    cap = float(np.quantile(d[:, 0].astype(np.float64), 0.1))
    want, count = check(sp, cap, nontrivial=True)
    assert 4 < count < n
    close = d[d[:, 0] <= np.float32(cap), 1]
    cap2 = float(np.median(close))
    both, count_both = check(sp, cap, cap2, nontrivial=True)        # the second cap removes edges: more clusters
    assert count_both > count


# ---- 2. a path graph: the union-find's hard case ----

def path_bins(order):
    """300 samples of 4 lengths x 512 bins.  Sample t of the CHAIN is sample t - 1 with the 32 bins from (32 t) % 512 replaced
    at every length by fresh values; at t in {0, 1, 2, 100, 299} it is a wholly fresh sketch: chains 2..99 and 100..298, and
    three samples on their own.  Sample order[t] of the slab is sample t of the chain."""
    n, nb = 300, SS64 * 64
    rng = np.random.default_rng(20240229)
    vals = np.empty((n, len(KMERS), nb), dtype=np.uint16)
    for t in range(n):
        if t in (0, 1, 2, 100, 299):
            vals[t] = rng.integers(0, 1 << 14, size=(len(KMERS), nb))
        else:
            vals[t] = vals[t - 1]
            a = (32 * t) % nb
            vals[t, :, a:a + 32] = rng.integers(0, 1 << 14, size=(len(KMERS), 32))
    out = np.empty_like(vals)
    out[order] = vals
    return synth.bitslice(out).reshape(n, -1)


PATH_ORDERS = {"chain": np.arange(300), "reversed": np.arange(300)[::-1].copy(), "permuted": np.random.default_rng(7).permutation(300)}


@pytest.mark.parametrize("band", [None, 1, 64])
@pytest.mark.parametrize("order", sorted(PATH_ORDERS))
def test_path_graph(oracle, skl, gpu_ctx, set_switch, order, band):
    """Single-k, because with the same Jaccard index at every length the core/accessory fit is degenerate."""
    perm = PATH_ORDERS[order]
    sp = space(oracle, skl, gpu_ctx, ("path", order), lambda: (path_bins(perm), 300, KMERS, SS64))
    d = sp.dense(21)[:, 0].astype(np.float64)
    chain_pos = np.empty(300, dtype=np.int64)
    chain_pos[perm] = np.arange(300)                                 # slab sample -> position in the chain
    ti, tj = chain_pos[sp.i.astype(np.int64)], chain_pos[sp.j.astype(np.int64)]
    lo, hi = np.minimum(ti, tj), np.maximum(ti, tj)
    adjacent = (hi - lo == 1) & ~np.isin(hi, (1, 2, 100, 299))
    assert adjacent.sum() == 295
    gap = (float(d[adjacent].max()), float(d[~adjacent].min()))
    print(f"path graph, {order}: adjacent pairs at {d[adjacent].min():.4f} .. {gap[0]:.4f}, every other pair >= {gap[1]:.4f}")
    assert gap[0] + 0.01 < gap[1]
    cap = 0.5 * (gap[0] + gap[1])
    want, count = expected(sp, cap, kmer=21)
    assert int((d <= np.float32(cap)).sum()) == 295 and sizes_of(want).tolist() == [199, 98, 1, 1, 1] and count == 5
    if order == "permuted":                                          # the lowest index sits inside a path, not at its end
        root = int(want[perm[150]])
        assert 100 < chain_pos[root] < 298
    if band is not None:
        set_switch("SKL_PAIRS_BAND", band)
    check(sp, cap, kmer=21, nontrivial=True, continuing=band is None)
    assert (" bands)" in sp.ctx.last_kernel()) == (band is not None)


# ---- 3. chunks ----

@pytest.mark.parametrize("extra", [1, 2])
def test_one_chunk_and_one_more(oracle, skl, gpu_ctx, extra):
    chunk = consts()[0]
    n = chunk + extra                                                # row 0 holds chunk (+ 1) pairs
    sp = space(oracle, skl, gpu_ctx, ("chunk", n), clustered(n, 40))
    assert sp.start(1) - sp.start(0) == chunk + extra - 1
    d = sp.dense()
    # row 0 alone: the star of sample 0's neighbours, everything else a singleton
    want, count = check(sp, 0.5, r0=0, r1=1, nontrivial=True)
    near = np.flatnonzero(d[:n - 1, 0] <= np.float32(0.5)) + 1
    assert near.size >= 2 and count == n - near.size and not want[near].any() and np.array_equal(np.delete(want, near), np.delete(np.arange(n), near))
    # the whole call.  Not set_r's own 40 clusters: the oracle's fit gives a few unrelated pairs a core distance of 0 (all their
    # Jaccard values at the floor), and those pairs join clusters -- 21 components at n = 2 049, the largest of 666
    want, count = check(sp, 0.5, nontrivial=True)
    assert count <= 40 and sizes_of(want)[0] >= n // 40
    cap = float(np.quantile(d[:, 0].astype(np.float64), 0.01))       # long chains, many untouched chunks
    want, count = check(sp, cap, nontrivial=True)
    assert 40 < count < n
    check(sp, cap, r0=n - 3, r1=n - 1)                               # the triangle's last two rows


# ---- 4. more chunks than one scan step, mostly empty; all lanes on one root ----

def test_mostly_empty_chunks_and_one_contended_root(oracle, skl, gpu_ctx):
    """2 100 unrelated samples, then 100 copies of one: a cap of 0 leaves the copies as one cluster of 100 at label 2100 and nearly
    every other sample on its own (the oracle's fit puts 60 unrelated pairs at a core distance of 0 too: 2 041 clusters, not
    2 101); a cap of 2.0 makes every one of 2.4 M pairs hook into one tree."""
    def make():
        a = synth.set_r(2100, KMERS, SS64, n_clusters=2100)
        b = np.repeat(synth.set_r(1, KMERS, SS64, n_clusters=1, seed=synth.SEED_R + 5), 100, axis=0)
        return np.concatenate([a, b]), 2200, KMERS, SS64

    sp = space(oracle, skl, gpu_ctx, "clustered2200", make)
    want, count = check(sp, 0.0, nontrivial=True, continuing=True)
    assert (want[2100:] == 2100).all() and int((want == 2100).sum()) == 100
    assert 2000 < count <= 2101 and int((sizes_of(want) == 1).sum()) > 0.9 * 2100
    assert (sp.dense()[:, 0] <= np.float32(2.0)).all()
    want, count = check(sp, 2.0, continuing=True)
    assert count == 1 and not want.any()


# ---- 5. row ranges, CONTINUE and the merge ----

RANGES = ((0, 7), (7, 8), (8, 40), (40, 65))


@pytest.mark.parametrize("device", [False, True])
def test_row_ranges_chained_and_merged(sp65, device):
    skl, ctx, n = sp65.skl, sp65.ctx, sp65.n
    d = sp65.dense()
    for cap in (0.5, float(np.quantile(d[:, 0].astype(np.float64), 0.1))):
        whole, n_whole = expected(sp65, cap)
        assert_nontrivial(whole)
        # chained with CONTINUE: every step is the oracle's components of the rows so far
        labels = np.append(np.arange(n, dtype=np.uint32), np.uint32(SENT))
        for r0, r1 in RANGES:
            labels, count = run(sp65, cap, r0=r0, r1=r1, labels=labels, device=device)
            want, n_want = expected(sp65, cap, r0=0, r1=r1)
            assert np.array_equal(labels[:-1], want) and count == n_want and labels[-1] == SENT
        assert np.array_equal(labels[:-1], whole) and count == n_whole
        # empty ranges change nothing
        for r0, r1 in ((20, 20), (65, 65)):
            again, count = run(sp65, cap, r0=r0, r1=r1, labels=labels, device=device)
            assert np.array_equal(again, labels) and count == n_whole
            assert "cluster_union_kernel" not in ctx.last_kernel()
        # each range from the identity, folded with the merge
        parts = []
        for r0, r1 in RANGES:
            part, count = run(sp65, cap, r0=r0, r1=r1)
            want, n_want = expected(sp65, cap, r0=r0, r1=r1)
            assert np.array_equal(part, want) and count == n_want
            parts.append(part)
        assert any(not np.array_equal(p, whole) for p in parts)
        if device:
            import torch

            acc = torch.from_numpy(np.append(parts[0], np.uint32(SENT)).view(np.int32)).to("cuda:0")
            for part in parts[1:]:
                t = torch.from_numpy(part.view(np.int32).copy()).to("cuda:0")
                # (the merge takes n from the first array: hand it the n labels, not the sentinel)
                out, count = skl.clusters_merge(ctx, acc[:n], t)
            merged = acc.cpu().numpy().view(np.uint32)
            assert merged[-1] == SENT
            merged = merged[:-1]
        else:
            merged = parts[0]
            for part in parts[1:]:
                before = merged.copy()
                out, count = skl.clusters_merge(ctx, merged, part)
                assert out is not merged and np.array_equal(merged, before)          # a new array: the inputs are untouched
                merged = out
        assert np.array_equal(merged, whole) and count == n_whole
        assert "cluster_merge_kernel" in ctx.last_kernel()
    with pytest.raises(skl.SklError) as e:
        run(sp65, 0.5, r0=5, r1=n + 1)
    assert e.value.code == skl.ERR_INVALID_ARG


def test_merge_textbook_case(skl, gpu_ctx):
    """A links (0,1) and (2,3), B links (1,2): one cluster."""
    a, b = np.array([0, 0, 2, 2], dtype=np.uint32), np.array([0, 1, 1, 3], dtype=np.uint32)
    out, count = skl.clusters_merge(gpu_ctx, a, b)
    assert out.tolist() == [0, 0, 0, 0] and count == 1 and a.tolist() == [0, 0, 2, 2] and b.tolist() == [0, 1, 1, 3]
    out, count = skl.clusters_merge(gpu_ctx, np.arange(5, dtype=np.uint32), np.array([0, 0, 2, 1, 4], dtype=np.uint32))
    assert out.tolist() == [0, 0, 2, 0, 4] and count == 3


# ---- 6. refused inputs ----

def raw_call(skl, ctx, g, p, cap, cap2, labels_addr, dev, flags, count_ref, r0=0, r1=None):
    return skl.load().skl_self_clusters_within(ctx._h, g._h, C.byref(p), r0, g.n if r1 is None else r1, cap, cap2, labels_addr, dev, flags, count_ref)


def test_refused_inputs(sp65):
    """The guard refuses a label beyond its index before any label is followed: the call returns SKL_ERR_INVALID_ARG from the
    check kernel's error word, no union, merge or flatten kernel is launched with the bad value, and the array is unchanged."""
    import torch

    skl, ctx, n = sp65.skl, sp65.ctx, sp65.n
    good, _count = run(sp65, 0.5)
    for at, value in ((0, 1), (3, 7), (5, n)):
        bad = good.copy()
        bad[at] = value
        for device in (False, True):
            arr = torch.from_numpy(bad.view(np.int32).copy()).to("cuda:0") if device else bad.copy()
            g = ctx.sketches(sp65.bins, n, sp65.kmers, sp65.ss64)
            with pytest.raises(skl.SklError) as e:
                skl.clusters_within(ctx, g, g.set_k(), 0.5, labels=arr)
            assert e.value.code == skl.ERR_INVALID_ARG and "labels[i] <= i" in e.value.message
            g.close()
            after = arr.cpu().numpy().view(np.uint32) if device else arr
            assert np.array_equal(after, bad)
            # the merge checks both sides the same way
            other = torch.from_numpy(good.view(np.int32).copy()).to("cuda:0") if device else good.copy()
            for x, y in ((arr, other), (other, arr)):
                with pytest.raises(skl.SklError) as e:
                    skl.clusters_merge(ctx, x, y)
                assert e.value.code == skl.ERR_INVALID_ARG
            if device:
                assert np.array_equal(arr.cpu().numpy().view(np.uint32), bad) and np.array_equal(other.cpu().numpy().view(np.uint32), good)
    # caps, as the within calls refuse them
    for cap, cap2 in ((float("nan"), INF), (0.1, float("nan")), (-1e-9, INF), (-1.0, 0.5)):
        with pytest.raises(skl.SklError) as e:
            run(sp65, cap, cap2)
        assert e.value.code == skl.ERR_INVALID_ARG
    # null pointers, unknown flags
    g = ctx.sketches(sp65.bins, n, sp65.kmers, sp65.ss64)
    p = g.set_k()
    labels = np.arange(n, dtype=np.uint32)
    count = C.c_uint64(77)
    assert raw_call(skl, ctx, g, p, 0.5, INF, None, 0, 0, C.byref(count)) == skl.ERR_INVALID_ARG
    assert raw_call(skl, ctx, g, p, 0.5, INF, labels.ctypes.data, 0, 0, None) == skl.ERR_INVALID_ARG
    assert raw_call(skl, ctx, g, p, 0.5, INF, labels.ctypes.data, 0, 2, C.byref(count)) == skl.ERR_INVALID_ARG
    assert np.array_equal(labels, np.arange(n))
    L = skl.load()
    assert L.skl_clusters_merge(ctx._h, None, labels.ctypes.data, n, 0, C.byref(count)) == skl.ERR_INVALID_ARG
    assert L.skl_clusters_merge(ctx._h, labels.ctypes.data, None, n, 0, C.byref(count)) == skl.ERR_INVALID_ARG
    assert L.skl_clusters_merge(ctx._h, labels.ctypes.data, labels.ctypes.data, n, 0, None) == skl.ERR_INVALID_ARG
    count.value = 77
    assert L.skl_clusters_merge(ctx._h, None, None, 0, 0, C.byref(count)) == skl.OK and count.value == 0
    assert raw_call(skl, ctx, g, p, 0.5, INF, labels.ctypes.data, 0, 0, C.byref(count)) == skl.OK and count.value == 4
    g.close()


# ---- 7. modes ----

def test_ani_turns_the_test_round(oracle, skl, gpu_ctx):
    sp = space(oracle, skl, gpu_ctx, "sp63", clustered(63, 4, seed=2))
    _below, stored, above = caps_of(sp, kmer=21, ani=True)
    d = sp.dense(21, True)[:, 0]
    assert int((d >= np.float32(0.98)).sum()) not in (0, d.size)
    want, count = check(sp, 0.02, kmer=21, ani=True, nontrivial=True)      # close pairs have a HIGH identity
    assert count < sp.n
    check(sp, stored, kmer=21, ani=True)
    want, count = check(sp, above, kmer=21, ani=True)
    assert count == 1


@pytest.mark.parametrize("kmer", [None, 21])
def test_with_a_completeness_vector(oracle, skl, gpu_ctx, kmer):
    def make():
        bins, n, kmers, ss64 = clustered(65, 4)()
        return bins, n, kmers, ss64, np.linspace(0.75, 1.0, n)

    sp = space(oracle, skl, gpu_ctx, "sp65comp", make)
    v = sp.dense(kmer)[:, 0]
    counts = []
    for share in (0.05, 0.3, 0.9):
        cap = gap_cap(v, share)                                      # (asserts the gap on the CPU)
        counts.append(check(sp, cap, kmer=kmer, continuing=share == 0.3)[1])
    assert counts[0] >= counts[1] >= counts[2] and counts[0] > counts[2]
    check(sp, gap_cap(v, 0.3), kmer=kmer, r0=11, r1=29)


def test_nan_semantics_inputs(oracle, skl, gpu_ctx):
    """The inputs tests/test_gpu_edges.py takes the reference's NaN semantics from: a completeness of 0 under cutoff 0.  The NaN
    of those inputs lives inside the fit: the oracle stores (0, 0) for every pair of sample 3, plain numbers that pass any cap,
    so the clusters must show what the dense call stores -- sample 3 linked to everyone -- and a pair that did hold a NaN
    would never link it (that a NaN value never passes is the native check's, tests/test_within_plan_cpu.py)."""
    def make():
        kmers, ss64, n = [17, 21, 25], 8, 12
        comp = np.ones(n)
        comp[3] = 0.0
        return synth.set_r(n, kmers, ss64, n_clusters=2), n, kmers, ss64, comp, None, 0.0

    sp = space(oracle, skl, gpu_ctx, "nan12", make)
    d = sp.dense()
    nan = np.isnan(d).any(axis=1)
    for share in (0.2, 0.6):
        want, _count = check(sp, gap_cap(d[:, 0], share))
    pairs3 = (sp.i == 3) | (sp.j == 3)
    want, count = check(sp, 2.0)
    if np.isnan(d[pairs3, 0]).all():
        assert want[3] == 3 and not (np.delete(want, 3) == 3).any()
    print(f"{int(nan.sum())} pairs hold a NaN; cap 2.0: {count} clusters, labels {want.tolist()}")


# ---- 8. Python ----

def test_python_calls(sp65):
    skl, ctx, n = sp65.skl, sp65.ctx, sp65.n
    d = sp65.dense()
    cap = float(np.quantile(d[:, 0].astype(np.float64), 0.1))
    want, n_want = expected(sp65, cap)
    assert_nontrivial(want)
    g = ctx.sketches(sp65.bins, n, sp65.kmers, sp65.ss64)
    p = g.set_k()
    labels, count = skl.clusters_within(ctx, g, p, cap)
    assert isinstance(labels, np.ndarray) and labels.dtype == np.uint32 and labels.shape == (n,) and isinstance(count, int)
    assert np.array_equal(labels, want) and count == n_want
    rep, ids = skl.dereplicate(ctx, g, p, cap)
    assert ids.dtype == np.uint32 and np.array_equal(ids, np.flatnonzero(want == np.arange(n))) and rep.n == n_want
    # representatives of different clusters are never within the cap of each other
    assert skl.count_within(ctx, rep, rep.set_k(), cap) == 0
    # ... and they are the samples they claim to be: their distances are the oracle's for those ids
    got = skl.self_dists_all(ctx, rep, rep.set_k())
    pick = np.isin(sp65.i, ids) & np.isin(sp65.j, ids)
    assert got.tobytes() == d[pick].tobytes()
    rep.close()
    # the source slab is still usable
    labels, count = skl.clusters_within(ctx, g, p, cap, np.inf, 0, None)
    assert np.array_equal(labels, want) and count == n_want
    assert skl.count_within(ctx, g, p, cap) == int((d[:, 0] <= np.float32(cap)).sum())
    g.close()
