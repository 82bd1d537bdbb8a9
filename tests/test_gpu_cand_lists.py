"""The precluster candidate path where lists, groups and batches are cut: cand_gen.hip (counting sort of the index bins, one
workgroup per row OR-ing groups into an LDS bitmap), pair_cand.hip (pair_cand_rows_kernel<TRIPS>, its symmetric write-back and
binary search) and capi_cand.cpp (the ragged selection and copy-back).

WHOLE lists are observed: knn = the longest list of the input, so every member of every list and every key -- the symmetric
copies included -- comes back and is compared, exactly, with the oracle's self_dists_knn_precluster and with the lists of
cand_reference.py.  The inputs are built by cand_inputs.py, which asserts that each holds the edge it is named after
(tests/test_cand_reference_cpu.py runs those assertions without a GPU); profiles/cand_lists_tests.md lists the cases."""
import time

import numpy as np
import pytest

import cand_inputs as ci
from cand_reference import candidate_lists, list_lengths, row_list
from sketchlib.rust_amd import synth

pytestmark = pytest.mark.gpu

KMERS, SS64 = [17, 21], 2        # the second length is the one asked for: k_begin > 0


def slab(n, kmers=KMERS, ss64=SS64, clusters=5, near_copies=False):
    """Clustered sketches (sample s in cluster s % clusters): keys that tell pairs apart; near_copies: a third of the slab
    is one sketch, so that most keys tie."""
    bins = synth.set_r(n, kmers, ss64, n_clusters=clusters)
    if near_copies:
        bins[::3] = bins[0]
    return bins


@pytest.fixture()
def ref_ties(skl, gpu_ctx):
    gpu_ctx.set_knn_ties(skl.TIES_REFERENCE)
    yield
    gpu_ctx.set_knn_ties(skl.TIES_CANONICAL)


def device_lists(skl, ctx, g, p, skq, lists=None):
    """self_dists_knn_shared_bins at knn = max(1, longest reference list) -> (knn, idx, d0, total, [(ids, values) per row up
    to the padding]).  Padding is (i, 1.0) and a row never lists itself: everything behind the first idx == i is padding."""
    lists = candidate_lists(skq) if lists is None else lists
    n = skq.shape[0]
    knn = max(1, int(list_lengths(lists).max(initial=0)))
    idx, d0, total = skl.self_dists_knn_shared_bins(ctx, g, p, knn, skq)
    pad = idx == np.arange(n, dtype=np.uint64)[:, None]
    lens = np.where(pad.any(axis=1), pad.argmax(axis=1), knn)
    behind = np.arange(knn)[None, :] >= lens[:, None]
    assert np.array_equal(pad, behind), "a row lists itself, or lists something behind its padding"
    assert (d0[behind] == 1.0).all()
    return knn, idx, d0, total, [(idx[i, :lens[i]], d0[i, :lens[i]]) for i in range(n)]


def oracle_knn(oracle, bins, n, kmers, ss64, skq, knn, ties=None):
    if knn >= n:       # (the oracle, like the reference's caller, wants knn < n): one sample, one padded row
        assert n == 1
        return np.zeros((1, knn), dtype=np.uint64), np.ones((1, knn), dtype=np.float32)
    o = oracle.Sketches(bins, n, kmers, ss64)
    exp = oracle.self_dists_knn_precluster(o, skq, knn, len(kmers) - 1, ties=oracle.TIES_CANONICAL if ties is None else ties, threads=16)
    return exp["idx"], exp["d0"]


def assert_rows_equal(idx, d0, exp_idx, exp_d0, what=""):
    bad = np.flatnonzero((idx != exp_idx).any(axis=1) | (d0 != exp_d0).any(axis=1))
    if bad.size:
        r = int(bad[0])
        c = int(np.flatnonzero((idx[r] != exp_idx[r]) | (d0[r] != exp_d0[r]))[0])
        raise AssertionError(f"{what}: {bad.size} rows differ, first row {r} at position {c}: device ({idx[r, c]}, {d0[r, c]!r}), "
                             f"oracle ({exp_idx[r, c]}, {exp_d0[r, c]!r})")


def assert_whole_lists(oracle, skl, ctx, inp, bins, kmers=KMERS, ties=None, distinct=3):
    """Every list whole and every key, exactly: the oracle at the same knn, the reference CSR, the total."""
    skq, lists = inp.skq, inp.lists
    n = skq.shape[0]
    g = ctx.sketches(bins, n, kmers, SS64)
    try:
        knn, idx, d0, total, rows = device_lists(skl, ctx, g, g.set_k(kmers[-1]), skq, lists)
    finally:
        g.close()
    assert "pair_cand_rows_kernel" in ctx.last_kernel()
    exp_idx, exp_d0 = oracle_knn(oracle, bins, n, kmers, SS64, skq, knn, ties)
    if distinct:       # keys that distinguish pairs: an unstored or misplaced symmetric copy cannot hide among ties
        lens = list_lengths(lists)
        assert any(np.unique(exp_d0[i, :lens[i]]).size >= distinct for i in np.argsort(-lens)[:50])
    for i, (ids, _) in enumerate(rows):
        assert np.array_equal(np.sort(ids), row_list(lists, i)), f"the members of row {i}'s list"
    assert total == lists.cols.size
    assert_rows_equal(idx, d0, exp_idx, exp_d0, f"n = {n}, S = {skq.shape[1]}, knn = {knn}")
    return idx, d0


# ---- cand_gen.hip: groups and lists ----
@pytest.mark.parametrize("n", ci.N_ALIGNMENT)
def test_n_alignment(oracle, skl, gpu_ctx, n):
    """base = bin * n at every residue mod 4: the aligned-down 16-byte read of a group that starts in the previous bin's members."""
    assert_whole_lists(oracle, skl, gpu_ctx, ci.n_alignment(n), slab(n), distinct=3 if n >= 31 else 0)


def test_group_length_and_start(oracle, skl, gpu_ctx):
    """Groups of 1, 2, 3, 4, 255, 256, 257, 260, 511 and 513 members, each starting at every residue mod 4 of the members
    array; values at the first and last counter of a scan thread."""
    assert_whole_lists(oracle, skl, gpu_ctx, ci.group_ladder(), slab(ci.LADDER_N))


def test_last_block_in_the_slack(oracle, skl, gpu_ctx):
    """n * S = 3 (mod 4): the last group's last 16-byte block ends in the slack behind the members array; the first group starts at element 0."""
    assert_whole_lists(oracle, skl, gpu_ctx, ci.slack_tail(), slab(1021))


@pytest.mark.parametrize("S", ci.BIN_COUNTS)
def test_bins_per_block_and_trip(oracle, skl, gpu_ctx, S):
    """Bin counts around the 16 bins of a trip and the 192 of a block; a candidate that only the last bin, the last bin of a
    block or the first of the next yields."""
    inp, only = ci.bin_blocks(S)
    idx, _ = assert_whole_lists(oracle, skl, gpu_ctx, inp, slab(203), distinct=0)
    for _, i, j in only:
        assert idx[i, 0] == j and idx[j, 0] == i


def test_a_wave_far_behind_in_the_first_block_of_bins(oracle, skl, gpu_ctx):
    """Two blocks of 192 bins; wave 0 reads the parked bounds of the first block's later bins long after the other waves
    have left the block: the bounds must not have been replaced by the second block's."""
    inp, partners = ci.unbalanced_blocks()
    idx, _ = assert_whole_lists(oracle, skl, gpu_ctx, inp, slab(inp.skq.shape[0]))
    assert set(partners.tolist()) <= set(idx[0].tolist())


@pytest.mark.parametrize("n", sorted(ci.WORDS_N))
def test_several_bitmap_words_per_thread(oracle, skl, gpu_ctx, n):
    """Step C with 3 (2) words per thread and idle trailing threads: ascending output across the threads' ranges, the last word, id n - 1."""
    assert_whole_lists(oracle, skl, gpu_ctx, ci.bitmap_words(n), slab(n))


def test_empty_rows_and_empty_symmetric_halves(oracle, skl, gpu_ctx):
    assert_whole_lists(oracle, skl, gpu_ctx, ci.ragged_small(), slab(131))


def test_everybody_group(oracle, skl, gpu_ctx):
    assert_whole_lists(oracle, skl, gpu_ctx, ci.everybody(), slab(130))


# ---- pair_cand.hip: the symmetric halves ----
def test_symmetric_work_items(oracle, skl, gpu_ctx):
    """Rows whose upper half takes 2, 3 and 4 work items and does not start at a multiple of 64 within the list."""
    inp, rows = ci.symmetric_items()
    assert ci.work_items(inp.lists, rows[2])[1] == 2 and ci.work_items(inp.lists, rows[3])[1] == 3
    assert_whole_lists(oracle, skl, gpu_ctx, inp, slab(700))


@pytest.mark.ab_library
def test_symmetric_and_row_order_switches(oracle, skl, gpu_ctx, set_switch):
    """SKL_CAND_SYMMETRIC=0 (every listed pair evaluated from its own row) and SKL_CAND_ROW_ORDER=0 (sample order): identical arrays."""
    inp, _ = ci.symmetric_items()
    bins = slab(700)
    got = []
    for name in (None, "SKL_CAND_SYMMETRIC", "SKL_CAND_ROW_ORDER"):
        if name:
            set_switch(name, "0")
        got.append(assert_whole_lists(oracle, skl, gpu_ctx, inp, bins))
        if name:
            set_switch(name, None)
    for idx, d0 in got[1:]:
        assert np.array_equal(idx, got[0][0]) and np.array_equal(d0, got[0][1])


# ---- reference ties over whole lists ----
@pytest.mark.parametrize("which", ["ladder", "words"])
def test_reference_ties_over_whole_lists(oracle, skl, gpu_ctx, ref_ties, which):
    inp = ci.group_ladder() if which == "ladder" else ci.bitmap_words(8193)
    assert_whole_lists(oracle, skl, gpu_ctx, inp, slab(inp.skq.shape[0], near_copies=True), ties=oracle.TIES_RUST_HEAP)


# ---- pair_cand_rows_kernel<TRIPS> of the product library past each trip edge ----
@pytest.mark.parametrize("ss64", [32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 200])
def test_sketch_sizes_past_each_trip_edge(oracle, skl, gpu_ctx, ss64):
    n = 150
    bins = synth.set_r(n, KMERS, ss64, n_clusters=11)
    skq = np.random.default_rng(ss64).integers(0, 25, size=(n, 4), dtype=np.uint16)
    lists = candidate_lists(skq)
    longest = int(list_lengths(lists).max())
    assert 6 < longest < n
    g = gpu_ctx.sketches(bins, n, KMERS, ss64)
    for knn in (6, longest):
        exp_idx, exp_d0 = oracle_knn(oracle, bins, n, KMERS, ss64, skq, knn)
        idx, d0 = skl.self_dists_knn_candidates(gpu_ctx, g, g.set_k(21), knn, lists.offs, lists.cols)
        assert "pair_cand_rows_kernel" in gpu_ctx.last_kernel()
        assert_rows_equal(idx, d0, exp_idx, exp_d0, f"host lists, ss64 = {ss64}, knn = {knn}")
        idx, d0, total = skl.self_dists_knn_shared_bins(gpu_ctx, g, g.set_k(21), knn, skq)
        assert "pair_cand_rows_kernel" in gpu_ctx.last_kernel()
        assert total == lists.cols.size
        assert_rows_equal(idx, d0, exp_idx, exp_d0, f"device lists, ss64 = {ss64}, knn = {knn}")
    g.close()


# ---- capi_cand.cpp: the branches of knn_from_device_csr ----
@pytest.fixture(params=["canonical", "reference"])
def tie_rule(request, skl, gpu_ctx, oracle):
    reference = request.param == "reference"
    if reference:
        gpu_ctx.set_knn_ties(skl.TIES_REFERENCE)
    yield reference, (oracle.TIES_RUST_HEAP if reference else oracle.TIES_CANONICAL)
    gpu_ctx.set_knn_ties(skl.TIES_CANONICAL)


def test_four_copy_back_batches(oracle, skl, gpu_ctx, tie_rule):
    """2 801 rows x 1 000 neighbours x 12 B >= 32 MiB: four batches of 700/700/700/701 rows; x 998: one batch."""
    near_copies, ties = tie_rule
    inp = ci.two_halves()
    n, kmers = inp.skq.shape[0], [21]
    assert n * 1000 * 12 >= (32 << 20) > n * 998 * 12
    assert ci.copy_back_batches(n, 1000) == 4 and ci.copy_back_batches(n, 998) == 1
    bins = slab(n, kmers, clusters=7, near_copies=near_copies)
    g = gpu_ctx.sketches(bins, n, kmers, SS64)
    for knn in (1000, 998):
        idx, d0, total = skl.self_dists_knn_shared_bins(gpu_ctx, g, g.set_k(21), knn, inp.skq)
        assert total == inp.lists.cols.size
        assert_rows_equal(idx, d0, *oracle_knn(oracle, bins, n, kmers, SS64, inp.skq, knn, ties), f"knn = {knn}")
    g.close()


def test_more_neighbours_than_the_lds_selection_holds(oracle, skl, gpu_ctx, tie_rule):
    """knn > 2 048: canonical ties collect and sort a row's items in a global scratch, reference ties keep the heaps in global memory."""
    near_copies, ties = tie_rule
    n, kmers = 2600, [21]
    inp = ci.everybody(n, 1, 0)
    bins = slab(n, kmers, clusters=7, near_copies=near_copies)
    g = gpu_ctx.sketches(bins, n, kmers, SS64)
    for knn in (2599, 2049):
        assert knn > ci.LIST_CAP
        idx, d0, total = skl.self_dists_knn_shared_bins(gpu_ctx, g, g.set_k(21), knn, inp.skq)
        assert total == n * (n - 1)
        assert_rows_equal(idx, d0, *oracle_knn(oracle, bins, n, kmers, SS64, inp.skq, knn, ties), f"knn = {knn}")
        if not near_copies:      # the same pairs through the dense kNN
            fi, fd, _ = skl.self_dists_knn(gpu_ctx, g, g.set_k(21), knn)
            assert_rows_equal(idx, d0, fi, fd, f"self_dists_knn, knn = {knn}")
    g.close()


# ---- the limit ----
def tiled_slab(oracle, gpu_ctx, n):
    """bins[i] = pattern[i % 3] on the device, and the oracle's 3 x 3 distances of the three patterns."""
    kmers = [21]
    pattern = synth.set_r(3, kmers, SS64, n_clusters=1)
    o = oracle.Sketches(pattern, 3, kmers, SS64)
    exp = oracle.self_dists_knn_precluster(o, np.zeros((3, 1), dtype=np.uint16), 2, 0, threads=1)
    dist3 = np.zeros((3, 3), dtype=np.float32)
    for i in range(3):
        dist3[i, exp["idx"][i].astype(np.int64)] = exp["d0"][i]
    off = dist3[np.triu_indices(3, 1)]
    assert np.unique(off).size == 3 and (off > 0).all() and (off < 1).all() and np.array_equal(dist3, dist3.T)
    g3 = gpu_ctx.sketches(pattern, 3, kmers, SS64)
    g = g3.select(np.arange(n, dtype=np.uint32) % 3)
    g3.close()
    return g, dist3


def test_one_sample_past_the_limit_is_refused(oracle, skl, gpu_ctx):
    limit = skl.load().skl_shared_bins_max_samples()
    assert limit == ci.MAX_SAMPLES
    n = limit + 1
    g, _ = tiled_slab(oracle, gpu_ctx, n)
    with pytest.raises(skl.SklError) as e:
        skl.self_dists_knn_shared_bins(gpu_ctx, g, g.set_k(21), 1, ci.limit_skq(n))
    g.close()
    assert str(limit) in str(e.value) and str(n) in str(e.value)
    assert_whole_lists(oracle, skl, gpu_ctx, ci.ragged_small(), slab(131))     # the context still answers


def test_at_the_limit(oracle, skl, gpu_ctx):
    """n = skl_shared_bins_max_samples(): the full LDS allotment (163 328 B) and 158 bitmap words per thread.  One bin,
    skq[i] = (i // 2) mod 65 536: groups of 18 and 20 whose members lie 131 072 ids apart; expected ids from arithmetic,
    expected distances from the oracle's 3 x 3 matrix of the three sketches the slab is tiled from.  knn = 20: whole lists
    (17 or 19 candidates) and padding."""
    n = skl.load().skl_shared_bins_max_samples()
    assert n == ci.MAX_SAMPLES and ci.words_per_thread(n) == (40448, 158)
    t0 = time.perf_counter()
    g, dist3 = tiled_slab(oracle, gpu_ctx, n)
    skq, ids = ci.limit_skq(n), ci.limit_lists(n)
    for knn in (1, 2, 20):
        t1 = time.perf_counter()
        idx, d0, total = skl.self_dists_knn_shared_bins(gpu_ctx, g, g.set_k(21), knn, skq)
        t2 = time.perf_counter()
        exp_idx, exp_d0, exp_total = ci.limit_expected(n, dist3, knn, ids)
        assert total == exp_total
        assert_rows_equal(idx, d0, exp_idx, exp_d0, f"knn = {knn}")
        print(f"at the limit: n = {n}, knn = {knn}: device call {t2 - t1:.2f} s, expectation {time.perf_counter() - t2:.2f} s")
    g.close()
    print(f"at the limit: whole test {time.perf_counter() - t0:.2f} s")
