"""cand_reference.py against the brute-force definition, and every input builder of cand_inputs.py at its real size: an input
that misses the edge it is named after, or whose longest list exceeds its cap, fails here -- without a GPU."""
import numpy as np
import pytest

import cand_inputs as ci
from cand_reference import bin_groups, candidate_lists, list_lengths, row_list
from test_gpu_precluster import candidates


def small_inputs():
    rng = np.random.default_rng(42)
    out = {}
    for n, S, alphabet in [(1, 1, 2), (2, 1, 1), (7, 1, 3), (40, 1, 5), (97, 3, 30), (150, 6, 50), (300, 4, 25), (299, 9, 4000)]:
        out[f"random n={n} S={S}"] = rng.integers(0, alphabet, size=(n, S))
    dup = rng.integers(0, 60000, size=(120, 5))
    dup[::7] = dup[3]                                           # duplicate rows
    out["duplicate rows"] = dup
    shared = ci.unique_bins(rng, 200, 4).astype(np.int64)
    shared[:, 2] = 9                                            # an all-shared bin
    out["all-shared bin"] = shared
    ends = rng.integers(0, 4, size=(250, 3)) * 21845            # values 0, 21845, 43690, 65535
    out["values 0 and 65535"] = ends
    none = ci.unique_bins(rng, 64, 8)
    out["no candidates"] = none
    return out


SMALL = small_inputs()


@pytest.mark.parametrize("name", sorted(SMALL))
def test_reference_equals_brute_force(name):
    skq = SMALL[name].astype(np.uint16)
    offs, cols = candidates(skq)
    got = candidate_lists(skq)
    assert got.offs.dtype == np.uint64 and got.cols.dtype == np.uint32
    assert np.array_equal(got.offs, offs) and np.array_equal(got.cols, cols)
    n = skq.shape[0]
    for b, g in enumerate(got.groups):                          # the groups as a counting sort lays them out
        col = skq[:, b]
        assert g.length.sum() == n and np.array_equal(np.sort(g.order), np.arange(n))
        for v, s, l in zip(g.value, g.start, g.length):
            assert s == (col < v).sum() and l == (col == v).sum()
            assert (col[g.order[s:s + l]] == v).all()
    if name == "values 0 and 65535":
        assert {0, 65535} <= set(got.groups[0].value.tolist())
    if name == "all-shared bin":
        assert (list_lengths(got) == n - 1).all()
    if name == "no candidates":
        assert got.cols.size == 0


@pytest.mark.parametrize("n", ci.N_ALIGNMENT)
def test_input_n_alignment(n):
    inp = ci.n_alignment(n)
    assert inp.skq.shape == (n, 7)
    if n == 1:
        assert inp.lists.cols.size == 0


def test_input_group_ladder():
    inp = ci.group_ladder()
    assert inp.skq.shape == (1543, 8) and list_lengths(inp.lists).max() >= 513


def test_input_slack_tail():
    assert ci.slack_tail().skq.shape == (1021, 3)


@pytest.mark.parametrize("S", ci.BIN_COUNTS)
def test_input_bin_blocks(S):
    inp, only = ci.bin_blocks(S)
    assert inp.skq.shape == (203, S)
    assert [b for b, _, _ in only] == ci.special_bins(S) and S - 1 in ci.special_bins(S)
    assert ci.special_bins(385) == [191, 192, 383, 384] and ci.special_bins(192) == [191] and ci.special_bins(193) == [191, 192]


def test_input_unbalanced_blocks():
    inp, partners = ci.unbalanced_blocks()
    assert inp.skq.shape == (2049, 384) and all(b % 4 == 0 for x in partners for b in np.flatnonzero(inp.skq[x] == inp.skq[0]))


@pytest.mark.parametrize("n", sorted(ci.WORDS_N))
def test_input_bitmap_words(n):
    assert ci.bitmap_words(n).skq.shape == (n, 4)


def test_input_empty_full_and_symmetric():
    ci.ragged_small()
    ci.everybody()
    inp, rows = ci.symmetric_items()
    for items, i in rows.items():
        row = row_list(inp.lists, i)
        assert -(-int((row > i).sum()) // 64) == items and int((row < i).sum()) % 64


def test_input_beyond_the_cap():
    n = ci.two_halves().skq.shape[0]
    assert n * 1000 * 12 >= 32 << 20 > n * 998 * 12
    assert ci.copy_back_batches(n, 1000) == 4 and ci.copy_back_batches(n, 998) == 1
    assert [n * b // 4 for b in range(5)] == [0, 700, 1400, 2100, 2801]
    big = ci.everybody(2600, 1, 0)
    assert (list_lengths(big.lists) == 2599).all() and 2599 > 2049 > ci.LIST_CAP


def test_limit_lists_from_arithmetic():
    """limit_lists / limit_expected against the reference at a size where groups of 4 and 6 occur, and the figures of the limit."""
    n = 3 * 131072 - 1000
    skq = ci.limit_skq(n)
    ref = candidate_lists(skq)
    ids = ci.limit_lists(n)
    assert ids.shape[1] == 5 and np.array_equal(ids[ids >= 0].astype(np.uint32), ref.cols)
    assert np.array_equal((ids >= 0).sum(axis=1), list_lengths(ref))
    dist3 = np.array([[0.0, 0.25, 0.5], [0.25, 0.0, 0.75], [0.5, 0.75, 0.0]], dtype=np.float32)
    idx, d0, total = ci.limit_expected(n, dist3, 7)
    assert total == ref.cols.size and idx.shape == (n, 7)
    for i in (0, 1, 2, 131071, 131072, n - 1):
        row = row_list(ref, i).astype(np.int64)
        want = sorted((float(dist3[i % 3, j % 3]), int(j)) for j in row)
        want += [(1.0, i)] * (7 - len(want))
        assert [(float(d), int(j)) for j, d in zip(idx[i], d0[i])] == want
    n_words, per = ci.words_per_thread(ci.MAX_SAMPLES)
    assert ci.MAX_SAMPLES == 1294336 and per == 158 and (2 * ci.CG_BIN_BLOCK + n_words) * 4 == 163328
    groups = bin_groups(ci.limit_skq(ci.MAX_SAMPLES)[:, 0])
    assert sorted(set(groups.length.tolist())) == [18, 20]
