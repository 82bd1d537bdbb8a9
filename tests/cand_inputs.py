"""Index sketches ([n, S] u16) that put cand_gen.hip, pair_cand.hip and capi_cand.cpp at the places where lists, groups and
batches are cut.  Every builder ASSERTS, from the reference of cand_reference.py, that the edge it names is present in what it
returns and that its longest list stays within LIST_CAP (the LDS selection of topk.hip) -- tests/test_cand_reference_cpu.py
runs them all without a GPU; tests/test_gpu_cand_lists.py hands them to the device."""
import functools
from collections import namedtuple

import numpy as np

from cand_reference import candidate_lists, list_lengths, row_list, start_residues

LIST_CAP = 2048            # TOPK_LDS_MAX = REFHEAP_LDS_MAX (kernels.h): knn = longest list stays in the LDS selection
CG_THREADS = 256           # cand_gen.hip
CG_BIN_BLOCK = 192         # cand_gen.hip: bins whose bounds are parked in LDS at a time
MAX_SAMPLES = 158 * 1024 * 8   # kernels.h MAX_DEVICE_CANDGEN_SAMPLES (asserted against the library by the GPU test)

Input = namedtuple("Input", "skq lists")


def _finish(skq, cap=LIST_CAP):
    skq = np.ascontiguousarray(skq, dtype=np.uint16)
    skq.setflags(write=False)
    lists = candidate_lists(skq)
    assert list_lengths(lists).max(initial=0) <= cap, "the longest list exceeds the cap of this input"
    return Input(skq, lists)


def unique_bins(rng, n, S):
    """No value twice in any bin: no candidates at all."""
    assert n <= 65536
    return np.stack([rng.permutation(65536)[:n] for _ in range(S)], axis=1).astype(np.uint16)


def words_per_thread(n):
    """cand_rows_kernel step C: (bitmap words, words per thread)."""
    n_words = (n + 31) // 32
    return n_words, (n_words + CG_THREADS - 1) // CG_THREADS


# ---- n alignment: base = bin * n at every residue mod 4 ----
N_ALIGNMENT = (1, 2, 3, 5, 31, 33, 63, 65, 127, 129, 1021, 1030)


@functools.lru_cache(maxsize=None)
def n_alignment(n):
    S = 7
    rng = np.random.default_rng(1000 + n)
    inp = _finish(rng.integers(0, max(2, n // 12), size=(n, S)))
    bases = {(b * n) % 4 for b in range(S)}
    # an odd n puts the bins' bases at all four residues; n = 2 (mod 4) only at 0 and 2 (b * n is even): the groups' STARTS,
    # base + start, are what the kernel aligns down, and those are asserted at all four residues below
    assert bases == ({0, 1, 2, 3} if n % 2 else {0, 2} if n % 4 else {0})
    if n >= 3:
        for g in inp.lists.groups:
            assert ((g.length >= 2) & (g.length <= 40)).any()
    if n >= 31:
        assert {r for _, r in start_residues(inp.lists, n)} == {0, 1, 2, 3}
    return inp


# ---- group length and start: every length of the ladder at every residue of its first element ----
LADDER = (1, 2, 3, 4, 255, 256, 257, 260, 511, 513)
EDGE_VALUES = (0, 255, 256, 65279, 65280, 65535)     # first and last value of a thread's 256 in bin_scan_kernel
LADDER_N, LADDER_S = 1543, 8


def _lay_out(rng, n, segs):
    """One bin from its groups in ascending order of value: segs = [(length, value or None: the previous value + 1)];
    the members of every group are drawn from the whole id range."""
    col = np.empty(n, dtype=np.uint16)
    perm = rng.permutation(n)
    pos, prev = 0, -1
    for length, value in segs:
        value = prev + 1 if value is None else value
        assert prev < value <= 65535
        col[perm[pos:pos + length]] = value
        pos, prev = pos + length, value
    assert pos == n
    return col


@functools.lru_cache(maxsize=None)
def group_ladder():
    """The ten lengths sum to 2 062 > n = 1 543, so one bin cannot hold a whole ladder: the 40 (length, residue) combinations
    are packed into bins 0-6 (bin 0 also carries the edge values), bin 7 is unique per sample.  Lists stay below n <= LIST_CAP."""
    n, S = LADDER_N, LADDER_S
    rng = np.random.default_rng(n)
    skq = unique_bins(rng, n, S)
    ones = lambda k: [(1, None)] * k
    # bin 0: groups at the values where bin_scan_kernel's threads begin and end
    segs = [(2, 0)] + [(1, v) for v in range(1, 255)] + [(3, 255), (4, 256)]
    used = sum(l for l, _ in segs) + 255 + 256 + 254 + 513
    segs += ones(n - used) + [(255, 65279), (256, 65280)] + [(1, v) for v in range(65281, 65535)] + [(513, 65535)]
    skq[:, 0] = _lay_out(rng, n, segs)
    needed = {(L, r) for L in LADDER for r in range(4)} - start_residues(candidate_lists(skq[:, :1]), n, 1)
    for b in range(1, S - 1):
        segs, pos = [], 0
        for L, r in sorted(needed, reverse=True):
            pad = (r - (b * n + pos)) % 4
            if pos + pad + L <= n:
                segs += ones(pad) + [(L, None)]
                pos += pad + L
                needed.discard((L, r))
        skq[:, b] = _lay_out(rng, n, segs + ones(n - pos))
    assert not needed, needed
    inp = _finish(skq)
    found = start_residues(inp.lists, n, 1)
    assert all((L, r) in found for L in LADDER for r in range(4))
    g0 = inp.lists.groups[0]
    for v in EDGE_VALUES:
        assert g0.length[g0.value == v].tolist()[0] in LADDER[1:], v      # a ladder group of at least 2 holds this value
    assert inp.lists.groups[S - 1].length.max() == 1 and n % 4 == 3
    return inp


# ---- the last block of the last group ends in the +16 slack of the members array ----
@functools.lru_cache(maxsize=None)
def slack_tail():
    n, S = 1021, 3
    rng = np.random.default_rng(1021)
    skq = rng.integers(1, 1 + n // 6, size=(n, S))
    skq[rng.choice(n, 258, replace=False), S - 1] = 65535
    skq[rng.choice(n, 5, replace=False), 0] = 0
    inp = _finish(skq)
    last, first = inp.lists.groups[S - 1], inp.lists.groups[0]
    assert (n * S) % 4 == 3                                   # the block that holds the last element reaches past the array
    assert last.value[-1] == 65535 and last.length[-1] == 258
    assert (S - 1) * n + last.start[-1] + last.length[-1] - 1 == n * S - 1
    assert first.value[0] == 0 and first.start[0] == 0 and first.length[0] == 5
    return inp


# ---- bins per block of 192 and per trip of 16 ----
BIN_COUNTS = (1, 2, 3, 15, 16, 17, 191, 192, 193, 384, 385)


def special_bins(S):
    return sorted({S - 1} | {b for k in range(1, S // CG_BIN_BLOCK + 1) for b in (CG_BIN_BLOCK * k - 1, CG_BIN_BLOCK * k) if b < S})


@functools.lru_cache(maxsize=None)
def bin_blocks(S):
    """-> (Input, [(bin, row, candidate)]): row and candidate (ids below 16, in no other group) meet in that bin only."""
    n = 203
    rng = np.random.default_rng(2000 + S)
    skq = unique_bins(rng, n, S)
    for b in range(S):
        sizes = rng.integers(2, 5, size=int(rng.integers(2, 4)))
        members = rng.choice(np.arange(16, n), size=int(sizes.sum()), replace=False)
        for m in np.split(members, np.cumsum(sizes)[:-1]):
            skq[m, b] = skq[m[0], b]
    only = []
    for t, b in enumerate(special_bins(S)):
        skq[2 * t + 1, b] = skq[2 * t, b]
        only.append((b, 2 * t, 2 * t + 1))
    inp = _finish(skq)
    for g in inp.lists.groups:
        assert 2 <= (g.length >= 2).sum() <= 4
    for b, i, j in only:
        assert np.flatnonzero(inp.skq[i] == inp.skq[j]).tolist() == [b]
        assert row_list(inp.lists, i).tolist() == [j] and row_list(inp.lists, j).tolist() == [i]
    return inp, only


# ---- two blocks of bins with one wave far behind the others ----
@functools.lru_cache(maxsize=None)
def unbalanced_blocks():
    """cand_rows_kernel parks the bounds of 192 bins at a time and a wave takes the bins = its number (mod 4).  Row 0: a
    1 501-member group in each bin of wave 0's first three trips (bins 0, 4, .. 44: six loads per group, one after the
    other), then a partner of its own in each of wave 0's later bins of the first block (48, 52, .. 188) -- bounds that
    wave 0 reads long after the other three waves, whose bins hold nothing, are done with the block.  A second full block
    follows, so the parked bounds ARE replaced.  -> (Input, row 0's 36 partners)."""
    n, S = 2049, 2 * CG_BIN_BLOCK
    rng = np.random.default_rng(2049)
    skq = unique_bins(rng, n, S)
    crowd = np.concatenate([[0], 1 + rng.choice(n - 1, 1500, replace=False)])
    partners = np.setdiff1d(np.arange(1, n), crowd)[:36]
    for b in range(0, 48, 4):
        skq[crowd, b] = skq[0, b]
    for x, b in zip(partners, range(48, CG_BIN_BLOCK, 4)):
        skq[x, b] = skq[0, b]
    inp = _finish(skq)
    assert partners.size == 36 and list_lengths(inp.lists)[0] == 1500 + 36 and S > CG_BIN_BLOCK
    for x in partners:
        assert row_list(inp.lists, x).tolist() == [0]
    return inp, partners


# ---- several bitmap words per thread in step C ----
WORDS_N = {16421: 3, 8193: 2}     # n -> words per thread


@functools.lru_cache(maxsize=None)
def bitmap_words(n):
    S = 4
    rng = np.random.default_rng(n)
    skq = np.empty((n, S), dtype=np.uint16)
    for b in range(S):
        perm = rng.permutation(n)
        sizes = []
        if b == 0:      # one list with bit 31 of word 5 and bit 0 of word 6
            trio = np.array([7, 191, 192])
            perm = np.concatenate([trio, perm[~np.isin(perm, trio)]])
            sizes.append(3)
        while sum(sizes) < n:
            left = n - sum(sizes)
            L = int(rng.integers(2, 31))
            sizes.append(left if left - L < 2 else L)
        for x, m in enumerate(np.split(perm, np.cumsum(sizes)[:-1])):
            skq[m, b] = x * (65535 // len(sizes))
    inp = _finish(skq)
    n_words, per = words_per_thread(n)
    assert per == WORDS_N[n]
    assert (CG_THREADS - 1) * per > n_words                   # trailing threads whose range starts past the bitmap
    lens = list_lengths(inp.lists)
    assert lens.min() >= 1 and lens.max() > 30
    threads = lambda i: np.unique((row_list(inp.lists, i) >> 5) // per)
    assert any(threads(i).size >= 3 for i in range(64))
    in_last_word = inp.lists.cols[(inp.lists.cols >> 5) == n_words - 1]
    assert in_last_word.size and (in_last_word == n - 1).any()
    assert {191, 192} <= set(row_list(inp.lists, 7).tolist())
    if n == 8193:
        assert (n - 1) % 32 == 0                              # the last word holds one bit
    return inp


# ---- empty and full ----
@functools.lru_cache(maxsize=None)
def ragged_small():
    n, S = 131, 5
    rng = np.random.default_rng(131)
    skq = rng.integers(0, 20, size=(n, S))
    skq[5] = 60000 + np.arange(S)
    inp = _finish(skq)
    lens = list_lengths(inp.lists)
    assert lens[5] == 0 and lens[0] > 0 and lens[n - 1] > 0
    assert row_list(inp.lists, 0).min() > 0 and row_list(inp.lists, n - 1).max() < n - 1
    return inp


@functools.lru_cache(maxsize=None)
def everybody(n=130, S=3, bin_=1):
    rng = np.random.default_rng(n)
    skq = unique_bins(rng, n, S)
    skq[:, bin_] = 4242
    inp = _finish(skq, cap=n - 1)
    assert (list_lengths(inp.lists) == n - 1).all()
    return inp


# ---- symmetric work items: a row's items start at its first candidate with a larger id ----
def work_items(lists, i):
    """(candidates below i, 64-candidate work items of row i's upper half)."""
    row = row_list(lists, i)
    below = int(np.searchsorted(row, i))
    return below, (row.size - below + 63) // 64


@functools.lru_cache(maxsize=None)
def symmetric_items():
    """-> (Input, {work items: a row with that many whose upper half does not start at a multiple of 64 within its list})."""
    n, S = 700, 4
    rng = np.random.default_rng(700)
    skq = unique_bins(rng, n, S)
    skq[:, 0] = np.arange(n) % 3
    skq[:, 1] = rng.integers(0, 70, size=n)
    inp = _finish(skq)
    rows = {}
    for i in range(n):
        below, items = work_items(inp.lists, i)
        if below % 64:
            rows.setdefault(items, i)
    assert {1, 2, 3, 4} <= set(rows)          # 2: more than 64 above the row, 3 and 4: more than 128
    assert work_items(inp.lists, n - 1)[1] == 0 and work_items(inp.lists, 0)[0] == 0
    return inp, rows


# ---- the branches of knn_from_device_csr beyond the cap (deliberately) ----
@functools.lru_cache(maxsize=None)
def two_halves():
    n = 2801
    inp = _finish((np.arange(n) % 2).reshape(n, 1), cap=n)
    assert sorted(set(list_lengths(inp.lists).tolist())) == [1399, 1400]
    return inp


def copy_back_batches(n, knn):
    """select_and_copy_back: four row batches from 32 MiB of results (u64 id + f32 distance per entry)."""
    return 4 if n * knn * 12 >= (32 << 20) else 1


# ---- the limit: an n-bit bitmap in 158 KB of LDS ----
def limit_skq(n):
    """One bin, skq[i] = (i // 2) mod 65 536.  (i // 2 itself does not fit a u16 beyond n = 131 072: no index sketch gives
    lists of one at the limit -- 1.29 M samples over 65 536 values leave ~20 per group.)"""
    return ((np.arange(n) // 2) % 65536).astype(np.uint16).reshape(n, 1)


def limit_lists(n):
    """The lists of limit_skq(n) from arithmetic: ids [n, width] i32 ascending per row, -1 behind the end."""
    i = np.arange(n, dtype=np.int64)
    q = i // 2
    mult = -(-((n + 1) // 2) // 65536)
    qq = (q % 65536)[:, None] + 65536 * np.arange(mult)[None, :]
    j = np.stack([2 * qq, 2 * qq + 1], axis=2).reshape(n, 2 * mult)
    j[(j >= n) | (j == i[:, None])] = np.iinfo(np.int64).max
    j.sort(axis=1)
    j[j == np.iinfo(np.int64).max] = -1
    width = int((j >= 0).sum(axis=1).max(initial=0))
    return j[:, :max(width, 1)].astype(np.int32)


def limit_expected(n, dist3, knn, ids=None):
    """Canonical kNN (ascending distance, then id) of limit_skq(n) over a slab tiled from three sketches, bins[i] =
    pattern[i % 3]; dist3 = their 3 x 3 distances (f32).  -> (idx u64 [n, knn], d0 f32 [n, knn], total), padding (i, 1.0)."""
    ids = limit_lists(n) if ids is None else ids
    i = np.arange(n)
    valid = ids >= 0
    keys = np.where(valid, np.asarray(dist3, dtype=np.float32)[(i % 3)[:, None], ids % 3], np.float32(np.inf)).astype(np.float32)
    order = np.argsort(keys, axis=1, kind="stable")[:, :knn]          # (ids ascend within a row: stable = ties by id)
    idx = np.take_along_axis(ids, order, axis=1).astype(np.int64)
    d0 = np.take_along_axis(keys, order, axis=1)
    pad = idx < 0
    idx[pad] = np.broadcast_to(i[:, None], idx.shape)[pad]
    d0[pad] = 1.0
    if idx.shape[1] < knn:
        extra = knn - idx.shape[1]
        idx = np.concatenate([idx, np.repeat(i[:, None], extra, axis=1)], axis=1)
        d0 = np.concatenate([d0, np.ones((n, extra), dtype=np.float32)], axis=1)
    return idx.astype(np.uint64), d0.astype(np.float32), int(valid.sum())
