"""Reference for the candidate lists of `inverted precluster` (Inverted::any_shared_bins for every sample): sample j is a
candidate of sample i iff their index sketches hold the same u16 value at some bin position.

Not the device's algorithm (histogram, scan, scatter, an n-bit bitmap per row) and not the O(n^2 * S) definition that
tests/test_gpu_precluster.py::candidates spells out: every bin is grouped by value with a stable argsort, the groups' member
pairs are written out, and the union over the bins is one np.unique.  Beside the lists it returns each bin's groups as the
device's counting sort lays them out, so that a test can assert -- from the data, before the device is asked -- that the edge it
names (a group of 257 members that starts at residue 3 of the members array, ...) is present in its input."""
from collections import namedtuple

import numpy as np

Groups = namedtuple("Groups", "order value start length")
"""One bin: `order` = the samples in the counting sort's order of VALUES (ascending value; within a value the device's order is
whatever its atomics gave, here ascending id), and per group its value, its start (= the number of samples with a smaller
value in the bin: the group occupies members[bin * n + start : bin * n + start + length]) and its length."""

Lists = namedtuple("Lists", "offs cols groups")


def bin_groups(col):
    col = np.ascontiguousarray(col, dtype=np.uint16)
    order = np.argsort(col, kind="stable")
    sv = col[order]
    start = np.flatnonzero(np.r_[True, sv[1:] != sv[:-1]]) if col.size else np.zeros(0, dtype=np.int64)
    length = np.diff(np.r_[start, col.size])
    return Groups(order, sv[start], start.astype(np.int64), length.astype(np.int64))


def candidate_lists(skq):
    """skq [n, S] u16 -> Lists(offs u64 [n + 1], cols u32 ascending per row with the row itself removed, groups [S])."""
    skq = np.ascontiguousarray(skq, dtype=np.uint16)
    assert skq.ndim == 2
    n, S = skq.shape
    groups = [bin_groups(skq[:, b]) for b in range(S)]
    codes = []
    for g in groups:
        for L in np.unique(g.length[g.length > 1]):
            first = g.start[g.length == L]
            members = g.order[first[:, None] + np.arange(L)[None, :]].astype(np.uint64)       # [groups of L members, L]
            pair = members[:, :, None] * np.uint64(n) + members[:, None, :]                   # row * n + candidate
            codes.append(pair[:, ~np.eye(int(L), dtype=bool)].reshape(-1))
    code = np.unique(np.concatenate(codes)) if codes else np.zeros(0, dtype=np.uint64)
    rows = (code // np.uint64(max(n, 1))).astype(np.int64)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return Lists(offs, (code % np.uint64(max(n, 1))).astype(np.uint32), groups)


def row_list(lists, i):
    return lists.cols[int(lists.offs[i]):int(lists.offs[i + 1])]


def list_lengths(lists):
    return np.diff(lists.offs.astype(np.int64))


def start_residues(lists, n, min_length=2):
    """{(length, (bin * n + start) % 4)} over every group of at least min_length members: the alignment of the group's
    first element in the device's members array (cand_rows_kernel reads it in aligned 16-byte blocks)."""
    found = set()
    for b, g in enumerate(lists.groups):
        keep = g.length >= min_length
        found |= set(zip(g.length[keep].tolist(), ((b * n + g.start[keep]) % 4).tolist()))
    return found
