// pair_prune.hpp -- tile pruning of the symmetric self kNN in pair_kernel_kslice (pair_kslice.hip, PRUNE): the words the
// workgroup keeps for it and the test every vote runs.  What happens to a tile BEFORE its walk -- the plane-pair probe and,
// for a tile that survives it for a few rows only, the sparse walk and its finish -- is pair_kslice_probe.inc; the checks
// at the walk's stage boundaries are in pair_kslice_walk.inc.
//
// q = floor(allow / 4) + 1 per sample (PairArgs::prune_q_*), allow = the largest mismatch count whose key is still below
// that sample's knn-th best.  All 4 waves compute the same plan from the same bounds (they meet at a barrier per check).  A
// tile with one sample whose list is not full (q beyond any count) is neither probed nor checked: no cost outside the
// regime pruning is for.
#pragma once

#include "pair_finish.hpp"

namespace skl {

// The workgroup's pruning words behind its row buffers: [0, 128) the bounds of the tile's columns (the same values written by
// every wave), [128, 136) two rotating rows of 4 votes (one barrier per check), [136, 136 + R) the bounds of its rows, then
// the probe's own 4 row masks and 4 block masks.
constexpr uint32_t PRUNE_VOTES = 2u * LANES, PRUNE_ROW_BOUNDS = PRUNE_VOTES + 8u;
__host__ __device__ constexpr uint32_t prune_lds_words(int rows) { return PRUNE_ROW_BOUNDS + (uint32_t)rows + 8u; }

// Which lanes' pairs of one row are still alive?  `packed` = this lane's counts so far against the row
// (column block 0 in the low u16 field, block 1 in the high one), q_* = the per-wave bounds of the row and of the lane's two
// columns (a pair is hopeless once its count reaches the larger of its two), col*_ok = the column exists.
struct AliveBallots {
    uint64_t blk0, blk1;
};
__device__ __forceinline__ AliveBallots alive_pairs(uint32_t packed, uint32_t q_row, uint32_t q_col0, uint32_t q_col1, bool col0_ok, bool col1_ok)
{
    return {__ballot(col0_ok && (packed & 0xFFFFu) < max(q_row, q_col0)), __ballot(col1_ok && (packed >> 16) < max(q_row, q_col1))};
}

}  // namespace skl
