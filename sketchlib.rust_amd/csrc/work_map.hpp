// work_map.hpp -- WHICH WORKGROUP COMPUTES WHAT in the pair kernels, forward (the host's plan: how many tiles, units and
// workgroups a launch has) and inverse (the kernels' decode of their workgroup index), as plain functions of the launch's
// fields: the ONE place the numbering is written.
//
//   tiles   workgroup index -> (XCD, slot) -> tile number -> (column group, row tile): plan_tile_geometry() and
//           plan_tile_numbering() against lookup_tile_at();
//   units   the chunk-split kernel's k-sliced grid, slot on an XCD -> (tile slot, k index, chunk slice) and the slice's chunk
//           range: plan_kslice_grid() against kslice_unit() and slice_chunk_range().
//
// Every function is a template over the argument struct and reads or writes the PairArgs fields of those names (kernels.h), so
// that tests/native/work_map_check.cpp can hand it a plain struct: nothing here touches a device or needs a device header.
// Under hipcc the functions are host + device and forced inline, under a host compiler plain inline.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define SKL_MAP_FN __host__ __device__ __forceinline__
#define SKL_MAP_UNROLL _Pragma("unroll")
#else
#define SKL_MAP_FN inline
#define SKL_MAP_UNROLL
#endif

namespace skl {

constexpr int TILE_PREFIX_INLINE = 16;     // entries of the super-group prefix table that ride in the kernel arguments
constexpr uint32_t XCD_DEAL_SHIFT = 5;     // xcd_interleave: the XCDs take the tile numbering in turns, 32 tiles at a time
constexpr uint32_t KSL_TILE_BLOCK = 32;    // k-sliced launches: tiles that walk a k-mer length together

SKL_MAP_FN uint32_t map_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// ---------------------------------------------------------------------------
// tiles
// ---------------------------------------------------------------------------

// Row tiles column group `group` needs in self mode: those with some i < j, i.e. first row below the group's last column.
template <class G>
SKL_MAP_FN uint32_t group_row_tiles(const G &g, uint32_t group)
{
    const uint64_t last_col = (uint64_t)(group + 1u) * g.group_cols - 1u;
    const uint32_t lim = last_col < g.row_end ? (uint32_t)last_col : g.row_end;
    return lim > g.row_begin ? (lim - g.row_begin + g.tile_rows - 1u) / g.tile_rows : 0u;
}

// A super-group is group_span consecutive column groups; the self-mode prefix table has one entry per super-group and one more.
template <class G>
SKL_MAP_FN uint32_t n_supergroups(const G &g)
{
    return (g.n_groups + g.group_span - 1u) / g.group_span;
}

// Forward, step 1: the tile grid of a launch of rows_per_tile x cols_per_group tiles over rows [row_begin, row_end) x nB columns.
template <class G>
SKL_MAP_FN void plan_tile_geometry(G &g, uint32_t rows_per_tile, uint32_t cols_per_group)
{
    if (g.group_span == 0) g.group_span = 1;
    g.tile_rows = rows_per_tile;
    g.group_cols = cols_per_group;
    g.a_tiles = (g.row_end - g.row_begin + rows_per_tile - 1) / rows_per_tile;
    g.n_jblocks = (g.nB + 63u) / 64u;
    g.n_groups = (g.nB + cols_per_group - 1) / cols_per_group;
    g.tile_prefix = nullptr;
    g.n_prefix_inline = 0;
}

// Forward, step 2: the numbering of the ACTIVE tiles, super-group by super-group, and its split over the XCDs.  Self mode fills
// prefix[0 .. n_supergroups(g)] with the first tile number of each super-group (the caller uploads it and sets g.tile_prefix)
// and copies it into the arguments when it is short enough and the launch allows it.  Workgroup b runs on XCD
// b mod 2^xcd_shift and is slot b >> xcd_shift there; XCD x takes tiles [x * tiles_per_xcd, (x + 1) * tiles_per_xcd) of the
// numbering -- every XCD the same number of (equal-cost) tiles -- or, interleaved, whole blocks of 32 tiles dealt in turns.
// Returns false when the launch has too many tiles; *grid_out = tiles_per_xcd << xcd_shift workgroups, 0 = nothing to do.
template <class G>
SKL_MAP_FN bool plan_tile_numbering(G &g, uint32_t *prefix, uint64_t *grid_out)
{
    *grid_out = 0;
    g.n_active_tiles = g.tiles_per_xcd = 0;
    uint64_t total = (uint64_t)g.a_tiles * g.n_groups;
    if (g.self_mode) {
        const uint32_t n_super = n_supergroups(g);
        total = 0;
        for (uint32_t gi = 0; gi < g.n_groups; ++gi) {
            if (gi % g.group_span == 0) prefix[gi / g.group_span] = (uint32_t)total;
            total += group_row_tiles(g, gi);
        }
        prefix[n_super] = (uint32_t)total;
        if (g.inline_prefix_ok && n_super + 1u <= (uint32_t)TILE_PREFIX_INLINE) {
            g.n_prefix_inline = n_super + 1u;
            for (uint32_t x = 0; x <= n_super; ++x) g.tile_prefix_inline[x] = prefix[x];
        }
    }
    if (total >= (1ull << 31)) return false;
    const uint64_t n_xcd = 1ull << g.xcd_shift;
    g.n_active_tiles = (uint32_t)total;
    g.tiles_per_xcd = (uint32_t)((total + n_xcd - 1) >> g.xcd_shift);
    if (g.xcd_interleave) {
        const uint64_t blocks = (total + (1u << XCD_DEAL_SHIFT) - 1) >> XCD_DEAL_SHIFT;
        g.tiles_per_xcd = (uint32_t)(((blocks + n_xcd - 1) >> g.xcd_shift) << XCD_DEAL_SHIFT);
    }
    *grid_out = (uint64_t)g.tiles_per_xcd << g.xcd_shift;
    return true;
}

// Inverse.  Tile u of super-group sg, self mode: its tiles are numbered row tile by row tile, the groups that need that row
// tile side by side.  Later groups need more row tiles (the triangle), so row tile `at` belongs to the LAST groups of the
// super-group: all of them up to the first group's count, one fewer up to the second's, ...
template <class G>
SKL_MAP_FN void tile_in_supergroup_self(const G &g, uint32_t sg, uint32_t u, uint32_t &group, uint32_t &row_tile)
{
    const uint32_t first = sg * g.group_span;
    const uint32_t gcount = map_min(g.group_span, g.n_groups - first);
    uint32_t lo_at = 0;
    for (uint32_t gi = 0; gi + 1u < gcount; ++gi) {
        const uint32_t width = gcount - gi;
        const uint32_t n_gi = group_row_tiles(g, first + gi);
        const uint32_t span = (n_gi - lo_at) * width;
        if (u < span) {
            row_tile = lo_at + u / width;
            group = first + gi + (u - (u / width) * width);
            return;
        }
        u -= span;
        lo_at = n_gi;
    }
    row_tile = lo_at + u;
    group = first + gcount - 1u;
}

// ... cross mode: every group needs all a_tiles row tiles
template <class G>
SKL_MAP_FN void tile_in_supergroup_cross(const G &g, uint32_t t, uint32_t &group, uint32_t &row_tile)
{
    const uint32_t per = g.group_span * g.a_tiles;
    const uint32_t sg = t / per, u = t - sg * per;
    const uint32_t first = sg * g.group_span;
    const uint32_t gcount = map_min(g.group_span, g.n_groups - first);
    row_tile = u / gcount;
    group = first + (u - row_tile * gcount);
}

// Slot `slot` of XCD `xcd` -> its tile; false when that workgroup has none.  The ~100 workgroups resident on an XCD are
// consecutive tiles = row tiles x group_span column groups, each row tile shared by group_span neighbouring workgroups.  HBM
// bytes per launch at n = 16 000 with 32 x 128 tiles: 44.8 GB numbered group by group, 31.6 GB with group_span = 2 (the
// default), 32.0 GB with 4; at cfg 2 (k-sliced, 16 x 128): 261 / 257 / 321 MB (profiles/r02_tile32_*.md, r02c_*).
template <class G>
SKL_MAP_FN bool lookup_tile_at(const G &g, uint32_t xcd, uint32_t slot, uint32_t &group, uint32_t &row_tile)
{
    if (slot >= g.tiles_per_xcd) return false;
    const uint32_t t = g.xcd_interleave ? ((((slot >> XCD_DEAL_SHIFT) << g.xcd_shift) + xcd) << XCD_DEAL_SHIFT) + (slot & ((1u << XCD_DEAL_SHIFT) - 1u))
                                        : xcd * g.tiles_per_xcd + slot;
    if (t >= g.n_active_tiles) return false;
    if (!g.self_mode) {
        tile_in_supergroup_cross(g, t, group, row_tile);
        return true;
    }
    const uint32_t n_super = n_supergroups(g);
    if (g.n_prefix_inline != 0u) {   // the table rides in the kernel arguments: no global load before the first row DMA
        uint32_t lo = 0, base = 0;
        SKL_MAP_UNROLL
        for (int x = 1; x < TILE_PREFIX_INLINE; ++x) {
            if ((uint32_t)x < n_super && g.tile_prefix_inline[x] <= t) {
                lo = (uint32_t)x;
                base = g.tile_prefix_inline[x];
            }
        }
        tile_in_supergroup_self(g, lo, t - base, group, row_tile);
        return true;
    }
    uint32_t lo = 0, hi = n_super;  // largest lo with prefix[lo] <= t
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (g.tile_prefix[mid] <= t) lo = mid; else hi = mid;
    }
    tile_in_supergroup_self(g, lo, t - g.tile_prefix[lo], group, row_tile);
    return true;
}

// ---------------------------------------------------------------------------
// units of the chunk-split kernel (pair_kslice.hip)
// ---------------------------------------------------------------------------
//
// k-sliced (one workgroup per (tile, k-mer length)): blocks of KSL_TILE_BLOCK consecutive tiles of an XCD walk one k-mer length
// together (tile index fastest, then k, then block), so that the workgroups resident on an XCD at one time share a (column
// group, k) plane of the lane slab in its L2: 2 % at n = 4 000 ... 8 000 against k fastest
// (profiles/r02_ab_korder_l2prefetch.jsonl).  The last block of an XCD may be short: the grid has exactly tiles_per_xcd x k x
// slices workgroups per XCD, no padding slots that would be dispatched only to exit.
// MODE_COUNTS launches (`counts`) may also cut a k-mer length into k_slices chunk ranges, one workgroup each -- more, shorter
// workgroups for launches that would otherwise fill the chip 1.4 times; slice s of k index kk stores its counts as "k index"
// s * k_count + kk, summed by the epilogue.
// TAIL SLICING (tail_slices > 1, instead of the uniform slices): the workgroups of an XCD up to index tail_first -- its whole
// rounds of tail_resident resident workgroups -- are whole units, the ones after are chunk slices of the remaining units.  The
// last round of a launch is then made of short workgroups that spread over all SIMDs instead of a few long ones that run 1-2
// per SIMD at a lone wave's issue interval, and the rounds before it pay nothing.  Slice 0 stores, the others add into plane 1
// (kernels.h).

// Forward: normalises k_slices / tail_slices / slice_chunks / round_size of a launch whose tiles are planned, sets tail_first
// and counts the workgroups.  False = a request the kernel cannot serve (the launcher's hipErrorInvalidValue).
template <class G>
SKL_MAP_FN bool plan_kslice_grid(G &g, bool k_sliced, bool counts, uint64_t *n_wg)
{
    const uint64_t units = (uint64_t)g.tiles_per_xcd * (k_sliced ? g.k_count : 1u);   // per XCD
    if (!(k_sliced && counts) || g.k_slices == 0) g.k_slices = 1;
    if (!(k_sliced && counts)) g.tail_slices = 0;
    if (g.tail_slices > 1u) {
        if (g.tail_resident == 0) return false;
        g.k_slices = 1;
    }
    const uint32_t S = g.tail_slices > 1u ? g.tail_slices : g.k_slices;
    if (S <= 1u) {
        g.slice_chunks = 0;
    } else if (g.slice_chunks == 0u) {   // whole stages (8 chunks) per slice, every slice holds something
        if (g.ss64 % (S * 8u) != 0) return false;
    } else if (g.slice_chunks % 8u != 0 || (uint64_t)g.slice_chunks * (S - 1u) >= g.ss64 || (uint64_t)g.slice_chunks * S < g.ss64) {
        return false;
    }
    // wave priority by round: for launches of up to 2.25 rounds of workgroups (it costs 2 % at 2.5-2.7 rounds and is neutral
    // beyond; profiles/r02_ab_round_priority.jsonl)
    if (!k_sliced || units * g.k_slices * 4u > 9ull * g.round_size) g.round_size = 0;
    *n_wg = (units * g.k_slices) << g.xcd_shift;
    if (g.tail_slices > 1u) {
        const uint64_t first = units / g.tail_resident * g.tail_resident;
        *n_wg = (first + (units - first) * g.tail_slices) << g.xcd_shift;
        g.tail_first = (uint32_t)first;
    }
    return *n_wg < (1ull << 31);
}

// Inverse: what workgroup s_idx of an XCD computes.  ksl / counts: the kernel's form (compile-time there).
//   none      no unit: a slot past the XCD's last tile block (the planned grid has none)
//   tail_mode a tail-sliced launch; in_tail: this workgroup is one of its slices
//   slot      tile slot on the XCD (lookup_tile_at); kk0: first k index of the workgroup (k-sliced: its only one)
//   slice     of n_slices chunk slices (whole unit: 0 of 1)
struct KsliceUnit {
    bool none, tail_mode, in_tail;
    uint32_t slot, kk0, slice, n_slices;
};
template <class G>
SKL_MAP_FN KsliceUnit kslice_unit(const G &g, uint32_t s_idx, bool ksl, bool counts)
{
    constexpr uint32_t KB = KSL_TILE_BLOCK;
    KsliceUnit u = {false, false, false, s_idx, 0u, 0u, 1u};
    u.tail_mode = ksl && counts && g.tail_slices > 1u;
    u.in_tail = u.tail_mode && s_idx >= g.tail_first;
    u.n_slices = u.in_tail ? g.tail_slices : (ksl && counts && !u.tail_mode ? g.k_slices : 1u);
    if (!ksl) return u;
    const uint32_t u_idx = u.in_tail ? g.tail_first + (s_idx - g.tail_first) / u.n_slices : s_idx;   // unit index (tail mode) / workgroup index
    const uint32_t per_blk = KB * g.k_count * (u.tail_mode ? 1u : u.n_slices);
    const uint32_t blk_ = u_idx / per_blk, rem_ = u_idx - blk_ * per_blk;
    const uint32_t in_blk = map_min(KB, g.tiles_per_xcd - map_min(g.tiles_per_xcd, blk_ * KB));
    // (no early return for `none`, a divisor that is never 0 instead: with one, the fused-epilogue forms of the A/B build
    // spilled 4 registers they do not spill with the decode written out in the kernel)
    u.none = in_blk == 0u;
    const uint32_t tiles = in_blk | (uint32_t)u.none;
    u.slot = blk_ * KB + rem_ % tiles;
    const uint32_t kslot = rem_ / tiles;
    u.kk0 = u.tail_mode ? kslot : kslot / u.n_slices;
    u.slice = u.in_tail ? (s_idx - g.tail_first) % u.n_slices : (u.tail_mode ? 0u : kslot - u.kk0 * u.n_slices);
    return u;
}

// Chunk range of slice `slice` of n_slices: whole stages per slice, the last slice takes what is left (any sketch size)
template <class G>
SKL_MAP_FN void slice_chunk_range(const G &g, uint32_t n_slices, uint32_t slice, uint32_t &c_begin, uint32_t &c_end)
{
    const uint32_t per_slice = g.slice_chunks != 0u ? g.slice_chunks : g.ss64 / n_slices;
    c_begin = n_slices > 1u ? map_min(g.ss64, slice * per_slice) : 0u;
    c_end = n_slices > 1u ? map_min(g.ss64, c_begin + per_slice) : g.ss64;
}

}  // namespace skl
