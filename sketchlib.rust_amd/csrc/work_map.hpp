// work_map.hpp -- WHICH WORKGROUP COMPUTES WHAT in the pair kernels, forward (the host's plan: how many tiles, units and
// workgroups a launch has) and inverse (the kernels' decode of their workgroup index), as plain functions of the launch's
// fields: the ONE place the numbering is written.
//
//   tiles   workgroup index -> (XCD, slot) -> tile number -> (column group, row tile): plan_tile_geometry() and
//           plan_tile_numbering() against lookup_tile_at(); dealt by cost (self mode, full tiles before half tiles on every
//           XCD): plan_tile_numbering_by_cost() against lookup_tile_by_cost_at(), tile_slot_by_cost() the forward map;
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
// numbering -- every XCD the same number of tiles, which are equal-cost in cross mode and wherever no half tile is walked; self-mode
// launches that walk half tiles are dealt by cost instead (plan_tile_numbering_by_cost below) -- or, interleaved, whole blocks of
// 32 tiles dealt in turns.
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
// tiles dealt by cost (self mode, 128-column groups: tile_cost_order)
// ---------------------------------------------------------------------------
//
// In self mode the active tiles are NOT equal-cost where the kernel walks half tiles (pair_kslice.hip): a tile whose 64-column
// block 0 lies on or below the diagonal, or whose block 1 lies past the launch's last column, walks one block and costs half.
// Every column group ends in 64 / tile_rows such tiles, so contiguous shares of the numbering above differ by up to a ninth in
// cost at 1 000 genomes, and the XCD that holds none of them ends last.  The second order numbers the two classes apart:
//   full tiles   the super-group numbering above with every group's row tiles cut at its last full one (same prefix table);
//   half tiles   group by group: the first group the band reaches, a run of groups with 64 / tile_rows each, the last group
//                the band's end cuts, and the group whose columns end in block 0 (all of its tiles) -- closed form, no table.
// XCD x takes the x-th share of the full numbering, then the x-th share of the half numbering: its slots run its full tiles
// first and its half tiles last.  Shares differ by at most one tile per class -- the odd full tiles go to the first XCDs,
// the odd half tiles to the last -- so the heaviest XCD is within one full tile of the mean.  tiles_per_xcd is the largest
// share; a slot past an XCD's own share yields nothing.

// The half-tile tests of a tile whose first row is a0 and first 64-column block jb0 (2 blocks per tile): the kernel's skip and
// the classes below are the same two lines.
SKL_MAP_FN bool tile_skips_block0(uint32_t self_mode, uint32_t a0, uint32_t jb0) { return self_mode && a0 + 1u >= (jb0 + 1u) * 64u; }
SKL_MAP_FN bool tile_skips_block1(uint32_t jb0, uint32_t n_jblocks) { return jb0 + 1u >= n_jblocks; }

// The launches the order is defined for
template <class G>
SKL_MAP_FN bool tile_cost_order_possible(const G &g)
{
    return g.self_mode && !g.xcd_interleave && g.group_cols == 128u && g.tile_rows != 0u && 64u % g.tile_rows == 0u;
}

// Column groups that can hold a full tile: all but a last group whose columns end in block 0
template <class G>
SKL_MAP_FN uint32_t n_full_groups(const G &g)
{
    return g.n_groups - (g.n_groups != 0u && tile_skips_block1((g.n_groups - 1u) * 2u, g.n_jblocks) ? 1u : 0u);
}

// Full row tiles of column group `group`: the first ones, those whose first row lies before the group's column 63
template <class G>
SKL_MAP_FN uint32_t group_full_row_tiles(const G &g, uint32_t group)
{
    if (tile_skips_block1(group * 2u, g.n_jblocks)) return 0u;
    const uint64_t mid = (uint64_t)group * g.group_cols + 63u;
    const uint32_t lim = mid < g.row_end ? (uint32_t)mid : g.row_end;
    return lim > g.row_begin ? (lim - g.row_begin + g.tile_rows - 1u) / g.tile_rows : 0u;
}

// Tile u of super-group sg of the full numbering: tile_in_supergroup_self() with the groups' limits pulled in
template <class G>
SKL_MAP_FN void full_tile_in_supergroup(const G &g, uint32_t sg, uint32_t u, uint32_t &group, uint32_t &row_tile)
{
    const uint32_t first = sg * g.group_span;
    const uint32_t gcount = map_min(g.group_span, n_full_groups(g) - first);
    uint32_t lo_at = 0;
    for (uint32_t gi = 0; gi + 1u < gcount; ++gi) {
        const uint32_t width = gcount - gi;
        const uint32_t n_gi = group_full_row_tiles(g, first + gi);
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

// The runs of the half numbering: group ga (h_a tiles), groups ga + 1 ... ga + n_mid (`per` each), group gb (h_b), group
// n_groups - 1 when its columns end in block 0 (whatever is left).  A group below ga has no tile, one above gb only full ones.
struct HalfRuns {
    uint32_t ga, h_a, n_mid, per, gb, h_b;
};
template <class G>
SKL_MAP_FN HalfRuns half_tile_runs(const G &g)
{
    HalfRuns r = {0u, 0u, 0u, 64u / g.tile_rows, 0u, 0u};
    const uint32_t ngf = n_full_groups(g);
    r.ga = (g.row_begin + 1u) / g.group_cols;    // the first group with a column right of row_begin
    if (ngf == 0u || g.row_end < 64u || r.ga >= ngf) return r;
    r.gb = map_min(ngf - 1u, (g.row_end - 64u) / g.group_cols);   // the last group whose column 63 lies right of a row
    if (r.gb < r.ga) return r;
    r.h_a = group_row_tiles(g, r.ga) - group_full_row_tiles(g, r.ga);
    if (r.gb > r.ga) {
        r.n_mid = r.gb - r.ga - 1u;
        r.h_b = group_row_tiles(g, r.gb) - group_full_row_tiles(g, r.gb);
    }
    return r;
}

// Inverse: half tile v
template <class G>
SKL_MAP_FN void half_tile_at(const G &g, uint32_t v, uint32_t &group, uint32_t &row_tile)
{
    const HalfRuns r = half_tile_runs(g);
    const uint32_t mid = r.n_mid * r.per;
    if (v < r.h_a) {
        group = r.ga;
    } else if (v - r.h_a < mid) {
        const uint32_t q = (v - r.h_a) / r.per;
        group = r.ga + 1u + q;
        v = v - r.h_a - q * r.per;
    } else if (v - r.h_a - mid < r.h_b) {
        group = r.gb;
        v = v - r.h_a - mid;
    } else {
        group = g.n_groups - 1u;
        v = v - r.h_a - mid - r.h_b;
    }
    row_tile = group_full_row_tiles(g, group) + v;
}

// The share of XCD `xcd`: tiles [full_begin, + n_full) of the full numbering, then [half_begin, + n_half) of the half numbering
struct CostShare {
    uint32_t full_begin, n_full, half_begin, n_half;
};
template <class G>
SKL_MAP_FN CostShare tile_cost_share(const G &g, uint32_t xcd)
{
    const uint32_t n_xcd = 1u << g.xcd_shift, n_half = g.n_active_tiles - g.n_full_tiles;
    const uint32_t qf = g.n_full_tiles >> g.xcd_shift, rf = g.n_full_tiles & (n_xcd - 1u);
    const uint32_t qh = n_half >> g.xcd_shift, plain = n_xcd - (n_half & (n_xcd - 1u));   // XCDs before those with one half tile more
    CostShare s;
    s.full_begin = xcd * qf + map_min(xcd, rf);
    s.n_full = qf + (xcd < rf ? 1u : 0u);
    s.half_begin = xcd * qh + (xcd > plain ? xcd - plain : 0u);
    s.n_half = qh + (xcd >= plain ? 1u : 0u);
    return s;
}

// Forward, step 2 in this order (tile_cost_order_possible() launches): as plan_tile_numbering(), the table being the full
// numbering's; sets n_full_tiles too.
template <class G>
SKL_MAP_FN bool plan_tile_numbering_by_cost(G &g, uint32_t *prefix, uint64_t *grid_out)
{
    *grid_out = 0;
    g.n_active_tiles = g.tiles_per_xcd = g.n_full_tiles = 0;
    g.n_prefix_inline = 0;
    const uint32_t ngf = n_full_groups(g), n_super = (ngf + g.group_span - 1u) / g.group_span;
    uint64_t total = 0, full = 0;
    for (uint32_t gi = 0; gi < g.n_groups; ++gi) total += group_row_tiles(g, gi);
    for (uint32_t gi = 0; gi < ngf; ++gi) {
        if (gi % g.group_span == 0) prefix[gi / g.group_span] = (uint32_t)full;
        full += group_full_row_tiles(g, gi);
    }
    prefix[n_super] = (uint32_t)full;
    if (total >= (1ull << 31)) return false;
    if (g.inline_prefix_ok && n_super + 1u <= (uint32_t)TILE_PREFIX_INLINE) {
        g.n_prefix_inline = n_super + 1u;
        for (uint32_t x = 0; x <= n_super; ++x) g.tile_prefix_inline[x] = prefix[x];
    }
    g.n_active_tiles = (uint32_t)total;
    g.n_full_tiles = (uint32_t)full;
    for (uint32_t x = 0; x < (1u << g.xcd_shift); ++x) {
        const CostShare s = tile_cost_share(g, x);
        if (s.n_full + s.n_half > g.tiles_per_xcd) g.tiles_per_xcd = s.n_full + s.n_half;
    }
    *grid_out = (uint64_t)g.tiles_per_xcd << g.xcd_shift;
    return true;
}

// Inverse in this order: lookup_tile_at()
template <class G>
SKL_MAP_FN bool lookup_tile_by_cost_at(const G &g, uint32_t xcd, uint32_t slot, uint32_t &group, uint32_t &row_tile)
{
    const CostShare s = tile_cost_share(g, xcd);
    if (slot >= s.n_full + s.n_half) return false;
    if (slot >= s.n_full) {
        half_tile_at(g, s.half_begin + (slot - s.n_full), group, row_tile);
        return true;
    }
    const uint32_t t = s.full_begin + slot;
    const uint32_t n_super = (n_full_groups(g) + g.group_span - 1u) / g.group_span;
    if (g.n_prefix_inline != 0u) {
        uint32_t lo = 0, base = 0;
        SKL_MAP_UNROLL
        for (int x = 1; x < TILE_PREFIX_INLINE; ++x) {
            if ((uint32_t)x < n_super && g.tile_prefix_inline[x] <= t) {
                lo = (uint32_t)x;
                base = g.tile_prefix_inline[x];
            }
        }
        full_tile_in_supergroup(g, lo, t - base, group, row_tile);
        return true;
    }
    uint32_t lo = 0, hi = n_super;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (g.tile_prefix[mid] <= t) lo = mid; else hi = mid;
    }
    full_tile_in_supergroup(g, lo, t - g.tile_prefix[lo], group, row_tile);
    return true;
}

// Forward in this order: the (XCD, slot) of active tile (group, row_tile) -- what the plan promises the decode above
template <class G>
SKL_MAP_FN void tile_slot_by_cost(const G &g, uint32_t group, uint32_t row_tile, uint32_t &xcd, uint32_t &slot)
{
    const uint32_t n_full_here = group_full_row_tiles(g, group);
    const bool half = row_tile >= n_full_here;
    uint32_t t;
    if (half) {
        const HalfRuns r = half_tile_runs(g);
        const bool in_runs = group < n_full_groups(g);   // (then ga <= group <= gb: no other group has a half tile)
        t = (!in_runs ? r.h_a + r.n_mid * r.per + r.h_b : group == r.ga ? 0u : r.h_a + (group - r.ga - 1u) * r.per) + (row_tile - n_full_here);
    } else {
        const uint32_t sg = group / g.group_span, first = sg * g.group_span;
        const uint32_t gcount = map_min(g.group_span, n_full_groups(g) - first);
        t = g.n_prefix_inline != 0u ? g.tile_prefix_inline[sg] : g.tile_prefix[sg];
        uint32_t lo_at = 0;
        for (uint32_t gi = 0; gi < gcount; ++gi) {   // the stretch of row tiles the groups from gi on share
            const uint32_t width = gcount - gi, n_gi = group_full_row_tiles(g, first + gi);
            if (row_tile < n_gi) {
                t += (row_tile - lo_at) * width + (group - first - gi);
                break;
            }
            t += (n_gi - lo_at) * width;
            lo_at = n_gi;
        }
    }
    for (xcd = 0;; ++xcd) {
        const CostShare s = tile_cost_share(g, xcd);
        const uint32_t begin = half ? s.half_begin : s.full_begin, count = half ? s.n_half : s.n_full;
        if (t < begin + count) {
            slot = (half ? s.n_full : 0u) + (t - begin);
            return;
        }
    }
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
