// unit_table.hpp -- THE UNIT TABLE of a k-sliced launch of the chunk-split kernel (pair_kslice.hip): what every workgroup of the
// grid computes, decoded ONCE on the host into one 16-byte descriptor per workgroup, in grid order, instead of by every wave of
// every launch at its head.  The decode is a pure function of the launch's shape, and a shape comes back call after call (a
// repeated dist on a resident slab, the bands of a banded call), so the table is cached under a key of every field the decode
// reads (UnitKey, UnitCache).
//
// The table is BUILT with the functions of work_map.hpp themselves -- kslice_unit, lookup_tile_at / lookup_tile_by_cost_at,
// slice_chunk_range, tile_skips_block0/1 -- composed as the kernel's head composes them, so the numbering stays written in one
// place; tests/native/unit_table_check.cpp holds the head's sequence restated and compares the two workgroup by workgroup.
// Pure: no device header, nothing here touches a device (kernels.hip stage_unit_table uploads what build_unit_table made).
#pragma once

#include <stdint.h>
#include <string.h>

#include "work_map.hpp"

namespace skl {

constexpr uint32_t UNIT_TABLE_MAX_WG = 65536;   // workgroups of a launch that gets a table: 1 MiB of descriptors
constexpr int UNIT_CACHE_ENTRIES = 4;           // tables a context keeps (the band loop of a dense call alternates shapes)

// One workgroup's descriptor.  Every early `return` of the kernel's own decode -- a slot past an XCD's share, a tile past the
// band or on / below the diagonal, a block of sample ids that wants fewer lengths -- is UNIT_NONE: the grid stays as planned.
//   a0         first row of the tile
//   jb0_flags  bits 0-25 first 64-column block; 26-27 the half-tile case (UNIT_WALK_*); 28 adds into plane 1 (a tail slice
//              other than slice 0); 29-30 wave priority of the workgroup's round; 31 none
//   cb_kk      bits 0-23 c_begin, 24-31 k index
//   ce_slice   bits 0-23 c_end, 24-31 chunk slice
struct UnitDesc {
    uint32_t a0, jb0_flags, cb_kk, ce_slice;
};
static_assert(sizeof(UnitDesc) == 16, "one s_load_dwordx4 per workgroup");

constexpr uint32_t UNIT_JB_MASK = (1u << 26) - 1u;
constexpr uint32_t UNIT_WALK_SHIFT = 26, UNIT_WALK_BOTH = 0u, UNIT_WALK_1_2 = 1u, UNIT_WALK_0_1 = 2u;   // 64-column blocks walked: 0-2, 1-2, 0-1
constexpr uint32_t UNIT_PLANE1 = 1u << 28;
constexpr uint32_t UNIT_PRIO_SHIFT = 29;
constexpr uint32_t UNIT_NONE = 1u << 31;
constexpr uint32_t UNIT_CHUNK_MASK = (1u << 24) - 1u;

SKL_MAP_FN bool unit_none(const UnitDesc &d) { return (d.jb0_flags & UNIT_NONE) != 0u; }
SKL_MAP_FN uint32_t unit_jb0(const UnitDesc &d) { return d.jb0_flags & UNIT_JB_MASK; }
SKL_MAP_FN uint32_t unit_walk(const UnitDesc &d) { return (d.jb0_flags >> UNIT_WALK_SHIFT) & 3u; }
SKL_MAP_FN bool unit_plane1(const UnitDesc &d) { return (d.jb0_flags & UNIT_PLANE1) != 0u; }
SKL_MAP_FN uint32_t unit_prio(const UnitDesc &d) { return (d.jb0_flags >> UNIT_PRIO_SHIFT) & 3u; }
SKL_MAP_FN uint32_t unit_c_begin(const UnitDesc &d) { return d.cb_kk & UNIT_CHUNK_MASK; }
SKL_MAP_FN uint32_t unit_kk0(const UnitDesc &d) { return d.cb_kk >> 24; }
SKL_MAP_FN uint32_t unit_c_end(const UnitDesc &d) { return d.ce_slice & UNIT_CHUNK_MASK; }
SKL_MAP_FN uint32_t unit_slice(const UnitDesc &d) { return d.ce_slice >> 24; }

// Does a planned k-sliced launch of n_wg workgroups fit the table and its fields?  (g: after plan_kslice_grid)
template <class G>
inline bool unit_table_fits(const G &g, uint64_t n_wg)
{
    const uint32_t slices = g.tail_slices > 1u ? g.tail_slices : (g.k_slices != 0u ? g.k_slices : 1u);
    return n_wg != 0u && n_wg <= UNIT_TABLE_MAX_WG && g.ss64 <= UNIT_CHUNK_MASK && g.k_count <= 256u && slices <= 256u && g.n_jblocks <= UNIT_JB_MASK;
}

// What workgroup b of the grid computes: the head of pair_kernel_kslice<R, 2, counts ? COUNTS : JACCARD, k-sliced>, step by
// step.  g: the planned launch with tile_prefix pointing at a HOST copy of the prefix table (or the table inline);
// block_ke: the host's copy of PairArgs::block_ke (null when the launch has none).
template <class G>
inline UnitDesc unit_of(const G &g, uint32_t b, uint32_t R, bool counts, const uint8_t *block_ke)
{
    const UnitDesc none = {0u, UNIT_NONE, 0u, 0u};
    const uint32_t xcd = b & ((1u << g.xcd_shift) - 1u), s_idx = b >> g.xcd_shift;
    const KsliceUnit u = kslice_unit(g, s_idx, true, counts);
    if (u.none) return none;
    const uint32_t prio = !u.tail_mode && g.round_size != 0u ? map_min(s_idx / g.round_size, 3u) : 0u;
    uint32_t c_begin, c_end;
    slice_chunk_range(g, u.n_slices, u.slice, c_begin, c_end);
    uint32_t jg, at;
    const bool by_cost = counts && R == 16u && g.tile_cost_order != 0u;
    if (!(by_cost ? lookup_tile_by_cost_at(g, xcd, u.slot, jg, at) : lookup_tile_at(g, xcd, u.slot, jg, at))) return none;
    const uint32_t jb0 = jg * 2u, a0 = g.row_begin + at * R;
    if (jb0 >= g.n_jblocks || a0 >= g.row_end) return none;
    if (g.self_mode && a0 >= (jg + 1u) * 128u - 1u) return none;   // tile entirely on / below the diagonal
    if (counts && block_ke != nullptr) {   // the early break decided per block: this tile's block(s) may want fewer lengths
        const uint32_t r_last = map_min(a0 + R, g.row_end) - 1u;
        const uint32_t bc = (jb0 * 64u) >> g.blk_shift_c;
        const uint32_t ke_a = block_ke[(size_t)(a0 >> g.blk_shift_r) * g.blk_cols + bc];
        const uint32_t ke_b = block_ke[(size_t)(r_last >> g.blk_shift_r) * g.blk_cols + bc];
        if (u.kk0 >= (ke_a > ke_b ? ke_a : ke_b)) return none;
    }
    const bool half_ok = R == 16u && g.no_half_tiles == 0u;
    const uint32_t walk = half_ok && tile_skips_block0(g.self_mode, a0, jb0) ? UNIT_WALK_1_2
                        : half_ok && tile_skips_block1(jb0, g.n_jblocks)    ? UNIT_WALK_0_1
                                                                             : UNIT_WALK_BOTH;
    UnitDesc d;
    d.a0 = a0;
    d.jb0_flags = jb0 | (walk << UNIT_WALK_SHIFT) | (u.in_tail && u.slice != 0u ? UNIT_PLANE1 : 0u) | (prio << UNIT_PRIO_SHIFT);
    d.cb_kk = c_begin | (u.kk0 << 24);
    d.ce_slice = c_end | (u.slice << 24);
    return d;
}

template <class G>
inline void build_unit_table(const G &g, uint32_t R, bool counts, const uint8_t *block_ke, uint64_t n_wg, UnitDesc *table)
{
    for (uint64_t b = 0; b < n_wg; ++b) table[b] = unit_of(g, (uint32_t)b, R, counts, block_ke);
}

// ---------------------------------------------------------------------------
// the cache: a key of every field unit_of() reads, a few entries, the least recently used one evicted
// ---------------------------------------------------------------------------

struct UnitKey {
    uint64_t v[18];
};
inline bool operator==(const UnitKey &a, const UnitKey &b) { return memcmp(a.v, b.v, sizeof a.v) == 0; }

inline uint64_t unit_hash_bytes(const uint8_t *p, size_t n)   // FNV-1a
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

// (the prefix table is a function of the fields below: no need to hash it; block_ke is the caller's data: hashed)
template <class G>
inline UnitKey unit_key(const G &g, uint32_t R, bool counts, const uint8_t *block_ke, size_t block_ke_bytes, uint64_t n_wg)
{
    auto two = [](uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; };
    UnitKey k;
    k.v[0] = n_wg;
    k.v[1] = two(R, counts ? 1u : 0u);
    k.v[2] = two(g.row_begin, g.row_end);
    k.v[3] = two(g.nB, g.self_mode);
    k.v[4] = two(g.k_count, g.ss64);
    k.v[5] = two(g.xcd_shift, g.xcd_interleave);
    k.v[6] = two(g.group_span, g.n_groups);
    k.v[7] = two(g.tile_rows, g.group_cols);
    k.v[8] = two(g.a_tiles, g.n_jblocks);
    k.v[9] = two(g.n_active_tiles, g.tiles_per_xcd);
    k.v[10] = two(g.tile_cost_order, g.n_full_tiles);
    k.v[11] = two(g.k_slices, g.slice_chunks);
    k.v[12] = two(g.tail_slices, g.tail_first);
    k.v[13] = two(g.round_size, g.no_half_tiles);
    k.v[14] = two(g.n_prefix_inline, block_ke != nullptr ? 1u : 0u);
    k.v[15] = block_ke != nullptr ? two(g.blk_shift_r, g.blk_shift_c) : 0ull;
    k.v[16] = block_ke != nullptr ? two(g.blk_cols, (uint32_t)block_ke_bytes) : 0ull;
    k.v[17] = block_ke != nullptr ? unit_hash_bytes(block_ke, block_ke_bytes) : 0ull;
    return k;
}

struct UnitCache {
    UnitKey key[UNIT_CACHE_ENTRIES];
    uint64_t used[UNIT_CACHE_ENTRIES] = {};   // clock of the entry's last use (0: empty)
    uint64_t clock = 0;
    uint64_t hits = 0, builds = 0;

    // the entry of key k; *hit: it already holds k's table, else it is the caller's to fill (an empty entry, or the one unused longest)
    int lookup(const UnitKey &k, bool *hit)
    {
        ++clock;
        for (int i = 0; i < UNIT_CACHE_ENTRIES; ++i) {
            if (used[i] != 0u && key[i] == k) {
                used[i] = clock;
                ++hits;
                *hit = true;
                return i;
            }
        }
        int victim = 0;
        for (int i = 1; i < UNIT_CACHE_ENTRIES; ++i) {
            if (used[i] < used[victim]) victim = i;
        }
        key[victim] = k;
        used[victim] = clock;
        ++builds;
        *hit = false;
        return victim;
    }
    void drop(int entry) { used[entry] = 0; }   // the fill failed: the entry holds nothing
};

}  // namespace skl
