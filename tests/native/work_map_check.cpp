// work_map_check.cpp -- CPU check of csrc/work_map.hpp: which workgroup of a pair-kernel launch computes what (test infrastructure).
// Host compiler only: the header alone, no device header, no device, the library is never loaded.  The plan (forward) and the
// kernels' decode (inverse) are run against each other:
//   work_map_check tiles  : every small launch shape -- the (XCD, slot) pairs of the planned grid yield every tile once, the
//                           tiles hold every pair the launch owes once, nothing else
//   work_map_check units  : the chunk-split kernel's k-sliced grid -- every workgroup index of the planned grid is one (tile
//                           slot, k index, chunk slice), each once, the slices of a unit partition the sketch
//   work_map_check pinned : cases whose numbers are derived BY HAND from the rules (the arithmetic stands beside each case)
// Prints one line per failed check and "ok <checks>" / "FAILED <failures> of <checks>"; the exit status says which.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sketchlib.rust_amd/csrc/work_map.hpp"

using namespace skl;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) {                                                       \
            ++g_failed;                                                      \
            if (g_failed <= 40) printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                    \
    } while (0)
#define CHECK_EQ(a, b)                                                                                          \
    do {                                                                                                        \
        ++g_checks;                                                                                             \
        const long long a_ = (long long)(a), b_ = (long long)(b);                                               \
        if (a_ != b_) {                                                                                         \
            ++g_failed;                                                                                         \
            if (g_failed <= 40) printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #a, a_, b_);    \
        }                                                                                                       \
    } while (0)

// The fields of PairArgs (kernels.h) the map reads and writes, under the same names.
struct Map {
    uint32_t nB = 0, ss64 = 0, k_count = 1;
    uint32_t row_begin = 0, row_end = 0, self_mode = 0;
    uint32_t a_tiles = 0, n_jblocks = 0, n_active_tiles = 0, tiles_per_xcd = 0, xcd_interleave = 0, xcd_shift = 0;
    uint32_t n_groups = 0, group_span = 0, tile_rows = 0, group_cols = 0;
    const uint32_t *tile_prefix = nullptr;
    uint32_t inline_prefix_ok = 0, n_prefix_inline = 0, tile_prefix_inline[TILE_PREFIX_INLINE] = {};
    uint32_t slice_chunks = 0, k_slices = 0, tail_slices = 0, tail_first = 0, tail_resident = 0, round_size = 0;
};

// plan_tiles() without the device: geometry, numbering, and the "uploaded" table is the host vector itself -- or nothing at all
// when the table rides in the arguments, so that the inline search is seen not to need it
static bool plan(Map &g, uint32_t rows_per_tile, uint32_t cols_per_group, std::vector<uint32_t> &prefix, uint64_t *grid)
{
    plan_tile_geometry(g, rows_per_tile, cols_per_group);
    prefix.assign(g.self_mode ? n_supergroups(g) + 1u : 0u, 0u);
    if (!plan_tile_numbering(g, prefix.data(), grid)) return false;
    if (g.self_mode && g.n_prefix_inline == 0u) g.tile_prefix = prefix.data();
    return true;
}

static Map launch(uint32_t nB, uint32_t row_begin, uint32_t row_end, bool self, uint32_t span, uint32_t xcd_shift, bool interleave, bool inline_ok)
{
    Map g;
    g.nB = nB;
    g.row_begin = row_begin;
    g.row_end = row_end;
    g.self_mode = self;
    g.group_span = span;
    g.xcd_shift = xcd_shift;
    g.xcd_interleave = interleave;
    g.inline_prefix_ok = inline_ok;
    return g;
}

// ---------------------------------------------------------------------------
// tiles
// ---------------------------------------------------------------------------
static long g_pairless = 0;

static void tiles_of_shape(uint32_t R, uint32_t W, uint32_t nB, uint32_t r0, uint32_t r1, bool self)
{
    // the cells (row tile, column group) that hold a pair the launch owes, pair by pair: row in the band, column below nB, i < j
    // in self mode.  A pair lies in one cell, so "every owed pair in exactly one yielded tile" is "every such cell yielded once".
    const uint32_t a_tiles = (r1 - r0 + R - 1) / R, n_groups = (nB + W - 1) / W;
    std::vector<uint8_t> need((size_t)a_tiles * n_groups, 0);
    for (uint32_t i = r0; i < r1; ++i) {
        for (uint32_t j = self ? i + 1 : 0; j < nB; ++j) need[(size_t)((i - r0) / R) * n_groups + j / W] = 1;
    }
    std::vector<uint32_t> prefix;
    std::vector<uint8_t> got(need.size());
    for (uint32_t span = 1; span <= 4; ++span) {
        for (uint32_t shift = 0; shift <= 3; ++shift) {
            for (int flags = 0; flags < 4; ++flags) {
                Map g = launch(nB, r0, r1, self, span, shift, (flags & 1) != 0, (flags & 2) != 0);
                uint64_t grid = 0;
                CHECK(plan(g, R, W, prefix, &grid));
                CHECK_EQ(g.a_tiles, a_tiles);
                CHECK_EQ(g.n_groups, n_groups);
                CHECK_EQ(grid, (uint64_t)g.tiles_per_xcd << shift);                        // (e)
                CHECK((grid == 0) == (g.n_active_tiles == 0));
                CHECK(!self || !(flags & 2) || (g.n_prefix_inline != 0u) == (n_supergroups(g) + 1u <= (uint32_t)TILE_PREFIX_INLINE));
                std::fill(got.begin(), got.end(), 0);
                uint32_t yielded = 0;
                for (uint32_t xcd = 0; xcd < (1u << shift); ++xcd) {
                    for (uint32_t slot = 0; slot <= g.tiles_per_xcd; ++slot) {
                        uint32_t jg = ~0u, at = ~0u;
                        if (!lookup_tile_at(g, xcd, slot, jg, at)) continue;               // (d): the slots that yield nothing
                        ++yielded;
                        CHECK(slot < g.tiles_per_xcd && jg < n_groups && at < a_tiles);
                        if (jg >= n_groups || at >= a_tiles) continue;
                        CHECK_EQ(got[(size_t)at * n_groups + jg]++, 0);                    // (a): no tile twice
                        // the kernels' defensive early returns (first column block past the end, first row past the band, tile
                        // entirely on or below the diagonal): none fires for a tile the map yields
                        const uint32_t a0 = r0 + at * R;
                        CHECK(jg * (W / 64u) < g.n_jblocks && a0 < r1 && !(self && a0 >= (jg + 1u) * W - 1u));
                        if (!need[(size_t)at * n_groups + jg]) {                           // (c): only past the launch's last column
                            ++g_pairless;
                            CHECK(self && jg == n_groups - 1u && a0 + 1u >= nB);
                        }
                    }
                }
                CHECK_EQ(yielded, g.n_active_tiles);                                       // (a), (d)
                for (size_t c = 0; c < need.size(); ++c) CHECK(!need[c] || got[c] == 1);   // (b)
            }
        }
    }
}

static void tiles()
{
    const uint32_t shapes[3][2] = {{16, 128}, {32, 128}, {8, 64}};
    const uint32_t sizes[] = {1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 413, 511, 513, 640, 700};
    for (const auto &s : shapes) {
        for (uint32_t nB : sizes) {
            const uint32_t R = s[0], W = s[1];
            for (int self = 0; self < 2; ++self) {
                const uint32_t rows = self ? nB : (nB % 2 ? 77u : 300u);   // cross mode: the row side has its own size
                tiles_of_shape(R, W, nB, 0, rows, self);                                   // the whole range
                if (rows > 12) tiles_of_shape(R, W, nB, 5, rows - 3, self);                // off the tile boundary at both ends
                tiles_of_shape(R, W, nB, rows / 2, rows / 2 + 1, self);                    // one row
                tiles_of_shape(R, W, nB, rows - 1, rows, self);   // self: the last sample's row owes nothing -- no tile at all when nB fills its group
                // below the diagonal of the first column group(s): they get no tile, the numbering starts further right
                if (rows > W) tiles_of_shape(R, W, nB, W - 1, rows < W + 40 ? rows : W + 40, self);
                if (rows > 3 * W) tiles_of_shape(R, W, nB, 3 * W - 1, rows, self);
            }
        }
    }
    {   // grid 0: one group, the band on its last column
        std::vector<uint32_t> prefix;
        Map g = launch(128, 127, 128, true, 2, 3, false, true);
        uint64_t grid = 99;
        CHECK(plan(g, 16, 128, prefix, &grid));
        CHECK(grid == 0 && g.n_active_tiles == 0 && g.tiles_per_xcd == 0);
    }
    printf("tiles without an owed pair (all in the last column group, from the launch's last sample on): %ld\n", g_pairless);
}

// ---------------------------------------------------------------------------
// units
// ---------------------------------------------------------------------------

// dense_plan.hpp slice_plan(), restated: `wanted` slices of whole stages (8 chunks), the last one shorter; sketches below 16
// chunks are not cut
static uint32_t slices_for(uint32_t ss64, uint32_t wanted, uint32_t *chunks)
{
    *chunks = 0;
    if (wanted < 2u || ss64 < 16u) return 1u;
    *chunks = ((ss64 + wanted - 1u) / wanted + 7u) / 8u * 8u;
    return (ss64 + *chunks - 1u) / *chunks;
}

static void units_of(Map g, bool ksl, bool counts)
{
    const uint32_t want_k = g.k_slices, want_tail = g.tail_slices;
    uint64_t n_wg = 0;
    CHECK(plan_kslice_grid(g, ksl, counts, &n_wg));
    const bool sliceable = ksl && counts, tail = sliceable && want_tail > 1u;
    CHECK_EQ(g.tail_slices, sliceable ? want_tail : 0u);
    CHECK_EQ(g.k_slices, sliceable && !tail && want_k > 1u ? want_k : 1u);
    const uint32_t S = tail ? g.tail_slices : g.k_slices, nk = ksl ? g.k_count : 1u, n_xcd = 1u << g.xcd_shift;
    if (tail) CHECK(g.tail_first <= g.tiles_per_xcd * nk && g.tail_first % g.tail_resident == 0 && g.tiles_per_xcd * nk - g.tail_first < g.tail_resident);
    CHECK(n_wg % n_xcd == 0);
    // per (slot, k index): the slices seen (bit s) and the chunks they cover
    std::vector<uint32_t> seen((size_t)g.tiles_per_xcd * nk), covered(seen.size());
    for (uint32_t xcd = 0; xcd < n_xcd; xcd += n_xcd > 1 ? n_xcd - 1 : 1) {   // (the decode does not see the XCD: the first and the last)
        std::fill(seen.begin(), seen.end(), 0u);
        std::fill(covered.begin(), covered.end(), 0u);
        uint64_t walked = 0;
        for (uint64_t b = xcd; b < n_wg; b += n_xcd, ++walked) {
            const uint32_t s_idx = (uint32_t)(b >> g.xcd_shift);
            const KsliceUnit u = kslice_unit(g, s_idx, ksl, counts);
            CHECK(!u.none);   // the grid is exact: no padding slots
            if (u.none) continue;
            CHECK(u.slot < g.tiles_per_xcd && u.kk0 < nk && u.slice < u.n_slices);
            if (u.slot >= g.tiles_per_xcd || u.kk0 >= nk || u.slice >= u.n_slices) continue;
            CHECK_EQ(u.tail_mode, tail);
            CHECK_EQ(u.in_tail, tail && s_idx >= g.tail_first);   // below tail_first: whole units
            CHECK_EQ(u.n_slices, tail ? (u.in_tail ? S : 1u) : S);
            uint32_t c0 = ~0u, c1 = ~0u;
            slice_chunk_range(g, u.n_slices, u.slice, c0, c1);
            CHECK(c0 < c1 && c1 <= g.ss64 && c0 % 8u == 0);       // non-empty, begins on a whole stage
            const size_t at = (size_t)u.slot * nk + u.kk0;
            CHECK((seen[at] & (1u << u.slice)) == 0u);
            seen[at] |= 1u << u.slice;
            // the slices of a unit come in order, so "they partition [0, ss64)" is: each begins where the one before ended
            if (u.slice == 0) CHECK_EQ(c0, 0);
            if (u.slice + 1u == u.n_slices) CHECK_EQ(c1, g.ss64);
            covered[at] += c1 - c0;
            if (u.n_slices > 1u && u.slice > 0u) {
                uint32_t p0, p1;
                slice_chunk_range(g, u.n_slices, u.slice - 1u, p0, p1);
                CHECK_EQ(p1, c0);
            }
            // a unit is whole or sliced, never both: a whole unit's only "slice" is 0 of 1
            if (u.n_slices == 1u) CHECK(c0 == 0u && c1 == g.ss64);
        }
        CHECK_EQ(walked, n_wg >> g.xcd_shift);
        uint64_t expect = 0;
        for (size_t at = 0; at < seen.size(); ++at) {   // every (slot, k index): once whole, or once per slice
            CHECK_EQ(covered[at], g.ss64);
            CHECK(seen[at] == 1u || seen[at] == (1u << S) - 1u);
            expect += seen[at] == 1u ? 1u : S;
            if (!tail && S > 1u) CHECK_EQ(seen[at], (1u << S) - 1u);
        }
        CHECK_EQ(expect, n_wg >> g.xcd_shift);          // n_wg is the sum just enumerated
    }
}

static void units()
{
    const uint32_t tiles_list[] = {1, 31, 32, 33, 64, 70}, ss_list[] = {8, 16, 24, 64, 157, 1016}, resident[] = {1, 3, 8, 100, 1000};
    std::vector<Map> maps;
    for (uint32_t t : tiles_list) {
        Map g;
        g.tiles_per_xcd = t;
        g.xcd_shift = t % 2 ? 3 : 0;
        maps.push_back(g);
    }
    {   // ... and real tile maps: 413 samples against themselves (74 tiles of 16 x 128: 10 per XCD; interleaved: 32), 700 x 300
        std::vector<uint32_t> prefix;
        uint64_t grid;
        Map a = launch(413, 0, 413, true, 2, 3, false, true), b = launch(413, 0, 413, true, 2, 3, true, true), c = launch(300, 0, 700, false, 2, 2, false, true);
        CHECK(plan(a, 16, 128, prefix, &grid) && a.tiles_per_xcd == 10);
        CHECK(plan(b, 16, 128, prefix, &grid) && b.tiles_per_xcd == 32);
        CHECK(plan(c, 32, 128, prefix, &grid) && c.tiles_per_xcd == 17);   // 22 x 3 = 66 tiles over 4 XCDs
        a.tile_prefix = b.tile_prefix = nullptr;
        maps.insert(maps.end(), {a, b, c});
    }
    for (Map g : maps) {
        for (g.k_count = 1; g.k_count <= 6; ++g.k_count) {
            for (uint32_t ss64 : ss_list) {
                g.ss64 = ss64;
                g.round_size = 128;
                for (uint32_t want : {1u, 2u, 4u, 8u}) {
                    g.tail_slices = 0;
                    g.k_slices = slices_for(ss64, want, &g.slice_chunks);
                    units_of(g, true, true);    // k-sliced counts: sliced
                    units_of(g, true, false);   // k-sliced single-k keys: never
                    units_of(g, false, false);  // all k in one workgroup: one per tile
                }
                for (uint32_t want : {2u, 4u}) {
                    for (uint32_t res : resident) {
                        g.k_slices = 1;
                        g.tail_slices = slices_for(ss64, want, &g.slice_chunks);
                        g.tail_resident = res;
                        units_of(g, true, true);
                        units_of(g, true, false);
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// pinned
// ---------------------------------------------------------------------------
static void expect_tile(const Map &g, uint32_t xcd, uint32_t slot, bool yields, uint32_t group, uint32_t row_tile)
{
    uint32_t jg = ~0u, at = ~0u;
    CHECK_EQ(lookup_tile_at(g, xcd, slot, jg, at), yields);
    if (yields) {
        CHECK_EQ(jg, group);
        CHECK_EQ(at, row_tile);
    }
}

static void expect_unit(const Map &g, uint32_t s_idx, bool none, uint32_t slot, uint32_t kk0, uint32_t slice, uint32_t n_slices, bool in_tail)
{
    const KsliceUnit u = kslice_unit(g, s_idx, true, true);
    CHECK_EQ(u.none, none);
    if (none) return;
    CHECK_EQ(u.slot, slot);
    CHECK_EQ(u.kk0, kk0);
    CHECK_EQ(u.slice, slice);
    CHECK_EQ(u.n_slices, n_slices);
    CHECK_EQ(u.in_tail, in_tail);
}

static Map grid_case(uint32_t tiles_per_xcd, uint32_t k_count, uint32_t ss64, uint32_t k_slices, uint32_t slice_chunks, uint32_t tail_slices, uint32_t tail_resident,
                     uint32_t round_size = 0)
{
    Map g;
    g.xcd_shift = 3;
    g.tiles_per_xcd = tiles_per_xcd;
    g.k_count = k_count;
    g.ss64 = ss64;
    g.k_slices = k_slices;
    g.slice_chunks = slice_chunks;
    g.tail_slices = tail_slices;
    g.tail_resident = tail_resident;
    g.round_size = round_size;
    return g;
}

static void pinned()
{
    std::vector<uint32_t> prefix;
    uint64_t grid = 0, n_wg = 0;
    CHECK_EQ(KSL_TILE_BLOCK, 32);
    CHECK_EQ(1u << XCD_DEAL_SHIFT, 32);
    // ---- 413 samples against themselves, 16 x 128 tiles, two groups side by side, 8 XCDs.  4 column groups with last columns 127, 255,
    // 383, 511: rows below min(413, that): 127, 255, 383, 413 -> 8, 16, 24, 26 row tiles: 74 tiles, super-groups start at 0, 24, 74;
    // ceil(74 / 8) = 10 per XCD, 80 workgroups
    for (int inline_ok = 0; inline_ok < 2; ++inline_ok) {
        Map g = launch(413, 0, 413, true, 2, 3, false, inline_ok != 0);
        CHECK(plan(g, 16, 128, prefix, &grid));
        CHECK(g.a_tiles == 26 && g.n_groups == 4 && g.n_jblocks == 7 && g.n_active_tiles == 74 && g.tiles_per_xcd == 10 && grid == 80);
        CHECK(prefix.size() == 3 && prefix[0] == 0 && prefix[1] == 24 && prefix[2] == 74);
        CHECK_EQ(g.n_prefix_inline, inline_ok ? 3 : 0);
        CHECK(!inline_ok || (g.tile_prefix_inline[1] == 24 && g.tile_prefix_inline[2] == 74));
        // super-group 0 = groups 0 (8 row tiles) and 1 (16): row tiles 0..7 two wide (16 tiles), 8..15 group 1 alone
        expect_tile(g, 0, 0, true, 0, 0);
        expect_tile(g, 0, 1, true, 1, 0);
        expect_tile(g, 1, 5, true, 1, 7);     // tile 15: row tile 7, second group
        expect_tile(g, 1, 6, true, 1, 8);     // tile 16: the first of group 1 alone
        expect_tile(g, 2, 3, true, 1, 15);    // tile 23: the last of super-group 0
        expect_tile(g, 2, 4, true, 2, 0);     // tile 24: super-group 1 = groups 2 (24 row tiles) and 3 (26)
        expect_tile(g, 7, 0, true, 2, 23);    // tile 70 = 24 + 46: row tile 23, first group
        expect_tile(g, 7, 1, true, 3, 23);    // tile 71: ... second group, the last two wide
        expect_tile(g, 7, 2, true, 3, 24);    // tile 72 = 24 + 48: group 3 alone
        expect_tile(g, 7, 3, true, 3, 25);    // tile 73, the last
        expect_tile(g, 7, 4, false, 0, 0);    // tile 74: none
        expect_tile(g, 0, 10, false, 0, 0);   // a slot past the XCD's share, although tile 10 exists
    }
    {   // the same interleaved: ceil(74 / 32) = 3 blocks of 32 dealt to 8 XCDs: one block each, 32 slots per XCD, 256 workgroups
        Map g = launch(413, 0, 413, true, 2, 3, true, true);
        CHECK(plan(g, 16, 128, prefix, &grid));
        CHECK(g.n_active_tiles == 74 && g.tiles_per_xcd == 32 && grid == 256);
        expect_tile(g, 1, 0, true, 2, 4);     // tile 32 = 24 + 8: row tile 4, first group of super-group 1
        expect_tile(g, 2, 9, true, 3, 25);    // tile 64 + 9 = 73
        expect_tile(g, 2, 10, false, 0, 0);   // tile 74
        expect_tile(g, 3, 0, false, 0, 0);    // tile 96
        // cross mode, 8 x 64 tiles, 70 rows x 129 columns on 2 XCDs: 9 row tiles x 3 groups = 27 tiles = one block of 32, which XCD 0
        // takes: 32 slots per XCD all the same, 64 workgroups; group by group (span 1), 9 tiles each
        Map h = launch(129, 0, 70, false, 1, 1, true, true);
        CHECK(plan(h, 8, 64, prefix, &grid));
        CHECK(h.a_tiles == 9 && h.n_groups == 3 && h.n_active_tiles == 27 && h.tiles_per_xcd == 32 && grid == 64);
        expect_tile(h, 0, 26, true, 2, 8);
        expect_tile(h, 0, 27, false, 0, 0);
        expect_tile(h, 1, 0, false, 0, 0);    // tile 32
        // 257 rows: 33 row tiles x 3 groups = 99 tiles = 4 blocks, 2 per XCD: XCD 1 slot 37 = its block 1 = block 3 of the numbering:
        // tile 96 + 5 = 101 = 3 x 33 + 2: beyond; slot 34 = tile 98 = 2 x 33 + 32: group 2, row tile 32, the last
        Map k = launch(129, 0, 257, false, 1, 1, true, true);
        CHECK(plan(k, 8, 64, prefix, &grid));
        CHECK(k.n_active_tiles == 99 && k.tiles_per_xcd == 64 && grid == 128);
        expect_tile(k, 1, 34, true, 2, 32);
        expect_tile(k, 1, 37, false, 0, 0);
        expect_tile(k, 1, 5, true, 1, 4);     // block 1: tile 37 = 33 + 4
    }
    {   // cross mode: rows [10, 75) against 300 columns, 32 x 128: 3 row tiles x 3 groups = 9 tiles, 2 XCDs: 5 each, 10 workgroups.
        // Numbering: super-groups of 2 groups x 3 row tiles = 6 tiles, groups side by side; the last super-group has one group
        Map g = launch(300, 10, 75, false, 2, 1, false, true);
        CHECK(plan(g, 32, 128, prefix, &grid));
        CHECK(g.a_tiles == 3 && g.n_groups == 3 && g.n_jblocks == 5 && g.n_active_tiles == 9 && g.tiles_per_xcd == 5 && grid == 10 && g.n_prefix_inline == 0);
        expect_tile(g, 0, 3, true, 1, 1);     // tile 3: row tile 1, second group
        expect_tile(g, 1, 2, true, 2, 1);     // tile 7 = 6 + 1: one group wide
        expect_tile(g, 1, 3, true, 2, 2);     // tile 8
        expect_tile(g, 1, 4, false, 0, 0);    // tile 9
    }
    {   // too many tiles: 2^28 row tiles of 8 rows x 8 groups = 2^31; x 7 groups fits
        Map g = launch(512, 0, 0x80000000u, false, 1, 3, false, true);
        CHECK(!plan(g, 8, 64, prefix, &grid) && grid == 0);
        Map h = launch(448, 0, 0x80000000u, false, 1, 3, false, true);
        CHECK(plan(h, 8, 64, prefix, &grid) && h.n_active_tiles == 7u << 28 && grid == 7ull << 28);
    }
    // ---- the chunk-split grid, 8 XCDs.  Uniform slices: 10 tiles x 5 lengths x 4 slices x 8 XCDs; 64 chunks = 4 x 16
    {
        Map g = grid_case(10, 5, 64, 4, 0, 0, 0);
        CHECK(plan_kslice_grid(g, true, true, &n_wg) && n_wg == 1600 && g.k_slices == 4 && g.tail_slices == 0);
        uint32_t c0, c1;
        slice_chunk_range(g, 4, 3, c0, c1);
        CHECK(c0 == 48 && c1 == 64);
        // single-k keys are never sliced, nor is the all-k form, which has one workgroup per tile
        Map j = grid_case(10, 5, 64, 4, 16, 2, 100);
        CHECK(plan_kslice_grid(j, true, false, &n_wg) && n_wg == 400 && j.k_slices == 1 && j.tail_slices == 0 && j.slice_chunks == 0);
        Map a = grid_case(10, 5, 64, 4, 16, 2, 100, 128);
        CHECK(plan_kslice_grid(a, false, true, &n_wg) && n_wg == 80 && a.k_slices == 1 && a.tail_slices == 0 && a.round_size == 0);
    }
    {   // the launcher's refusals
        Map g = grid_case(10, 5, 24, 2, 0, 0, 0);      // 24 chunks in 2 even slices of whole stages: 24 % 16 != 0
        CHECK(!plan_kslice_grid(g, true, true, &n_wg));
        g = grid_case(10, 5, 24, 2, 12, 0, 0);         // slices of 12 chunks: not whole stages
        CHECK(!plan_kslice_grid(g, true, true, &n_wg));
        g = grid_case(10, 5, 24, 2, 8, 0, 0);          // 2 x 8 < 24: chunks left over
        CHECK(!plan_kslice_grid(g, true, true, &n_wg));
        g = grid_case(10, 5, 24, 2, 24, 0, 0);         // 1 x 24 >= 24: the last slice is empty
        CHECK(!plan_kslice_grid(g, true, true, &n_wg));
        g = grid_case(10, 5, 24, 2, 16, 0, 0);         // [0, 16) and [16, 24)
        CHECK(plan_kslice_grid(g, true, true, &n_wg) && n_wg == 800);
        uint32_t c0, c1;
        slice_chunk_range(g, 2, 1, c0, c1);
        CHECK(c0 == 16 && c1 == 24);
        g = grid_case(10, 5, 24, 1, 16, 4, 100);       // ... the same rules for tail slices: 3 x 16 >= 24
        CHECK(!plan_kslice_grid(g, true, true, &n_wg));
        g = grid_case(10, 5, 64, 1, 0, 2, 0);          // tail slices without the residency they are cut by
        CHECK(!plan_kslice_grid(g, true, true, &n_wg));
        g = grid_case(1u << 25, 8, 64, 1, 0, 0, 0);    // 2^25 tiles x 8 lengths x 8 XCDs = 2^31 workgroups
        CHECK(!plan_kslice_grid(g, true, true, &n_wg));
        g = grid_case(1u << 25, 7, 64, 1, 0, 0, 0);
        CHECK(plan_kslice_grid(g, true, true, &n_wg) && n_wg == 7ull << 28);
    }
    {   // round priority up to 9/4 rounds: a round of 128 workgroups per XCD -> up to 288 per XCD
        Map g = grid_case(72, 4, 64, 1, 0, 0, 0, 128);   // 288
        CHECK(plan_kslice_grid(g, true, true, &n_wg) && g.round_size == 128);
        g = grid_case(73, 4, 64, 1, 0, 0, 0, 128);       // 292
        CHECK(plan_kslice_grid(g, true, true, &n_wg) && g.round_size == 0);
        g = grid_case(36, 4, 64, 2, 0, 0, 0, 128);       // slices count: 36 x 4 x 2 = 288
        CHECK(plan_kslice_grid(g, true, true, &n_wg) && g.round_size == 128);
        g = grid_case(37, 4, 64, 2, 0, 0, 0, 128);
        CHECK(plan_kslice_grid(g, true, true, &n_wg) && g.round_size == 0);
    }
    {   // tail slicing: 33 tiles x 5 lengths = 165 units per XCD, 100 resident: 100 whole units, then 65 units x 4 slices
        Map g = grid_case(33, 5, 64, 8, 0, 4, 100);
        CHECK(plan_kslice_grid(g, true, true, &n_wg) && g.tail_first == 100 && g.k_slices == 1 && n_wg == (100 + 65 * 4) * 8);
        // units of an XCD: blocks of 32 tiles x 5 lengths = 160, tile fastest; the last block has 1 tile
        expect_unit(g, 37, false, 5, 1, 0, 1, false);
        expect_unit(g, 99, false, 3, 3, 0, 1, false);
        expect_unit(g, 100, false, 4, 3, 0, 4, true);     // unit 100, slice 0
        expect_unit(g, 103, false, 4, 3, 3, 4, true);
        expect_unit(g, 354, false, 32, 3, 2, 4, true);    // 100 + 254: unit 100 + 63 = 163 = block 1 (one tile: slot 32), length 3; slice 254 % 4
        expect_unit(g, 359, false, 32, 4, 3, 4, true);    // the last workgroup: unit 164
        Map h = grid_case(33, 5, 64, 1, 0, 4, 1000);      // fewer units than resident slots: every unit sliced
        CHECK(plan_kslice_grid(h, true, true, &n_wg) && h.tail_first == 0 && n_wg == 165 * 4 * 8);
        h = grid_case(33, 5, 64, 1, 0, 4, 3);             // whole rounds exactly: no tail
        CHECK(plan_kslice_grid(h, true, true, &n_wg) && h.tail_first == 165 && n_wg == 165 * 8);
    }
    {   // uniform slices: a block is 32 tiles x 5 lengths x 2 slices = 320 workgroups, slice fastest after the tile
        Map g = grid_case(33, 5, 64, 2, 0, 0, 0);
        CHECK(plan_kslice_grid(g, true, true, &n_wg) && n_wg == 330 * 8);
        expect_unit(g, 100, false, 4, 1, 1, 2, false);    // 100 = 3 x 32 + 4: k slot 3 = length 1, slice 1
        expect_unit(g, 327, false, 32, 3, 1, 2, false);   // block 1 (one tile), k slot 7
        expect_unit(g, 640, true, 0, 0, 0, 0, false);     // block 2 of 33 tiles: no unit (far beyond the grid)
    }
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "pinned";
    if (!strcmp(what, "pinned")) pinned();
    else if (!strcmp(what, "tiles")) tiles();
    else if (!strcmp(what, "units")) units();
    else return 2;
    if (g_failed) printf("FAILED %ld of %ld\n", g_failed, g_checks);
    else printf("ok %ld\n", g_checks);
    return g_failed ? 1 : 0;
}
