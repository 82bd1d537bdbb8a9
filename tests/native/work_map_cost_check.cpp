// work_map_cost_check.cpp -- CPU check of the cost order of csrc/work_map.hpp: self-mode tiles dealt to the XCDs by cost, full
// tiles before half tiles (test infrastructure).  Host compiler only, the header alone, as work_map_check.cpp.
//   work_map_cost_check order  : n = 2 ... 700 x row bands x tile heights 16 / 32 x 1 / 2 / 4 / 8 XCDs x group spans 1 ... 4
//   work_map_cost_check pinned : the 1 000-genome launch the order was made for, by hand
//   work_map_cost_check rule   : which launches plan_pair_shape() (csrc/dense_plan.hpp) gives the order to
// Prints one line per failed check and "ok <checks>" / "FAILED <failures> of <checks>"; the exit status says which.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "../../sketchlib.rust_amd/csrc/dense_plan.hpp"
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
    uint32_t row_begin = 0, row_end = 0, self_mode = 1;
    uint32_t a_tiles = 0, n_jblocks = 0, n_active_tiles = 0, tiles_per_xcd = 0, xcd_interleave = 0, xcd_shift = 0;
    uint32_t n_groups = 0, group_span = 0, tile_rows = 0, group_cols = 0;
    const uint32_t *tile_prefix = nullptr;
    uint32_t inline_prefix_ok = 0, n_prefix_inline = 0, tile_prefix_inline[TILE_PREFIX_INLINE] = {};
    uint32_t slice_chunks = 0, k_slices = 0, tail_slices = 0, tail_first = 0, tail_resident = 0, round_size = 0;
    uint32_t n_full_tiles = 0;
};

static Map launch(uint32_t n, uint32_t r0, uint32_t r1, uint32_t span, uint32_t shift, bool inline_ok)
{
    Map g;
    g.nB = n;
    g.row_begin = r0;
    g.row_end = r1;
    g.group_span = span;
    g.xcd_shift = shift;
    g.inline_prefix_ok = inline_ok;
    return g;
}

static bool plan(Map &g, uint32_t R, bool by_cost, std::vector<uint32_t> &prefix, uint64_t *grid)
{
    plan_tile_geometry(g, R, 128u);
    prefix.assign(n_supergroups(g) + 1u, 0u);
    if (by_cost) CHECK(tile_cost_order_possible(g));
    if (!(by_cost ? plan_tile_numbering_by_cost(g, prefix.data(), grid) : plan_tile_numbering(g, prefix.data(), grid))) return false;
    if (g.n_prefix_inline == 0u) g.tile_prefix = prefix.data();
    return true;
}

// The cells (row tile, column group) that hold a pair i < j the launch owes, and of those the ones that hold one in each
// 64-column block -- pair by pair in effect: row i meets a block iff the block's last column below n lies right of i.
struct Cells {
    uint32_t a_tiles, n_groups;
    std::vector<uint8_t> need, full;
};
static Cells cells_of(uint32_t n, uint32_t r0, uint32_t r1, uint32_t R)
{
    Cells c;
    c.a_tiles = (r1 - r0 + R - 1) / R;
    c.n_groups = (n + 127u) / 128u;
    c.need.assign((size_t)c.a_tiles * c.n_groups, 0);
    c.full = c.need;
    std::vector<uint8_t> b0(c.need.size(), 0), b1(c.need.size(), 0);
    for (uint32_t i = r0; i < r1; ++i) {
        for (uint32_t jb = 0; jb * 64u < n; ++jb) {
            const uint32_t last = jb * 64u + 63u < n - 1u ? jb * 64u + 63u : n - 1u;
            if (last > i) (jb & 1u ? b1 : b0)[(size_t)((i - r0) / R) * c.n_groups + jb / 2u] = 1;
        }
    }
    for (size_t x = 0; x < c.need.size(); ++x) {
        c.need[x] = b0[x] | b1[x];
        c.full[x] = b0[x] & b1[x];
    }
    return c;
}

// The chunk-split grid over `slots` tile slots per XCD: every (slot, k index) is computed once whole or once per slice.  The
// decode does not see the XCD or the tile order, so one walk per (slots, lengths, slices, residency) stands for every launch.
static std::set<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>> g_units_seen;
static void units_exact(const Map &planned, uint32_t k_count, uint32_t S, uint32_t resident)
{
    if (!g_units_seen.insert(std::make_tuple(planned.tiles_per_xcd, k_count, S, resident)).second) return;
    Map g = planned;
    g.ss64 = 64;
    g.k_count = k_count;
    g.k_slices = 1;
    g.tail_slices = S;
    g.slice_chunks = 0;
    g.tail_resident = resident;
    uint64_t n_wg = 0;
    CHECK(plan_kslice_grid(g, true, true, &n_wg));
    CHECK(n_wg % (1u << g.xcd_shift) == 0);
    std::vector<uint32_t> seen((size_t)g.tiles_per_xcd * k_count, 0u);
    for (uint32_t s_idx = 0; s_idx < (uint32_t)(n_wg >> g.xcd_shift); ++s_idx) {
        const KsliceUnit u = kslice_unit(g, s_idx, true, true);
        CHECK(!u.none && u.slot < g.tiles_per_xcd && u.kk0 < k_count && u.slice < u.n_slices);
        if (u.none || u.slot >= g.tiles_per_xcd || u.kk0 >= k_count) continue;
        CHECK((seen[(size_t)u.slot * k_count + u.kk0] & (1u << u.slice)) == 0u);
        seen[(size_t)u.slot * k_count + u.kk0] |= 1u << u.slice;
        CHECK(u.n_slices == (s_idx >= g.tail_first ? S : 1u));
    }
    for (uint32_t v : seen) CHECK(v == 1u || v == (1u << S) - 1u);
}

// ... and the composition written out: every (active tile, k index) of the launch once whole or once per slice, over the whole grid
static void units_composed(const Map &planned, const Cells &c, uint32_t k_count, uint32_t S, uint32_t resident)
{
    Map g = planned;
    g.ss64 = 64;
    g.k_count = k_count;
    g.k_slices = 1;
    g.tail_slices = S;
    g.tail_resident = resident;
    uint64_t n_wg = 0;
    CHECK(plan_kslice_grid(g, true, true, &n_wg));
    std::vector<uint32_t> seen(c.need.size() * k_count, 0u);
    for (uint64_t b = 0; b < n_wg; ++b) {
        const uint32_t xcd = (uint32_t)b & ((1u << g.xcd_shift) - 1u), s_idx = (uint32_t)(b >> g.xcd_shift);
        const KsliceUnit u = kslice_unit(g, s_idx, true, true);
        uint32_t jg, at;
        if (u.none || !lookup_tile_by_cost_at(g, xcd, u.slot, jg, at)) continue;
        uint32_t &w = seen[((size_t)at * c.n_groups + jg) * k_count + u.kk0];
        CHECK((w & (1u << u.slice)) == 0u);
        w |= 1u << u.slice;
    }
    uint32_t tiles = 0;
    for (size_t x = 0; x < seen.size(); ++x) {
        CHECK(seen[x] == 0u || seen[x] == 1u || seen[x] == (1u << S) - 1u);
        tiles += seen[x] != 0u;
    }
    CHECK_EQ(tiles, g.n_active_tiles * k_count);
}

static void order_of_shape(uint32_t n, uint32_t r0, uint32_t r1, uint32_t R)
{
    const Cells c = cells_of(n, r0, r1, R);
    std::vector<uint32_t> prefix, prefix_old;
    std::vector<uint8_t> got(c.need.size());
    for (uint32_t span = 1; span <= 4; ++span) {
        // the present numbering restated: super-group by super-group, row tile by row tile, the groups that need it side by side
        std::vector<std::pair<uint32_t, uint32_t>> present;
        for (uint32_t first = 0; first < c.n_groups; first += span) {
            for (uint32_t at = 0; at < c.a_tiles; ++at) {
                for (uint32_t jg = first; jg < first + span && jg < c.n_groups; ++jg) {
                    const uint32_t a0 = r0 + at * R, last_col = (jg + 1u) * 128u - 1u;
                    if (a0 < last_col && a0 < r1) present.push_back({jg, at});
                }
            }
        }
        for (uint32_t shift = 0; shift <= 3; ++shift) {
            const uint32_t n_xcd = 1u << shift;
            {   // flag off: the present order, slot for slot
                Map g = launch(n, r0, r1, span, shift, ((n + shift) & 1u) != 0);
                uint64_t grid = 0;
                CHECK(plan(g, R, false, prefix_old, &grid));
                CHECK_EQ(g.n_active_tiles, present.size());
                CHECK_EQ(g.tiles_per_xcd, (present.size() + n_xcd - 1) / n_xcd);
                for (uint32_t xcd = 0; xcd < n_xcd; ++xcd) {
                    for (uint32_t slot = 0; slot <= g.tiles_per_xcd; ++slot) {
                        uint32_t jg = ~0u, at = ~0u;
                        const size_t t = (size_t)xcd * g.tiles_per_xcd + slot;
                        const bool yields = lookup_tile_at(g, xcd, slot, jg, at);
                        CHECK_EQ(yields, slot < g.tiles_per_xcd && t < present.size());
                        if (yields && t < present.size()) CHECK(jg == present[t].first && at == present[t].second);
                    }
                }
            }
            Map g = launch(n, r0, r1, span, shift, ((n + shift) & 1u) != 0);
            uint64_t grid = 0;
            CHECK(plan(g, R, true, prefix, &grid));
            CHECK_EQ(g.n_active_tiles, present.size());
            CHECK_EQ(grid, (uint64_t)g.tiles_per_xcd << shift);
            std::fill(got.begin(), got.end(), 0);
            uint32_t yielded = 0, slots_max = 0, full_min = ~0u, full_max = 0, half_min = ~0u, half_max = 0, cost_max = 0, cost_sum = 0;
            for (uint32_t xcd = 0; xcd < n_xcd; ++xcd) {
                uint32_t n_full = 0, n_half = 0, last_slot = 0;
                for (uint32_t slot = 0; slot <= g.tiles_per_xcd; ++slot) {
                    uint32_t jg = ~0u, at = ~0u;
                    if (!lookup_tile_by_cost_at(g, xcd, slot, jg, at)) continue;
                    ++yielded;
                    CHECK(slot < g.tiles_per_xcd && jg < c.n_groups && at < c.a_tiles);
                    if (jg >= c.n_groups || at >= c.a_tiles) continue;
                    CHECK_EQ(slot, n_full + n_half);                                   // the share is the first slots, no hole
                    last_slot = slot + 1u;
                    const size_t cell = (size_t)at * c.n_groups + jg;
                    CHECK_EQ(got[cell]++, 0);                                          // no tile twice
                    uint32_t fx = ~0u, fs = ~0u;
                    tile_slot_by_cost(g, jg, at, fx, fs);                              // inverse o forward = identity
                    CHECK(fx == xcd && fs == slot);
                    // the classes are the kernel's skip tests
                    const uint32_t a0 = r0 + at * R;
                    const bool half = tile_skips_block0(1u, a0, jg * 2u) || tile_skips_block1(jg * 2u, g.n_jblocks);
                    CHECK_EQ(!half, c.full[cell] != 0);                                // ... and say which tiles hold a pair in both blocks
                    CHECK(a0 < r1 && a0 < (jg + 1u) * 128u - 1u);                      // none of the kernel's defensive returns fires
                    if (half) ++n_half;
                    else {
                        ++n_full;
                        CHECK_EQ(n_half, 0);                                           // every full tile before every half tile
                    }
                }
                slots_max = last_slot > slots_max ? last_slot : slots_max;
                full_min = n_full < full_min ? n_full : full_min;
                full_max = n_full > full_max ? n_full : full_max;
                half_min = n_half < half_min ? n_half : half_min;
                half_max = n_half > half_max ? n_half : half_max;
                const uint32_t cost = 2u * n_full + n_half;                            // 64-column blocks walked
                cost_max = cost > cost_max ? cost : cost_max;
                cost_sum += cost;
            }
            CHECK_EQ(yielded, g.n_active_tiles);
            CHECK_EQ(g.tiles_per_xcd, slots_max);                                      // the grid is slots_max << xcd_shift
            for (size_t x = 0; x < c.need.size(); ++x) CHECK(!c.need[x] || got[x] == 1);   // every owed pair in exactly one tile
            CHECK(full_max - full_min <= 1u && half_max - half_min <= 1u);
            CHECK(cost_max * n_xcd <= cost_sum + 2u * n_xcd);                          // heaviest XCD <= mean + one full tile
            if (g.n_active_tiles == 0) continue;
            for (uint32_t S : {2u, 4u, 8u}) {
                for (uint32_t k_count = 2; k_count <= 5; ++k_count) {
                    for (uint32_t resident : {96u, 128u}) units_exact(g, k_count, S, resident);
                    if (n % 61u == 5u && span == 2u) units_composed(g, c, k_count, S, 128u);
                }
            }
        }
    }
}

static void order()
{
    for (uint32_t R : {16u, 32u}) {
        for (uint32_t n = 2; n <= 700; ++n) {
            order_of_shape(n, 0, n, R);
            order_of_shape(n, 0, n - 1, R);                                     // what the dense calls launch: the last sample owes nothing
            if (n > 90) order_of_shape(n, 37, n - 50, R);                       // a band in the middle of the triangle
            if (n > 12) order_of_shape(n, n / 3, 2 * n / 3, R);
            if (n > 300) order_of_shape(n, 127, 129 + n % 200, R);              // begins on a group's last column
            order_of_shape(n, n / 2, n / 2 + 1, R);                             // one row
        }
    }
}

static void pinned()
{
    // 1 000 genomes against themselves, rows [0, 999), 16 x 128 tiles, two groups side by side, 8 XCDs.  8 column groups, 16 blocks
    // of 64 columns (even: no group ends in block 0).  Group j holds the row tiles with first row < min(128 j + 127, 999):
    // 8, 16, 24, 32, 40, 48, 56, 63 = 287 tiles; its full ones have first row < 128 j + 63: 4, 12, 20, 28, 36, 44, 52, 60 = 256;
    // 31 half tiles: 4 per group, 3 in the last (rows end at 999, not at 1 023).
    std::vector<uint32_t> prefix;
    uint64_t grid = 0;
    Map g = launch(1000, 0, 999, 2, 3, true);
    CHECK(plan(g, 16, true, prefix, &grid));
    CHECK(g.n_groups == 8 && g.n_jblocks == 16 && g.n_active_tiles == 287 && g.n_full_tiles == 256);
    CHECK(g.tiles_per_xcd == 36 && grid == 288);                         // 32 full + 4 half (XCD 0: 3)
    CHECK(prefix[0] == 0 && prefix[1] == 16 && prefix[2] == 64 && prefix[3] == 144 && prefix[4] == 256 && g.n_prefix_inline == 5);
    uint32_t jg, at;
    CHECK(lookup_tile_by_cost_at(g, 0, 0, jg, at) && jg == 0 && at == 0);
    CHECK(lookup_tile_by_cost_at(g, 0, 16, jg, at) && jg == 2 && at == 0);    // full tile 16: the first of super-group 1
    CHECK(lookup_tile_by_cost_at(g, 7, 31, jg, at) && jg == 7 && at == 59);   // full tile 255, the last
    CHECK(lookup_tile_by_cost_at(g, 0, 32, jg, at) && jg == 0 && at == 4);    // half tile 0
    CHECK(lookup_tile_by_cost_at(g, 0, 34, jg, at) && jg == 0 && at == 6);    // half tile 2: XCD 0 takes 3 (31 = 7 x 4 + 3: the odd ones go last)
    CHECK(!lookup_tile_by_cost_at(g, 0, 35, jg, at));
    CHECK(lookup_tile_by_cost_at(g, 1, 32, jg, at) && jg == 0 && at == 7);    // half tile 3
    CHECK(lookup_tile_by_cost_at(g, 1, 33, jg, at) && jg == 1 && at == 12);   // half tile 4: group 1's first (12 full ones below it)
    CHECK(lookup_tile_by_cost_at(g, 7, 35, jg, at) && jg == 7 && at == 62);   // half tile 30: first row 992
    CHECK(!lookup_tile_by_cost_at(g, 7, 36, jg, at));
    for (uint32_t x = 0; x < 8; ++x) {   // every XCD: 64 blocks of full tiles + 3 or 4 of half tiles (the present order: 63 ... 72)
        const CostShare s = tile_cost_share(g, x);
        CHECK(s.n_full == 32 && s.n_half == (x == 0 ? 3u : 4u));
    }
    // 193 samples on 2 XCDs: blocks 0 ... 3 (block 3 holds column 192 alone), both groups can hold a full tile
    Map h = launch(193, 0, 192, 2, 1, true);
    CHECK(plan(h, 16, true, prefix, &grid));
    CHECK(h.n_groups == 2 && h.n_jblocks == 4 && n_full_groups(h) == 2);
    // 192 samples: 3 blocks, group 1's columns end in block 0: all of its tiles are half tiles.  Group 0: first rows < 127: 8
    // tiles, 4 of them full (< 63); group 1: first rows < 191: 12 tiles
    Map k = launch(192, 0, 191, 2, 1, true);
    CHECK(plan(k, 16, true, prefix, &grid));
    CHECK(k.n_groups == 2 && k.n_jblocks == 3 && n_full_groups(k) == 1);
    CHECK(k.n_active_tiles == 8 + 12 && k.n_full_tiles == 4 && k.tiles_per_xcd == 10 && grid == 20);   // 2 + 8 slots on each of 2 XCDs
    CHECK(lookup_tile_by_cost_at(k, 0, 2, jg, at) && jg == 0 && at == 4);     // half tile 0
    CHECK(lookup_tile_by_cost_at(k, 0, 6, jg, at) && jg == 1 && at == 0);     // half tile 4: the group that ends in block 0
    CHECK(lookup_tile_by_cost_at(k, 1, 9, jg, at) && jg == 1 && at == 11);    // half tile 15, the last
}

static void rule()
{
    PairLaunch a;   // cfg 2's counts launch: 999 rows of 1 000 samples against themselves, 2 of 5 lengths, 4 tail slices, 8 XCDs
    a.mode = PLAN_MODE_COUNTS;
    a.rows = 999;
    a.nB = 1000;
    a.k_count = 2;
    a.ss64 = 64;
    a.k_sliced = true;
    a.tail_slices = 4;
    CHECK(plan_pair_shape(a).tile_cost_order && plan_pair_shape(a).shape == 165);
    PairLaunch b = a;
    b.xcd_interleave = true;                       // block-by-block plans deal their tiles in turns
    CHECK(!plan_pair_shape(b).tile_cost_order);
    b = a;
    b.xcd_shift = 0;                               // one XCD: nothing to deal
    CHECK(!plan_pair_shape(b).tile_cost_order);
    b = a;
    b.self_mode = false;                           // cross mode: every tile costs the same
    CHECK(!plan_pair_shape(b).tile_cost_order);
    b = a;
    b.mode = PLAN_MODE_JACCARD;                    // single-k keys
    CHECK(!plan_pair_shape(b).tile_cost_order);
    b = a;
    b.knobs.half_tiles = false;                    // (A/B build) no half tiles walked: equal cost
    CHECK(!plan_pair_shape(b).tile_cost_order);
    b = a;
    b.knobs.tile_cost_order = 0;                   // SKL_TILE_COST_ORDER=0
    CHECK(!plan_pair_shape(b).tile_cost_order);
    b = a;
    b.rows = 2499;                                 // 2 500 samples: 3.1 M pairs, past the rule's bound; x 2 lengths < 8 Mi: 16-row tiles still
    b.nB = 2500;
    CHECK(plan_pair_shape(b).shape == 165 && !plan_pair_shape(b).tile_cost_order);
    b.knobs.tile_cost_order = 1;                   // SKL_TILE_COST_ORDER=1: wherever the form allows
    CHECK(plan_pair_shape(b).tile_cost_order);
    b.xcd_shift = 0;
    CHECK(!plan_pair_shape(b).tile_cost_order);
    b = a;
    b.rows = 15999;                                // 32-row tiles walk no half tiles
    b.nB = 16000;
    b.knobs.tile_cost_order = 1;
    CHECK(plan_pair_shape(b).shape == 325 && !plan_pair_shape(b).tile_cost_order);
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "pinned";
    if (!strcmp(what, "pinned")) pinned();
    else if (!strcmp(what, "order")) order();
    else if (!strcmp(what, "rule")) rule();
    else return 2;
    if (g_failed) printf("FAILED %ld of %ld\n", g_failed, g_checks);
    else printf("ok %ld\n", g_checks);
    return g_failed ? 1 : 0;
}
