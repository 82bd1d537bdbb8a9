// unit_table_check.cpp -- CPU check of csrc/unit_table.hpp: the host-built unit table of a k-sliced launch of the chunk-split
// kernel against the kernel's own decode of its workgroup index (test infrastructure).  Host compiler only, the headers alone, as
// work_map_check.cpp.  device_unit() below is the head of pair_kernel_kslice (pair_kslice.hip) RESTATED, return by return, in
// the kernel's order; the table is what unit_table.hpp composes from the functions of work_map.hpp.
//   unit_table_check table : every small shape -- entry b equals the decode of workgroup b field for field, `none` included; among
//                            the entries that are not none every (tile, k index, chunk slice) appears once, the slices of a (tile, k)
//                            partition the sketch, and every active tile has all its k indices
//   unit_table_check cache : the key and the cache -- same key hits, one field changed misses, the entry unused longest is evicted
// Prints one line per failed check and "ok <checks>" / "FAILED <failures> of <checks>"; the exit status says which.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sketchlib.rust_amd/csrc/unit_table.hpp"

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

// The fields of PairArgs (kernels.h) the map and the table read and write, under the same names.
struct Map {
    uint32_t nB = 0, ss64 = 64, k_count = 1;
    uint32_t row_begin = 0, row_end = 0, self_mode = 1;
    uint32_t a_tiles = 0, n_jblocks = 0, n_active_tiles = 0, tiles_per_xcd = 0, xcd_interleave = 0, xcd_shift = 0;
    uint32_t n_groups = 0, group_span = 0, tile_rows = 0, group_cols = 0;
    const uint32_t *tile_prefix = nullptr;
    uint32_t inline_prefix_ok = 0, n_prefix_inline = 0, tile_prefix_inline[TILE_PREFIX_INLINE] = {};
    uint32_t slice_chunks = 0, k_slices = 0, tail_slices = 0, tail_first = 0, tail_resident = 0, round_size = 0;
    uint32_t tile_cost_order = 0, n_full_tiles = 0, no_half_tiles = 0;
    const uint8_t *block_ke = nullptr;
    uint32_t blk_shift_r = 0, blk_shift_c = 0, blk_cols = 0;
};

// What the kernel's head leaves the walk: pair_kslice.hip from `blockIdx -> (XCD, slot ...` to the choice of the walk's case.
struct DeviceUnit {
    bool none = true;
    uint32_t a0 = 0, jb0 = 0, kk0 = 0, slice = 0, c_begin = 0, c_end = 0, walk = 0, prio = 0;
    bool plane1 = false;
};
static DeviceUnit device_unit(const Map &g, uint32_t block_idx, uint32_t R, bool counts)
{
    DeviceUnit out;
    const uint32_t JL = 2;
    const uint32_t xcd = block_idx & ((1u << g.xcd_shift) - 1u), s_idx = block_idx >> g.xcd_shift;
    const KsliceUnit unit = kslice_unit(g, s_idx, true, counts);
    if (unit.none) return out;
    const bool tail_mode = unit.tail_mode, in_tail = unit.in_tail;
    const uint32_t slot = unit.slot, kk0 = unit.kk0, slice = unit.slice, n_slices = unit.n_slices;
    uint32_t prio = 0;
    if (!tail_mode && g.round_size != 0u) {
        const uint32_t round_ = s_idx / g.round_size;
        if (round_ == 1u) prio = 1;
        else if (round_ == 2u) prio = 2;
        else if (round_ >= 3u) prio = 3;
    }
    uint32_t c_begin, c_end;
    slice_chunk_range(g, n_slices, slice, c_begin, c_end);
    uint32_t jg, at;
    const bool COST_ORDER = counts && R == 16;
    if (COST_ORDER && g.tile_cost_order != 0u) {
        if (!lookup_tile_by_cost_at(g, xcd, slot, jg, at)) return out;
    } else if (!lookup_tile_at(g, xcd, slot, jg, at)) {
        return out;
    }
    const uint32_t jb0 = jg * JL;
    const uint32_t a0 = g.row_begin + at * R;
    if (jb0 >= g.n_jblocks) return out;
    if (a0 >= g.row_end) return out;
    if (g.self_mode && a0 >= (jg + 1u) * JL * 64u - 1u) return out;
    if (counts) {
        if (g.block_ke != nullptr) {
            const uint32_t r_last = (a0 + R < g.row_end ? a0 + R : g.row_end) - 1u;
            const uint32_t bc = (jb0 * 64u) >> g.blk_shift_c;
            const uint32_t ke_a = g.block_ke[(size_t)(a0 >> g.blk_shift_r) * g.blk_cols + bc];
            const uint32_t ke_b = g.block_ke[(size_t)(r_last >> g.blk_shift_r) * g.blk_cols + bc];
            if (kk0 >= (ke_a > ke_b ? ke_a : ke_b)) return out;
        }
    }
    const bool half_ok = R == 16 && g.no_half_tiles == 0u;
    const bool skip0 = half_ok && tile_skips_block0(g.self_mode, a0, jb0);
    const bool skip1 = half_ok && tile_skips_block1(jb0, g.n_jblocks);
    out.none = false;
    out.a0 = a0;
    out.jb0 = jb0;
    out.kk0 = kk0;
    out.slice = slice;
    out.c_begin = c_begin;
    out.c_end = c_end;
    out.walk = skip0 ? 1u : skip1 ? 2u : 0u;   // the walk's blocks: 1-2, 0-1, 0-2
    out.prio = prio;
    out.plane1 = in_tail && slice != 0u;
    return out;
}

struct Shape {
    uint32_t n, r0, r1;
    bool self;
    uint32_t R, span, shift, k_count, tail, k_slices;
    bool cost, counts, inline_ok, mixed, interleave;
};

static long g_launches = 0, g_none = 0, g_entries = 0;

static void check_shape(const Shape &s)
{
    Map g;
    g.nB = s.n;
    g.row_begin = s.r0;
    g.row_end = s.r1;
    g.self_mode = s.self;
    g.group_span = s.span;
    g.xcd_shift = s.shift;
    g.xcd_interleave = s.interleave;
    g.inline_prefix_ok = s.inline_ok;
    g.k_count = s.k_count;
    g.ss64 = 64;
    g.tail_slices = s.tail;
    g.k_slices = s.k_slices;
    g.tail_resident = s.R == 16 ? 128u : 96u;
    g.round_size = g.tail_resident;
    const uint32_t S = s.tail > 1u ? s.tail : s.k_slices;
    if (s.counts && S > 1u && S < 8u && s.n % 7u == 0u) {   // an uneven cut: 56 chunks in slices of 32 / 16, the last one short
        g.ss64 = 56;
        g.slice_chunks = S == 2u ? 32u : 16u;
        if ((uint64_t)g.slice_chunks * (S - 1u) >= g.ss64 || (uint64_t)g.slice_chunks * S < g.ss64) {
            g.ss64 = 64;
            g.slice_chunks = 0;
        }
    }
    plan_tile_geometry(g, s.R, 128u);
    std::vector<uint32_t> prefix(n_supergroups(g) + 1u, 0u);
    g.tile_cost_order = s.cost && s.counts && s.R == 16u && tile_cost_order_possible(g) ? 1u : 0u;   // (what the launcher and plan_tiles leave of the request)
    uint64_t grid = 0, n_wg = 0;
    if (!(g.tile_cost_order ? plan_tile_numbering_by_cost(g, prefix.data(), &grid) : plan_tile_numbering(g, prefix.data(), &grid))) return;
    if (grid == 0) return;
    if (g.self_mode && g.n_prefix_inline == 0u) g.tile_prefix = prefix.data();
    if (!plan_kslice_grid(g, true, s.counts, &n_wg)) return;
    std::vector<uint8_t> ke;
    if (s.mixed) {   // blocks of 256 sample ids, two different values: every length, or one fewer
        g.blk_shift_r = g.blk_shift_c = 8;
        g.blk_cols = (s.n + 255u) / 256u;
        ke.assign((size_t)g.blk_cols * g.blk_cols, 0);
        for (uint32_t r = 0; r < g.blk_cols; ++r) {
            for (uint32_t c = 0; c < g.blk_cols; ++c) ke[(size_t)r * g.blk_cols + c] = (uint8_t)((r + c) & 1u ? s.k_count : s.k_count - 1u);
        }
        g.block_ke = ke.data();
    }
    CHECK(unit_table_fits(g, n_wg));
    if (!unit_table_fits(g, n_wg)) return;
    ++g_launches;
    std::vector<UnitDesc> table(n_wg);
    build_unit_table(g, s.R, s.counts, g.block_ke, n_wg, table.data());
    // (tile, k index) -> chunks covered, slices seen
    const uint32_t slices_max = g.tail_slices > 1u ? g.tail_slices : g.k_slices;
    std::vector<uint32_t> chunks((size_t)g.a_tiles * g.n_groups * g.k_count, 0u), seen(chunks.size(), 0u);
    for (uint64_t b = 0; b < n_wg; ++b) {
        const UnitDesc &d = table[b];
        const DeviceUnit u = device_unit(g, (uint32_t)b, s.R, s.counts);
        CHECK_EQ(unit_none(d), u.none);
        if (u.none || unit_none(d)) {
            ++g_none;
            continue;
        }
        ++g_entries;
        CHECK(d.a0 == u.a0 && unit_jb0(d) == u.jb0 && unit_kk0(d) == u.kk0 && unit_slice(d) == u.slice);
        CHECK(unit_c_begin(d) == u.c_begin && unit_c_end(d) == u.c_end);
        CHECK(unit_walk(d) == u.walk && unit_plane1(d) == u.plane1 && unit_prio(d) == u.prio);
        CHECK(u.c_begin < u.c_end && u.c_end <= g.ss64 && u.slice < slices_max && u.kk0 < g.k_count);
        const size_t cell = ((size_t)((u.a0 - g.row_begin) / s.R) * g.n_groups + u.jb0 / 2u) * g.k_count + u.kk0;
        CHECK(cell < chunks.size());
        if (cell >= chunks.size()) continue;
        CHECK((seen[cell] & (1u << u.slice)) == 0u);   // every (tile, k, slice) once
        seen[cell] |= 1u << u.slice;
        chunks[cell] += u.c_end - u.c_begin;
    }
    if (!s.mixed) {   // (a per-block plan drops k indices on purpose)
        uint32_t units = 0;
        for (size_t x = 0; x < chunks.size(); ++x) {
            CHECK(chunks[x] == 0u || chunks[x] == g.ss64);   // whole, or slices that partition the sketch
            units += chunks[x] != 0u;
        }
        CHECK_EQ(units, (uint64_t)g.n_active_tiles * g.k_count);
    } else {
        for (size_t x = 0; x < chunks.size(); ++x) CHECK(chunks[x] == 0u || chunks[x] == g.ss64);
    }
}

static const uint32_t TAILS[3] = {0u, 4u, 8u};

static void bands_of(uint32_t n, bool self, uint32_t (*bands)[2], int *n_bands)
{
    int m = 0;
    if (self) {
        bands[m][0] = 0, bands[m++][1] = n - 1u;                          // what the dense calls launch
        if (n > 90u) bands[m][0] = 37u, bands[m++][1] = n - 50u;          // a band in the middle of the triangle
        bands[m][0] = n / 2u, bands[m++][1] = n / 2u + 1u;                // one row
        if (bands[m - 1][1] > n - 1u && n > 2u) --m;
    } else {
        const uint32_t nA = n / 2u + 3u;                                  // cross mode: nA != nB
        bands[m][0] = 0, bands[m++][1] = nA;
        if (nA > 40u) bands[m][0] = 37u, bands[m++][1] = nA - 1u;
        bands[m][0] = nA / 2u, bands[m++][1] = nA / 2u + 1u;
    }
    *n_bands = m;
}

static void table()
{
    // Every n = 2 ... 700 (the steps of work_map_cost_check), both modes, its row bands, both tile heights, 1 / 2 / 4 / 8 XCDs; the
    // other axes -- lengths 1 ... 5, tail slices 0 / 4 / 8, uniform slices 1 / 2, cost order, group span, inline prefix -- go
    // round with n and the XCD count, coprime periods, so that every pair of values meets many times ...
    for (uint32_t n = 2; n <= 700; ++n) {
        for (int self = 1; self >= 0; --self) {
            uint32_t bands[3][2];
            int n_bands = 0;
            bands_of(n, self != 0, bands, &n_bands);
            for (int bi = 0; bi < n_bands; ++bi) {
                for (uint32_t R : {16u, 32u}) {
                    for (uint32_t shift = 0; shift <= 3; ++shift) {
                        Shape s;
                        s.n = n, s.r0 = bands[bi][0], s.r1 = bands[bi][1], s.self = self != 0, s.R = R, s.shift = shift;
                        s.span = 1u + (n + shift) % 3u;
                        s.k_count = 1u + (n + shift) % 5u;
                        s.tail = TAILS[(n / 5u + shift + (uint32_t)bi) % 3u];
                        s.k_slices = 1u + ((n / 3u + shift) & 1u);
                        s.cost = ((n / 2u + shift + R / 16u) & 1u) != 0;
                        s.counts = true;
                        s.inline_ok = ((n + shift) & 1u) != 0;
                        s.mixed = false;
                        s.interleave = false;
                        check_shape(s);
                        s.counts = false;   // the single-k form: one length, no slices (plan_kslice_grid drops them)
                        s.k_count = 1;
                        check_shape(s);
                        if (n >= 257u && n % 4u == 1u && bi < 2) {   // the early break decided per block: two values, tiles dealt in turns
                            s.counts = true;
                            s.k_count = 2u + (n + shift) % 4u;
                            s.mixed = true;
                            s.interleave = true;
                            s.cost = false;
                            check_shape(s);
                        }
                    }
                }
            }
        }
    }
    // ... and the full product of them at the sizes the GPU test runs, self mode and cross
    for (uint32_t n : {2u, 17u, 65u, 129u, 193u, 257u, 413u, 700u}) {
        for (int self = 1; self >= 0; --self) {
            uint32_t bands[3][2];
            int n_bands = 0;
            bands_of(n, self != 0, bands, &n_bands);
            for (int bi = 0; bi < n_bands; ++bi) {
                for (uint32_t R : {16u, 32u}) {
                    for (uint32_t shift = 0; shift <= 3; ++shift) {
                        for (uint32_t k_count = 1; k_count <= 5; ++k_count) {
                            for (uint32_t tail : TAILS) {
                                for (uint32_t k_slices = 1; k_slices <= 2; ++k_slices) {
                                    for (int cost = 0; cost <= 1; ++cost) {
                                        Shape s;
                                        s.n = n, s.r0 = bands[bi][0], s.r1 = bands[bi][1], s.self = self != 0, s.R = R, s.shift = shift;
                                        s.span = 2;
                                        s.k_count = k_count;
                                        s.tail = tail;
                                        s.k_slices = k_slices;
                                        s.cost = cost != 0;
                                        s.counts = true;
                                        s.inline_ok = true;
                                        s.mixed = n >= 257u && k_count >= 2u && cost == 0 && k_slices == 1u;
                                        s.interleave = s.mixed;
                                        check_shape(s);
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    CHECK(g_launches > 50000 && g_none > 1000 && g_entries > 10000000);
    printf("launches %ld, entries %ld, of them none %ld\n", g_launches, g_entries + g_none, g_none);
    // cfg 2 by hand: 1 000 samples, rows [0, 999), 2 lengths, 4 tail slices, 8 XCDs, cost order: 36 slots x 2 lengths per XCD, all
    // in the tail (72 < 128 resident) -> 72 x 4 slices x 8 XCDs = 2 304 workgroups; 287 tiles x 2 x 4 = 2 296 entries, 8 none
    {
        Map g;
        g.nB = 1000, g.row_end = 999, g.group_span = 2, g.xcd_shift = 3, g.inline_prefix_ok = 1, g.k_count = 2, g.tail_slices = 4, g.tail_resident = 128;
        g.tile_cost_order = 1;
        plan_tile_geometry(g, 16, 128);
        std::vector<uint32_t> prefix(n_supergroups(g) + 1u, 0u);
        uint64_t grid = 0, n_wg = 0;
        CHECK(plan_tile_numbering_by_cost(g, prefix.data(), &grid) && plan_kslice_grid(g, true, true, &n_wg));
        CHECK_EQ(n_wg, 2304);
        std::vector<UnitDesc> t(n_wg);
        build_unit_table(g, 16, true, nullptr, n_wg, t.data());
        long none = 0, plane1 = 0, half = 0;
        for (const UnitDesc &d : t) {
            none += unit_none(d);
            plane1 += !unit_none(d) && unit_plane1(d);
            half += !unit_none(d) && unit_walk(d) != UNIT_WALK_BOTH;
        }
        CHECK_EQ(none, 8);
        CHECK_EQ(plane1, 287 * 2 * 3);
        CHECK_EQ(half, 31 * 2 * 4);
        // workgroup 0: XCD 0, unit 0 = slot 0, k index 0, slice 0 of 4: tile (0, group 0), chunks [0, 16)
        CHECK(t[0].a0 == 0 && unit_jb0(t[0]) == 0 && unit_kk0(t[0]) == 0 && unit_slice(t[0]) == 0 && unit_c_begin(t[0]) == 0 && unit_c_end(t[0]) == 16);
        // workgroup 8 x 3: XCD 0, slice 3 of the same unit: chunks [48, 64), adds into plane 1
        CHECK(t[24].a0 == 0 && unit_slice(t[24]) == 3 && unit_c_begin(t[24]) == 48 && unit_c_end(t[24]) == 64 && unit_plane1(t[24]));
    }
}

static void cache()
{
    Map g;
    g.nB = 1000, g.row_end = 999, g.group_span = 2, g.xcd_shift = 3, g.inline_prefix_ok = 1, g.k_count = 2, g.tail_slices = 4, g.tail_resident = 128, g.tile_cost_order = 1;
    plan_tile_geometry(g, 16, 128);
    std::vector<uint32_t> prefix(n_supergroups(g) + 1u, 0u);
    uint64_t grid = 0, n_wg = 0;
    CHECK(plan_tile_numbering_by_cost(g, prefix.data(), &grid) && plan_kslice_grid(g, true, true, &n_wg));
    const UnitKey base = unit_key(g, 16, true, nullptr, 0, n_wg);
    CHECK(base == unit_key(g, 16, true, nullptr, 0, n_wg));
    // one field changed at a time: a different key
    std::vector<UnitKey> others;
    others.push_back(unit_key(g, 32, true, nullptr, 0, n_wg));
    others.push_back(unit_key(g, 16, false, nullptr, 0, n_wg));
    others.push_back(unit_key(g, 16, true, nullptr, 0, n_wg + 8));
#define CHANGED(field, value)                                      \
    do {                                                           \
        Map h = g;                                                 \
        h.field = value;                                           \
        others.push_back(unit_key(h, 16, true, nullptr, 0, n_wg)); \
    } while (0)
    CHANGED(row_begin, 16);
    CHANGED(row_end, 998);
    CHANGED(nB, 1001);
    CHANGED(self_mode, 0);
    CHANGED(k_count, 3);
    CHANGED(ss64, 128);
    CHANGED(xcd_shift, 2);
    CHANGED(xcd_interleave, 1);
    CHANGED(group_span, 1);
    CHANGED(n_groups, 9);
    CHANGED(tile_rows, 32);
    CHANGED(group_cols, 64);
    CHANGED(a_tiles, 64);
    CHANGED(n_jblocks, 17);
    CHANGED(n_active_tiles, 288);
    CHANGED(tiles_per_xcd, 37);
    CHANGED(tile_cost_order, 0);
    CHANGED(n_full_tiles, 255);
    CHANGED(k_slices, 2);
    CHANGED(slice_chunks, 16);
    CHANGED(tail_slices, 8);
    CHANGED(tail_first, 128);
    CHANGED(round_size, 128);
    CHANGED(no_half_tiles, 1);
    CHANGED(n_prefix_inline, 0);
#undef CHANGED
    const uint8_t ke_a[4] = {2, 3, 3, 2}, ke_b[4] = {2, 3, 2, 2};
    {
        Map h = g;
        h.blk_shift_r = h.blk_shift_c = 9, h.blk_cols = 2;
        others.push_back(unit_key(h, 16, true, ke_a, 4, n_wg));
        others.push_back(unit_key(h, 16, true, ke_b, 4, n_wg));        // the same geometry, one block's value changed
        h.blk_shift_c = 8;
        others.push_back(unit_key(h, 16, true, ke_a, 4, n_wg));
    }
    for (size_t x = 0; x < others.size(); ++x) {
        CHECK(!(others[x] == base));
        for (size_t y = 0; y < x; ++y) CHECK(!(others[x] == others[y]));
    }
    // the cache: 4 entries
    UnitCache c;
    bool hit = true;
    const int e0 = c.lookup(base, &hit);
    CHECK(!hit && e0 >= 0 && e0 < UNIT_CACHE_ENTRIES);
    CHECK(c.lookup(base, &hit) == e0 && hit);                          // the same key hits
    const int e1 = c.lookup(others[0], &hit);
    CHECK(!hit && e1 != e0);                                           // a changed key misses and takes an empty entry
    const int e2 = c.lookup(others[1], &hit);
    const int e3 = c.lookup(others[2], &hit);
    CHECK(!hit && e2 != e0 && e2 != e1 && e3 != e0 && e3 != e1 && e3 != e2);
    CHECK(c.lookup(base, &hit) == e0 && hit);                          // four shapes in turn: all kept
    CHECK(c.lookup(others[0], &hit) == e1 && hit);
    const int e4 = c.lookup(others[3], &hit);                          // a fifth: the entry unused longest goes (others[1])
    CHECK(!hit && e4 == e2);
    CHECK(c.lookup(others[3], &hit) == e4 && hit);                     // eviction keeps the newest
    CHECK(c.lookup(base, &hit) == e0 && hit);
    CHECK(c.lookup(others[0], &hit) == e1 && hit);
    CHECK(c.lookup(others[2], &hit) == e3 && hit);
    const int e5 = c.lookup(others[1], &hit);                          // the evicted shape again: a miss, built anew
    CHECK(!hit && e5 == e4);                                           // (others[3] was then the one unused longest)
    c.drop(e5);                                                        // a fill that failed leaves nothing behind
    CHECK(c.lookup(others[1], &hit) == e5 && !hit);
    CHECK_EQ(c.hits, 7);
    CHECK_EQ(c.builds, 7);
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "cache";
    if (!strcmp(what, "table")) table();
    else if (!strcmp(what, "cache")) cache();
    else return 2;
    if (g_failed) printf("FAILED %ld of %ld\n", g_failed, g_checks);
    else printf("ok %ld\n", g_checks);
    return g_failed ? 1 : 0;
}
