// eb_stripes_check.cpp -- CPU check of csrc/eb_stripes.hpp, the striped order of the early-break epilogue (test infrastructure).
// Host compiler only: no HIP header, no device, the library is never loaded.
//   eb_stripes_check map     : forward against inverse over every small shape -- every pair of a launch is owned by exactly one
//                              (workgroup, thread), at its index in the launch; a workgroup stays inside its XCD's two stripes;
//                              a wave's pairs are consecutive; the grid is what the forward side says
//   eb_stripes_check balance : self mode, n = 1 000 on 8 XCDs: the pairs each XCD holds
//   eb_stripes_check rule    : dense_plan.hpp counts_striped through plan_counts_launch, cases derived BY HAND
// Prints one line per failed check and "ok <checks>" / "FAILED <failures> of <checks>"; the exit status says which.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../sketchlib.rust_amd/csrc/dense_plan.hpp"
#include "../../sketchlib.rust_amd/csrc/eb_stripes.hpp"

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

// the fields of EpilogueArgs (kernels.h) the map reads and writes
struct Launch {
    uint32_t self_mode = 1, row_begin = 0, row_end = 0, nB_cols = 0, xcd_shift = 3;
    uint32_t stripe_w = 0, stripe_rp = 0;
};

// One launch: rows [r0, r1) against n_cols columns.  per_xcd (may be null): pairs each XCD holds.
static void check_launch(bool self_mode, uint32_t n_cols, uint32_t r0, uint32_t r1, uint32_t xcd_shift, uint64_t *per_xcd)
{
    Launch g;
    g.self_mode = self_mode ? 1u : 0u;
    g.row_begin = r0;
    g.row_end = r1;
    g.nB_cols = n_cols;
    g.xcd_shift = xcd_shift;
    const uint64_t n_pairs = self_mode ? self_rows_pairs(r0, r1, n_cols) : (uint64_t)(r1 - r0) * n_cols;
    const uint64_t out_base = self_mode ? cond_index(r0, r0 + 1, n_cols) : (uint64_t)r0 * n_cols;
    const uint64_t grid = plan_eb_stripes(g);
    const uint32_t n_xcd = 1u << xcd_shift;
    // the forward side, said again: W = 64 ceil(n_cols / (128 X)), two rows per workgroup, one slot per (row pair, block)
    const uint32_t w_expected = 64u * ((n_cols + 128u * n_xcd - 1u) / (128u * n_xcd));
    CHECK_EQ(g.stripe_w, w_expected);
    CHECK_EQ(grid, (uint64_t)((r1 - r0 + 1u) / 2u) * (w_expected / 64u) * n_xcd);
    CHECK((uint64_t)2u * n_xcd * g.stripe_w >= n_cols);   // the stripes cover every column
    std::vector<uint8_t> owners(n_pairs, 0);
    uint64_t tally[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t wg = 0; wg < grid + 2ull * n_xcd * (g.stripe_w / 64u); ++wg) {
        const EbStripeWg w = eb_stripe_wg(g, (uint32_t)wg);
        if (wg >= grid) {   // past the grid: nothing
            CHECK(w.none);
            continue;
        }
        CHECK_EQ(w.xcd, wg % n_xcd);
        uint32_t held = 0;
        for (uint32_t wave = 0; wave < 4u; ++wave) {
            uint64_t p_prev = 0;
            bool have_prev = false;
            for (uint32_t lane = 0; lane < 64u; ++lane) {
                uint32_t i = 0, j = 0;
                if (!eb_stripe_pair(g, w, wave * 64u + lane, i, j)) {
                    CHECK(!have_prev || j >= n_cols);   // (a wave's pairs are one run: nothing invalid between two valid lanes)
                    continue;
                }
                ++held;
                CHECK(i >= r0 && i < r1 && j < n_cols && (!self_mode || j > i));
                CHECK(i == w.i0 || i == w.i0 + 1u);
                const uint32_t stripe = j / g.stripe_w;
                CHECK(stripe == w.xcd || stripe == 2u * n_xcd - 1u - w.xcd);
                const uint64_t at = (self_mode ? cond_index(i, j, n_cols) : (uint64_t)i * n_cols + j) - out_base;
                CHECK(at < n_pairs);
                if (at < n_pairs) ++owners[at];
                if (have_prev) CHECK_EQ(at, p_prev + 1u);   // consecutive in the counts and in the output
                p_prev = at;
                have_prev = true;
                ++tally[w.xcd];
                if (per_xcd) ++per_xcd[w.xcd];
            }
        }
        CHECK_EQ(w.none, held == 0u);   // a workgroup leaves exactly when it holds no pair
    }
    uint64_t wrong = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) wrong += owners[p] != 1u;
    CHECK_EQ(wrong, 0);
    // the balance the rule reads (closed form) against the pairs counted here
    if (n_pairs != 0) {
        uint64_t heaviest = 0;
        for (uint32_t x = 0; x < n_xcd; ++x) heaviest = std::max(heaviest, tally[x]);
        const double counted = (double)heaviest * (double)n_xcd / (double)n_pairs;
        const double said = eb_stripe_imbalance(self_mode, n_cols, r0, std::min<uint64_t>(r1, self_mode ? n_cols - 1u : r1), xcd_shift);
        CHECK(said > counted - 1e-9 && said < counted + 1e-9);
    }
}

static void map()
{
    std::mt19937_64 rng(0x57121BE5);
    for (uint32_t xs = 0; xs <= 3u; ++xs) {
        for (uint32_t n = 2; n <= 300u; ++n) {
            check_launch(true, n, 0, n - 1u, xs, nullptr);
            if (n <= 40u) {   // every row band
                for (uint32_t r0 = 0; r0 + 1u < n; ++r0)
                    for (uint32_t r1 = r0 + 1u; r1 <= n; ++r1) check_launch(true, n, r0, r1, xs, nullptr);
            } else {
                for (int s = 0; s < 2; ++s) {
                    const uint32_t r0 = (uint32_t)(rng() % (n - 1u)), r1 = r0 + 1u + (uint32_t)(rng() % (n - 1u - r0));
                    check_launch(true, n, r0, r1, xs, nullptr);
                }
            }
        }
        check_launch(true, 1000, 0, 999, xs, nullptr);
        check_launch(true, 1000, 1, 995, xs, nullptr);
        check_launch(true, 1000, 2, 995, xs, nullptr);
        const uint32_t rows[] = {1, 2, 3, 70};
        for (uint32_t r : rows)
            for (uint32_t cols = 1; cols <= 300u; ++cols) {
                const uint32_t r0 = (uint32_t)(rng() % 3u);
                check_launch(false, cols, r0, r0 + r, xs, nullptr);
            }
    }
}

static void balance()
{
    uint64_t per_xcd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    check_launch(true, 1000, 0, 999, 3, per_xcd);
    // stripe s of width 64 holds 4 096 s + 2 016 pairs: stripes x and 15 - x sum to 65 472; the last stripe has 40 columns
    // (960 ... 999: 39 180 pairs instead of 63 456), so XCD 0 holds 2 016 + 39 180 = 41 196
    uint64_t total = 0, heaviest = 0;
    for (int x = 0; x < 8; ++x) {
        CHECK_EQ(per_xcd[x], x == 0 ? 41196 : 65472);
        total += per_xcd[x];
        heaviest = std::max(heaviest, per_xcd[x]);
    }
    CHECK_EQ(total, 499500);
    CHECK((double)heaviest <= 1.05 * ((double)total / 8.0));   // 65 472 / 62 437.5 = 1.049
    CHECK_EQ(eb_stripe_width(1000, 3), 64);
    CHECK_EQ(eb_stripe_width(1024, 3), 64);
    CHECK_EQ(eb_stripe_width(1025, 3), 128);
    CHECK_EQ(eb_stripe_width(1000, 0), 512);
    CHECK_EQ(eb_stripe_slice_bytes(1000, 3, 64), 917504);   // 2 x 64 columns x 64 chunks x 112 bytes
}

// An MI355X as one device, default switches, 4 096 bins, 5 k-mer lengths, all-vs-all of n samples (as dense_plan_check.cpp)
static DenseCall self_call(uint64_t n)
{
    DenseCall c;
    c.mode = PLAN_MODE_COREACC;
    c.self_mode = true;
    c.n_cols = n;
    c.r0 = 0;
    c.r1 = n - 1;
    c.nk = 5;
    c.ss64 = 64;
    c.min_alive = 9;
    return c;
}
static void early_break(DenseCall &c, int lengths, double alive_share, bool mixed = false)
{
    c.eb_plan = true;
    c.eb_lengths = lengths;
    c.eb_alive_share = alive_share;
    c.eb_mixed = mixed;
}
static CountsLaunch whole(const DenseCall &c) { return plan_counts_launch(c, c.r0, c.r1); }

static void rule()
{
    {   // cfg 2: 1 000 genomes, 2 of 5 lengths, 4.8 % of the sampled pairs still in the running: rows staged; 8 XCDs, W = 64:
        // 2 x 64 x 64 x 112 = 917 504 bytes <= 8 MiB; the heaviest XCD at 1.049 x the mean <= 1.3
        DenseCall c = self_call(1000);
        early_break(c, 2, 0.048);
        const CountsLaunch L = whole(c);
        CHECK(L.early && L.lean && L.lds_rows && !L.blocked);
        CHECK(L.striped);
        // everything else as at 1.1 % (dense_plan_check.cpp): the order changes nothing about the counts
        CHECK(L.tail && L.tail_slices == 4 && L.planes == 2 && L.plane_bytes == 3996000 && !L.cnt_u16);
        early_break(c, 2, 0.011);            // 1.1 % < 3 %: no rows staged, no stripes
        CHECK(!whole(c).lds_rows && !whole(c).striped);
        early_break(c, 2, 0.048);
        c.knobs.eb_stripes = 0;              // SKL_EB_STRIPES=0
        CHECK(!whole(c).striped && whole(c).lds_rows);
        c.knobs.eb_stripes = -1;
        c.knobs.xcds = 1;                    // one XCD is asked for every slice whatever the order
        CHECK(!whole(c).striped);
        c.knobs.eb_stripes = 1;              // forced
        CHECK(whole(c).striped);
    }
    {   // the balance (heaviest XCD over the mean, at most 1.3), 8 XCDs.  W = 128 from 1 025 to 2 048 columns: at n = 1 500 stripes
        // 12 ... 15 are empty, XCDs 0 ... 3 hold stripes 0 ... 3 alone: 1.86; n = 1 800: 1.29; n = 2 000: 1.05; n = 2 049: W = 192, 2.25
        const struct { uint64_t n; bool striped; } cases[] = {{1100, false}, {1500, false}, {1800, true}, {1900, true}, {2000, true},
                                                             {2049, false}, {2700, true}, {3000, true}, {3500, false}, {4000, true},
                                                             {5000, true}, {8000, true}};
        for (const auto &k : cases) {
            DenseCall c = self_call(k.n);
            early_break(c, 2, 0.048);
            CHECK(whole(c).lds_rows);
            CHECK_EQ(whole(c).striped, k.striped);
            c.knobs.eb_stripes = 1;
            CHECK(whole(c).striped);
        }
        CHECK(eb_stripe_imbalance(true, 1500, 0, 1499, 3) > 1.86 && eb_stripe_imbalance(true, 1500, 0, 1499, 3) < 1.87);
        CHECK(eb_stripe_imbalance(true, 1000, 0, 999, 3) > 1.048 && eb_stripe_imbalance(true, 1000, 0, 999, 3) < 1.049);
        CHECK(eb_stripe_imbalance(false, 1024, 0, 100, 3) == 1.0);
        CHECK(eb_stripe_imbalance(false, 130, 0, 520, 3) > 3.9);   // 64 of 130 columns on one XCD: 64 / 16.25
        // the bytes: n = 8 000 -> W = 512: 2 x 512 x 64 x 112 = 7 340 032 <= 8 388 608; n = 9 000 -> W = 576: 8 257 536 <= 8 388 608, but
        // n = 9 216 = 16 x 576 is as balanced as can be and 40 Mi pairs: still taken; W = 640 (n = 10 000: 9 175 040 bytes) is not
        DenseCall c = self_call(9216);
        early_break(c, 2, 0.048);
        CHECK(whole(c).striped);
        c = self_call(10000);
        early_break(c, 2, 0.048);           // (49 995 000 pairs < 48 Mi = 50 331 648: not yet the blocked order)
        CHECK(!whole(c).blocked && !whole(c).striped);
        c.ss64 = 32;                         // half the bytes per slice
        CHECK(whole(c).striped);
    }
    {   // a row band of the triangle is judged by its own pairs: the first 200 rows of n = 2 000 are nearly a rectangle
        DenseCall c = self_call(2000);
        early_break(c, 2, 0.048);
        CHECK(plan_counts_launch(c, 0, 200).striped);       // every stripe holds ~200 rows x 128 columns: 1.07
        CHECK(!plan_counts_launch(c, 1500, 1999).striped);   // only the last four stripes hold a pair
    }
    {   // a blocked launch: n = 16 000 at 4.9 % (>= 48 Mi pairs)
        DenseCall c = self_call(16000);
        early_break(c, 2, 0.049);
        CHECK(whole(c).blocked && whole(c).lds_rows && !whole(c).striped);
        c.knobs.eb_stripes = 1;
        CHECK(!whole(c).striped);
    }
    {   // a mixed plan (block by block: the general kernel)
        DenseCall c = self_call(1000);
        early_break(c, 3, 0.05, true);
        CHECK(whole(c).mixed && !whole(c).striped);
        c.knobs.eb_stripes = 1;
        CHECK(!whole(c).striped);
    }
    {   // what the lean kernel does not take: a completeness vector outside (0, 1], a table that is not monotone, 157 chunks (the rows
        // do not fit the LDS), no early break
        DenseCall c = self_call(1000);
        early_break(c, 2, 0.048);
        c.knobs.eb_stripes = 1;
        c.has_comp = true;
        CHECK(!whole(c).striped);
        c.comp_unit = true;
        CHECK(whole(c).striped);
        c.min_alive = 0xFFFFFFFFu;
        CHECK(!whole(c).striped);
        c = self_call(1000);
        early_break(c, 2, 0.048);
        c.ss64 = 157;
        c.knobs.eb_stripes = 1;
        CHECK(!whole(c).striped);
        c = self_call(1000);
        c.knobs.eb_stripes = 1;
        CHECK(!whole(c).striped);
    }
    {   // the cases dense_plan_check.cpp pins keep the new field false
        DenseCall c = self_call(16000);
        early_break(c, 2, 0.02);
        CHECK(!whole(c).striped);
        c = self_call(2000);
        c.self_mode = false;
        c.r0 = 0;
        c.r1 = 500;
        early_break(c, 3, 0.01);
        CHECK(!whole(c).striped);
    }
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "map";
    if (!strcmp(what, "map")) map();
    else if (!strcmp(what, "balance")) balance();
    else if (!strcmp(what, "rule")) rule();
    else return 2;
    if (g_failed) printf("FAILED %ld of %ld\n", g_failed, g_checks);
    else printf("ok %ld\n", g_checks);
    return g_failed ? 1 : 0;
}
