// dense_plan_check.cpp -- CPU check of csrc/dense_plan.hpp, the launch plan of the dense distance calls (test infrastructure).
// Host compiler only: no HIP header, no device, the library is never loaded.
//   dense_plan_check pinned        : regimes whose plan is derived BY HAND from the rules (the arithmetic stands beside each case)
//   dense_plan_check bands N       : the band cuts as a property over N seeded calls
//   dense_plan_check consistency N : planes, record width and bytes agree with each other over N seeded launches
//   dense_plan_check shape         : the pair kernel's tile shape, form and name for launches derived BY HAND (plan_pair_shape)
//   dense_plan_check hostbands N   : the bands of a host-destined call, pinned cases and properties over N seeded calls
// Prints one line per failed check and "ok <checks>" / "FAILED <failures> of <checks>"; the exit status says which.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

#include "../../sketchlib.rust_amd/csrc/dense_plan.hpp"

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

// An MI355X as one device (256 CUs: 1 024 resident workgroup slots), default switches, 4 096 bins (64 chunks), 5 k-mer lengths,
// all-vs-all of n samples, no completeness; min_alive as ensure_ytab() sets it for a monotone table (any value but 0xFFFFFFFF).
static DenseCall self_call(uint64_t n, int mode = PLAN_MODE_COREACC)
{
    DenseCall c;
    c.mode = mode;
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
static bool uncut(const DenseCall &c)
{
    const RowBands b = plan_row_bands(c);
    return b.cuts.size() == 2 && b.cuts[0] == c.r0 && b.cuts[1] == c.r1 && !b.overlap;
}

static void pinned()
{
    // Thresholds all cases use: "tiny" below 2 x 4 x 256 x 2 048 = 4 194 304 evaluations (pairs x lengths); 4 x 256 = 1 024 slots;
    // a launch is tail-sliced up to 0.9 rounds: units x 100 <= 90 x 1 024 = 92 160 with units = evaluations / 2 048;
    // 8 slices when units x 16 <= 1 024; mid band from 4 194 304 to below 8 388 608 evaluations (tile32_min = 8 Mi).
    {   // n = 1 000, early break at 2 of 5 lengths
        DenseCall c = self_call(1000);
        early_break(c, 2, 0.011);
        const CountsLaunch L = whole(c);
        CHECK_EQ(L.form, FORM_COUNTS_EPILOGUE);
        CHECK_EQ(L.pairs, 499500);            // 1 000 x 999 / 2
        CHECK(L.early && !L.mixed && L.sliced);
        CHECK_EQ(L.lengths, 2);
        CHECK(!L.cnt_u16);                    // 999 000 evaluations < 4 194 304: tiny, u32
        CHECK_EQ(L.k_slices, 1);
        CHECK(L.tail && !L.mid_band);         // 999 000 / 2 048 = 487 units; 48 700 <= 92 160
        CHECK_EQ(L.tail_slices, 4);           // 487 x 16 = 7 792 > 1 024: 4 slices, not 8
        CHECK_EQ(L.slice_chunks, 16);         // ceil(64 / 4) = 16, already a multiple of 8
        CHECK(L.two_planes);
        CHECK_EQ(L.planes, 2);
        CHECK_EQ(L.plane_bytes, 3996000);     // 499 500 x 2 x 4
        CHECK(!L.blocked && !L.lds_rows);     // 1.1 % alive < 3 %, and far below 48 Mi pairs
        CHECK(L.lean && L.ahead && !L.comp_lean);
        CHECK(uncut(c));                      // 3 996 000 B of counts; overlapping bands start at 64 Mi pairs
    }
    {   // n = 1 000, no early break: all 5 lengths
        DenseCall c = self_call(1000);
        const CountsLaunch L = whole(c);
        CHECK_EQ(L.form, FORM_COUNTS_EPILOGUE);   // 499 500 pairs < 32 Mi: k-sliced counts + epilogue
        CHECK(!L.early && L.sliced);
        CHECK_EQ(L.lengths, 5);
        CHECK(!L.cnt_u16);                    // 2 497 500 evaluations < 4 194 304: still tiny
        CHECK(!L.tail && !L.two_planes);      // 2 497 500 / 2 048 = 1 219 units; 121 900 > 92 160
        CHECK(!L.mid_band);                   // 2 x 2 497 500 = 4 995 000 < 8 388 608
        CHECK_EQ(L.tail_slices, 0);
        CHECK_EQ(L.slice_chunks, 0);
        CHECK_EQ(L.planes, 1);
        CHECK_EQ(L.plane_bytes, 9990000);     // 499 500 x 5 x 4
        CHECK(uncut(c));
        early_break(c, 0, 0.6);               // a plan that says "count every length" changes nothing
        CHECK(!whole(c).early && whole(c).plane_bytes == 9990000 && uncut(c));
    }
    {   // n = 16 000, 2 lengths, 2 % alive: flat epilogue order, 4 overlapping bands
        DenseCall c = self_call(16000);
        early_break(c, 2, 0.02);
        const CountsLaunch L = whole(c);
        CHECK_EQ(L.pairs, 127992000);         // 16 000 x 15 999 / 2
        CHECK(L.cnt_u16 && !L.tail && !L.blocked && !L.lds_rows);   // 255 984 000 evaluations; 2 % < 3 %
        const RowBands b = plan_row_bands(c);
        // lean epilogue (2 lengths, no completeness) in the flat order: piping; 127 992 000 >= 64 Mi pairs.  want = max(32 Mi,
        // 127 992 000 / 8 = 15 999 000) = 33 554 432; fit = 4 Gi / (2 x 2) = 1 Gi; ceil(127 992 000 / 33 554 432) = 4 bands
        CHECK(b.overlap);
        CHECK_EQ(b.cuts.size(), 5);
        // cut b: the first row with at least b x 31 998 000 pairs before it; r rows hold 16 000 r - r (r + 1) / 2 pairs:
        // 2 143 -> 31 990 704, 2 144 -> 32 004 560; 4 686 -> 63 994 359, 4 687 -> 64 005 672; 7 999 -> 95 988 000, 8 000 -> 95 996 000
        if (b.cuts.size() == 5) {
            CHECK_EQ(b.cuts[0], 0);
            CHECK_EQ(b.cuts[1], 2144);
            CHECK_EQ(b.cuts[2], 4687);
            CHECK_EQ(b.cuts[3], 8000);
            CHECK_EQ(b.cuts[4], 15999);
            const CountsLaunch B = plan_counts_launch(c, b.cuts[0], b.cuts[1]);   // each band planned from its own pairs
            CHECK_EQ(B.pairs, 32004560);
            CHECK(B.cnt_u16 && !B.tail && !B.blocked);
            CHECK_EQ(B.plane_bytes, 128018240);   // 32 004 560 x 2 x 2
        }
        early_break(c, 2, 0.049);             // 4.9 % alive and >= 48 Mi pairs: blocked order; < 2^30 pairs: no bands
        CHECK(whole(c).blocked && whole(c).lds_rows && whole(c).cnt_u16);
        CHECK(uncut(c));
    }
    {   // block-by-block early break at n = 16 000: every length is a plane of the counts, the general epilogue, no overlap
        DenseCall c = self_call(16000);
        early_break(c, 3, 0.05, true);
        const CountsLaunch L = whole(c);
        CHECK(L.early && L.mixed && L.blocked && L.cnt_u16);
        CHECK_EQ(L.lengths, 5);
        CHECK_EQ(L.plane_bytes, 1279920000);  // 127 992 000 x 5 x 2 < 4 Gi
        CHECK(uncut(c));
    }
    {   // mid band: 1 300-1 790 genomes without early break
        const struct { uint64_t n; bool mid, u16; } cases[] = {
            {1290, false, false},   //   831 405 pairs, 4 157 025 evaluations: x 2 = 8 314 050 < 8 388 608; tiny
            {1300, true, false},    //   844 350 pairs, 4 221 750: x 2 = 8 443 500 >= 8 388 608
            {1500, true, false},    // 1 124 250 pairs, 5 621 250
            {1790, true, false},    // 1 601 155 pairs, 8 005 775 < 8 388 608
            {1840, false, true},    // 1 691 880 pairs, 8 459 400 >= 8 388 608: plain 32-row tiles (the dispatcher's rule), u16
        };
        for (const auto &k : cases) {
            const DenseCall c = self_call(k.n);
            const CountsLaunch L = whole(c);
            CHECK_EQ(L.mid_band, k.mid);
            CHECK_EQ(L.tail, k.mid);              // (none of them is under 0.9 rounds: 2 029 units and more)
            CHECK_EQ(L.two_planes, k.mid);
            CHECK_EQ(L.tail_slices, k.mid ? 2 : 0);
            CHECK_EQ(L.slice_chunks, k.mid ? 32 : 0);   // 64 / 2
            CHECK_EQ(L.cnt_u16, k.u16);
            CHECK_EQ(L.plane_bytes, L.pairs * 5 * (k.u16 ? 2 : 4));
        }
        DenseCall c = self_call(1500);
        c.knobs.mid_band = false;
        CHECK(!whole(c).mid_band && !whole(c).tail && whole(c).cnt_u16);   // 5 621 250 evaluations: not tiny
    }
    {   // under 1/16 round: n = 200, 19 900 pairs x 5 = 99 500 evaluations = 48 units; 48 x 16 = 768 <= 1 024
        DenseCall c = self_call(200);
        CountsLaunch L = whole(c);
        CHECK(L.tail && L.two_planes && !L.cnt_u16);
        CHECK_EQ(L.tail_slices, 8);
        CHECK_EQ(L.slice_chunks, 8);          // 64 / 8
        CHECK_EQ(L.plane_bytes, 398000);      // 19 900 x 5 x 4
        c.ss64 = 32;                          // 2 048 bins: too short for 8 slices (needs 64 chunks): 4 of 8
        L = whole(c);
        CHECK_EQ(L.tail_slices, 4);
        CHECK_EQ(L.slice_chunks, 8);
        c.ss64 = 8;                           // 512 bins: cannot be cut at all
        CHECK(!whole(c).tail && whole(c).planes == 1);
    }
    {   // beyond 65 535 bins: 1 563 chunks (100 032 bins)
        DenseCall c = self_call(3000);
        c.ss64 = 1563;
        c.fused_coreacc_ok = false;
        CountsLaunch L = whole(c);
        CHECK_EQ(L.form, FORM_COUNTS_EPILOGUE);
        CHECK(L.sliced && !L.cnt_u16);
        CHECK(L.tail);                        // 4 498 500 x 5 = 22 492 500 evaluations = 10 982 units <= 16 x 1 024 = 16 384 (10.7 rounds)
        CHECK_EQ(L.tail_slices, 4);           // ceil(1 563 / 4) = 391 -> 392; 1 563 / 392: 4 slices (392, 392, 392, 387)
        CHECK_EQ(L.slice_chunks, 392);
        CHECK_EQ(L.plane_bytes, 89970000);    // 4 498 500 x 5 x 4
        c = self_call(4000);                  // 7 998 000 x 5 = 39 990 000 evaluations = 19 526 units > 16 384
        c.ss64 = 1563;
        c.fused_coreacc_ok = false;
        L = whole(c);
        CHECK(!L.tail && !L.mid_band && !L.cnt_u16 && L.planes == 1);
        c = self_call(20000);                 // 199 990 000 pairs >= 32 Mi: still sliced
        c.ss64 = 1563;
        c.fused_coreacc_ok = false;
        CHECK(whole(c).sliced && !whole(c).cnt_u16);
        early_break(c, 2, 0.05);              // never the blocked order beyond 65 535 bins
        CHECK(!whole(c).blocked);
    }
    {   // 157 chunks (`-s 10000`): uneven slices
        DenseCall c = self_call(1000);
        c.ss64 = 157;
        early_break(c, 2, 0.011);
        CountsLaunch L = whole(c);            // 487 units as above
        CHECK(L.tail);
        CHECK_EQ(L.tail_slices, 4);           // ceil(157 / 4) = 40; ceil(157 / 40) = 4 slices (40, 40, 40, 37)
        CHECK_EQ(L.slice_chunks, 40);
        c = self_call(200);
        c.ss64 = 157;
        L = whole(c);                         // 48 units: 8 wanted; ceil(157 / 8) = 20 -> 24; ceil(157 / 24) = 7 slices (6 x 24 + 13)
        CHECK_EQ(L.tail_slices, 7);
        CHECK_EQ(L.slice_chunks, 24);
    }
    {   // single k
        DenseCall c = self_call(1000, PLAN_MODE_JACCARD);
        CountsLaunch L = whole(c);            // 499 500 pairs = 243 units; 24 300 <= 92 160; 243 x 16 > 1 024
        CHECK_EQ(L.form, FORM_SINGLE_K_TAIL);
        CHECK_EQ(L.lengths, 1);
        CHECK(L.tail && L.two_planes && !L.cnt_u16 && !L.mid_band && !L.early);
        CHECK_EQ(L.tail_slices, 4);
        CHECK_EQ(L.slice_chunks, 16);
        CHECK_EQ(L.planes, 2);
        CHECK_EQ(L.plane_bytes, 1998000);     // 499 500 x 4
        CHECK(uncut(c));
        c = self_call(3000, PLAN_MODE_JACCARD);   // 4 498 500 pairs = 2 196 units; 219 600 > 92 160
        CHECK_EQ(whole(c).form, FORM_DIRECT);
        c = self_call(1000, PLAN_MODE_JACCARD);
        c.forced_kernel = 3;                  // another kernel forced: no slices
        CHECK_EQ(whole(c).form, FORM_DIRECT);
        c = self_call(1000, PLAN_MODE_COUNTS);    // bin-match counts: always the mode's own kernel
        CHECK_EQ(whole(c).form, FORM_DIRECT);
        CHECK(uncut(c));
    }
    {   // cross: 500 reference rows against 2 000 queries, early break at 3 lengths
        DenseCall c = self_call(2000);
        c.self_mode = false;
        c.r0 = 0;
        c.r1 = 500;
        early_break(c, 3, 0.01);
        CountsLaunch L = whole(c);
        CHECK_EQ(L.pairs, 1000000);           // 500 x 2 000
        CHECK(!L.cnt_u16 && !L.tail && !L.mid_band);   // 3 000 000 evaluations: tiny; 1 464 units, 146 400 > 92 160; x 2 = 6 000 000 < 8 388 608
        CHECK_EQ(L.plane_bytes, 12000000);    // 1 000 000 x 3 x 4
        CHECK_EQ(c.out_base(100), 200000);
        L = plan_counts_launch(c, 100, 300);  // 400 000 pairs x 3 = 1 200 000 evaluations = 585 units; 58 500 <= 92 160
        CHECK(L.tail);
        CHECK_EQ(L.tail_slices, 4);
        CHECK_EQ(L.plane_bytes, 4800000);
    }
    {   // a row range of the condensed triangle
        const DenseCall c = self_call(1000);
        CHECK_EQ(c.out_base(0), 0);
        CHECK_EQ(c.out_base(1), 999);
        CHECK_EQ(c.out_base(998), 499499);    // the last pair
        CHECK_EQ(c.pairs(10, 20), 9845);      // rows 10..19 hold 989 + ... + 980 pairs
        CHECK_EQ(c.pairs(0, 1000), 499500);   // (row 999 holds none)
    }
    {   // SKL_K_SLICES=2 (A/B build): a plane per slice, u32, neither tail nor mid band
        DenseCall c = self_call(1500);
        c.knobs.k_slices = 2;
        const CountsLaunch L = whole(c);
        CHECK_EQ(L.k_slices, 2);
        CHECK_EQ(L.slice_chunks, 32);
        CHECK(!L.tail && !L.mid_band && !L.two_planes && !L.cnt_u16);
        CHECK_EQ(L.tail_slices, 0);
        CHECK_EQ(L.planes, 2);
        CHECK_EQ(L.plane_bytes, 22485000);    // 1 124 250 x 5 x 4
    }
    {   // u32 counts beyond COUNTS_SCRATCH_MAX: 30 000 genomes at 1 563 chunks, every length
        DenseCall c = self_call(30000);
        c.ss64 = 1563;
        c.fused_coreacc_ok = false;
        const RowBands b = plan_row_bands(c);
        // 449 985 000 pairs x 5 x 4 = 8 999 700 000 B > 4 294 967 296; fit = 4 Gi / 20 = 214 748 364 pairs; ceil(449 985 000 / fit) = 3
        CHECK(!b.overlap);
        CHECK_EQ(b.cuts.size(), 4);
        for (size_t i = 0; i + 1 < b.cuts.size(); ++i) CHECK(plan_counts_launch(c, b.cuts[i], b.cuts[i + 1]).plane_bytes <= COUNTS_SCRATCH_MAX);
        c.r0 = 7;                             // a single row is never cut
        c.r1 = 8;
        CHECK(uncut(c));
    }
    {   // more than 6 k-mer lengths and 32 Mi pairs or more: unfused but not k-sliced ([pair][k] records, one plane, u32)
        DenseCall c = self_call(9000);        // 40 495 500 pairs
        c.nk = 7;
        c.fused_coreacc_ok = false;
        const CountsLaunch L = whole(c);
        CHECK_EQ(L.form, FORM_COUNTS_EPILOGUE);
        CHECK(!L.sliced && !L.cnt_u16 && !L.tail && !L.mid_band);
        CHECK_EQ(L.k_slices, 1);
        CHECK_EQ(L.planes, 1);
        c.fused_coreacc_ok = true;
        c.nk = 5;
        CHECK_EQ(whole(c).form, FORM_DIRECT);     // the fused all-k kernel
        c.knobs.sliced_max_pairs = 1ll << 40;     // SKL_SLICED_MAX_PAIRS
        CHECK_EQ(whole(c).form, FORM_COUNTS_EPILOGUE);
        c.forced_kernel = 3;
        CHECK_EQ(whole(c).form, FORM_DIRECT);
    }
    {   // the lean epilogue's conditions decide the overlap: completeness values outside (0, 1], or a table that is not monotone
        DenseCall c = self_call(16000);
        early_break(c, 2, 0.02);
        c.has_comp = true;
        c.comp_unit = false;
        CHECK(uncut(c) && !whole(c).comp_lean);
        c.comp_unit = true;
        CHECK(plan_row_bands(c).overlap && whole(c).comp_lean);
        c.min_alive = 0xFFFFFFFFu;
        CHECK(uncut(c));
    }
}

// pairs of rows [a, b) counted one row at a time: independent of self_rows_pairs' closed form
static uint64_t pairs_by_rows(const DenseCall &c, uint64_t a, uint64_t b)
{
    uint64_t p = 0;
    for (uint64_t r = a; r < b; ++r) p += c.self_mode ? (r + 1 < c.n_cols ? c.n_cols - 1 - r : 0) : c.n_cols;
    return p;
}

static void bands(size_t n_cases)
{
    std::mt19937_64 rng(0x5EEDBA5D);
    for (size_t it = 0; it < n_cases; ++it) {
        DenseCall c = self_call(2 + rng() % 40000);
        c.self_mode = (rng() & 1) != 0;
        const uint64_t row_limit = c.self_mode ? c.n_cols - 1 : 1 + rng() % 40000;
        c.r0 = rng() % row_limit;
        c.r1 = c.r0 + 1 + rng() % (row_limit - c.r0);
        const uint64_t pairs = c.pairs(c.r0, c.r1), target = 1 + rng() % 12;
        // (1) the cutting itself, for a number of bands asked for
        {
            const std::vector<uint64_t> cuts = cut_row_bands(c, target);
            CHECK(cuts.size() >= 2 && cuts.size() <= target + 1);
            CHECK(cuts.front() == c.r0 && cuts.back() == c.r1);
            const uint64_t row_pairs = c.self_mode ? c.n_cols - 1 - c.r0 : c.n_cols;   // the widest row of the call
            uint64_t sum = 0;
            for (size_t b = 0; b + 1 < cuts.size(); ++b) {
                CHECK(cuts[b] < cuts[b + 1]);   // strictly increasing: every band has a row
                const uint64_t bp = c.pairs(cuts[b], cuts[b + 1]);
                CHECK_EQ(bp, pairs_by_rows(c, cuts[b], cuts[b + 1]));
                // equal pair counts up to the row granularity: a cut is the first row at or beyond its target
                CHECK(bp <= pairs / target + 1 + row_pairs || cuts[b + 1] - cuts[b] == 1);
                sum += bp;
            }
            CHECK_EQ(sum, pairs);
        }
        // (2) through the rule: the pipeline forced onto this size (A/B build: SKL_EB_PIPELINE_MIN), and a scratch bound that bites
        //     (a sketch beyond 65 535 bins with up to 8 lengths: u32 counts)
        const bool scratch_case = (it % 3) == 0;
        if (scratch_case) {
            c.ss64 = 1563;
            c.nk = 3 + (uint32_t)(rng() % 6);
            c.fused_coreacc_ok = false;
        } else {
            early_break(c, 2 + (int)(rng() % 3), 0.01);
            c.knobs.eb_pipeline_min = (long long)std::max<uint64_t>(2, pairs / (1 + rng() % 8));
        }
        const RowBands rb = plan_row_bands(c);
        CHECK(rb.cuts.size() >= 2 && rb.cuts.front() == c.r0 && rb.cuts.back() == c.r1);
        CHECK_EQ(rb.overlap, !scratch_case && rb.cuts.size() > 2);
        if (!scratch_case && c.r1 - c.r0 > 1) CHECK(rb.cuts.size() > 2);   // (pairs >= the forced minimum: always cut)
        const uint64_t row_bytes = (c.self_mode ? c.n_cols - 1 - c.r0 : c.n_cols) * c.nk * 4;
        for (size_t b = 0; b + 1 < rb.cuts.size(); ++b) {
            CHECK(rb.cuts[b] < rb.cuts[b + 1]);
            const CountsLaunch L = plan_counts_launch(c, rb.cuts[b], rb.cuts[b + 1]);
            CHECK_EQ(L.form, FORM_COUNTS_EPILOGUE);
            // the counts of a band fit the scratch bound, up to the one row a cut may overshoot its target by (the bound sizes an
            // allocation that grows to what is asked of it: it is a budget, not a buffer's end) -- unless the band is a single row
            CHECK(L.plane_bytes <= COUNTS_SCRATCH_MAX + row_bytes || rb.cuts[b + 1] - rb.cuts[b] == 1);
        }
    }
}

static void consistency(size_t n_cases)
{
    std::mt19937_64 rng(0xC0175157);
    const uint32_t sketch_sizes[] = {8, 16, 32, 64, 157, 256, 1023, 1024, 1563};
    for (size_t it = 0; it < n_cases; ++it) {
        DenseCall c = self_call(2 + rng() % 30000, rng() % 4 == 0 ? PLAN_MODE_JACCARD : PLAN_MODE_COREACC);
        c.self_mode = (rng() & 1) != 0;
        const uint64_t row_limit = c.self_mode ? c.n_cols - 1 : 1 + rng() % 30000;
        c.r0 = rng() % row_limit;
        c.r1 = c.r0 + 1 + rng() % (row_limit - c.r0);
        c.nk = 2 + (uint32_t)(rng() % 7);
        c.ss64 = sketch_sizes[rng() % 9];
        c.fused_coreacc_ok = c.nk <= 6 && 64 * c.ss64 <= 0xFFFFu;
        c.has_comp = rng() % 4 == 0;
        c.comp_unit = (rng() & 1) != 0;
        if (rng() % 8 == 0) c.min_alive = 0xFFFFFFFFu;
        if (rng() % 3 && c.nk >= 3) early_break(c, rng() % 3 ? 2 + (int)(rng() % 3) : 0, (double)(rng() % 100) / 1000.0, rng() % 5 == 0);
        if (c.eb_lengths >= (int)c.nk) c.eb_lengths = 0;
        if (rng() % 6 == 0) c.knobs.k_slices = 1 + (int)(rng() % 4);
        if (rng() % 6 == 0) c.knobs.tail_slices = (int)(rng() % 9);
        if (rng() % 6 == 0) c.knobs.tail_max_pct = 100000000;
        if (rng() % 6 == 0) c.knobs.tile32_min = rng() % 2 ? 0 : -1;
        if (rng() % 8 == 0) c.knobs.counts_u16 = false;
        if (rng() % 8 == 0) c.knobs.eb_blocked = (int)(rng() % 2);
        if (rng() % 8 == 0) c.knobs.sliced_max_pairs = 1ll << 40;
        if (rng() % 16 == 0) c.forced_kernel = 3 + (int)(rng() % 2);
        if (c.forced_kernel == 3) c.eb_plan = false;   // (dense_band asks for no early-break plan when another kernel is forced)
        const CountsLaunch L = whole(c);
        CHECK_EQ(L.pairs, c.pairs(c.r0, c.r1));
        if (L.form == FORM_DIRECT) continue;
        CHECK_EQ(L.two_planes, L.tail);
        CHECK(!L.cnt_u16 || (!L.tail && L.k_slices == 1 && L.sliced && c.ss64 <= 1023));
        CHECK(!L.mid_band || (L.tail && L.tail_slices == 2));
        CHECK(!L.tail || (L.tail_slices > 1 && L.slice_chunks >= 8 && L.slice_chunks % 8 == 0 && (uint64_t)L.tail_slices * L.slice_chunks >= c.ss64 &&
                          (uint64_t)(L.tail_slices - 1) * L.slice_chunks < c.ss64));
        CHECK(L.tail || L.tail_slices == 0);
        CHECK(!L.tail || L.k_slices == 1);
        CHECK_EQ(L.planes, L.tail ? 2 : L.k_slices);
        CHECK_EQ(L.lengths, L.form == FORM_SINGLE_K_TAIL ? 1 : c.eb_plan && !c.eb_mixed && c.eb_lengths > 0 ? c.eb_lengths : (int)c.nk);
        CHECK_EQ(L.plane_bytes, L.pairs * L.lengths * (L.cnt_u16 ? 2 : 4));
        CHECK(!L.blocked || L.early);
        CHECK(L.sliced || (!L.early && L.k_slices == 1 && !L.tail));
    }
}

// One launch on an MI355X as one device (256 CUs, 8 XCDs: 4 x 256 / 8 = 128 resident workgroups per XCD), default switches.
static PairLaunch launch_of(int mode, bool self_mode, uint64_t rows, uint32_t nB, uint32_t k_count, bool k_sliced)
{
    PairLaunch a;
    a.mode = mode;
    a.self_mode = self_mode;
    a.rows = rows;
    a.nB = nB;
    a.k_count = k_count;
    a.ss64 = 64;
    a.k_sliced = k_sliced;
    a.xcd_shift = plan_xcd_shift(a.n_cu, a.knobs.xcds);
    return a;
}
#define CHECK_NAME(shape, ok, text)                                                                   \
    do {                                                                                              \
        ++g_checks;                                                                                   \
        const std::string got_ = pair_kernel_name(shape, ok);                                         \
        if (got_ != (text)) {                                                                         \
            ++g_failed;                                                                               \
            if (g_failed <= 40) printf("%s:%d: name \"%s\"\n", __FILE__, __LINE__, got_.c_str());     \
        }                                                                                             \
    } while (0)

static void shape()
{
    // XCDs the tile order deals to: CUs / 32, at most 8, as a shift; SKL_XCDS overrides
    CHECK_EQ(plan_xcd_shift(256, 0), 3);
    CHECK_EQ(plan_xcd_shift(32, 0), 0);     // a CPX partition
    CHECK_EQ(plan_xcd_shift(64, 0), 1);
    CHECK_EQ(plan_xcd_shift(128, 0), 2);
    CHECK_EQ(plan_xcd_shift(304, 0), 3);    // 9 "XCDs": capped at 8
    CHECK_EQ(plan_xcd_shift(256, 2), 1);
    CHECK_EQ(plan_xcd_shift(256, 4), 2);
    CHECK_EQ(plan_xcd_shift(32, 8), 3);
    CHECK_EQ(TILE_ROWS_SMALL, 16);
    CHECK_EQ(TILE_ROWS_LARGE, 32);
    {   // DESIGN.md 4.1, row 1 -- cfg 2: 1 000 genomes, early break at 2 lengths, tail slices: 499 500 pairs x 2 = 999 000 < 8 Mi
        PairLaunch a = launch_of(PLAN_MODE_COUNTS, true, 999, 1000, 2, true);
        a.tail_slices = 4;
        const PairShape s = plan_pair_shape(a);
        CHECK_EQ(s.shape, 165);
        CHECK_EQ(s.tile_rows, 16);
        CHECK(s.sliced_launch && s.try_kslice && !s.no_half_tiles);
        CHECK_EQ(s.ablate, 0);
        CHECK_EQ(s.wg_per_cu, 4);
        CHECK_EQ(s.round_size, 128);       // 4 x 256 / 8
        CHECK_EQ(s.tail_resident, 128);
        CHECK_EQ(s.ksplit_rows, 8);
        CHECK_NAME(s, true, "skl::pair_kernel_kslice<R=16, JL=2, COUNTS, k-sliced, tight> (16x128 tiles, chunks split over 4 waves; 4 chunk slices per unit in the last round of workgroups)");
        CHECK_NAME(s, false, "skl::pair_kernel_ksplit<R=8, COUNTS> (8x64 tiles, chunks split over 4 waves)");   // the kernel declines: pair_ksplit.hip
        a.tail_slices = 1;                 // tail_resident only with more than one slice
        CHECK_EQ(plan_pair_shape(a).tail_resident, 0);
        a.tail_slices = 0;
        CHECK_EQ(plan_pair_shape(a).tail_resident, 0);
        CHECK_NAME(plan_pair_shape(a), true, "skl::pair_kernel_kslice<R=16, JL=2, COUNTS, k-sliced, tight> (16x128 tiles, chunks split over 4 waves)");
        a.tail_slices = 4;
        a.knobs.round_priority = false;    // SKL_ROUND_PRIORITY=0: no rounds, the tail still needs its residency
        CHECK_EQ(plan_pair_shape(a).round_size, 0);
        CHECK_EQ(plan_pair_shape(a).tail_resident, 128);
        a.knobs.half_tiles = false;
        CHECK(plan_pair_shape(a).no_half_tiles);
        a.n_cu = 32;                       // a CPX partition: 4 x 32 / 1
        a.xcd_shift = 0;
        a.knobs.round_priority = true;
        CHECK_EQ(plan_pair_shape(a).round_size, 128);
    }
    {   // row 2 -- from 8 Mi = 8 388 608 evaluations 32 x 128 tiles: 3 000 genomes at 2 lengths: 4 498 500 x 2 = 8 997 000
        const PairLaunch a = launch_of(PLAN_MODE_COUNTS, true, 2999, 3000, 2, true);
        const PairShape s = plan_pair_shape(a);
        CHECK_EQ(s.shape, 325);
        CHECK_EQ(s.tile_rows, 32);
        CHECK(s.sliced_launch);
        CHECK_EQ(s.wg_per_cu, 4);
        CHECK_NAME(s, true, "skl::pair_kernel_kslice<R=32, JL=2, COUNTS, k-sliced, tight> (32x128 tiles, chunks split over 4 waves)");
        // the threshold itself, single k (one length walked whatever k_count says): 4 096 x 2 048 = 8 388 608
        CHECK_EQ(plan_pair_shape(launch_of(PLAN_MODE_JACCARD, false, 4096, 2048, 5, false)).shape, 325);
        CHECK_EQ(plan_pair_shape(launch_of(PLAN_MODE_JACCARD, false, 4095, 2048, 5, false)).shape, 165);
        CHECK(plan_pair_shape(launch_of(PLAN_MODE_JACCARD, false, 4095, 2048, 1, false)).sliced_launch);   // single k: always k-sliced
        CHECK_NAME(plan_pair_shape(launch_of(PLAN_MODE_JACCARD, false, 4096, 2048, 1, false)), true,
                   "skl::pair_kernel_kslice<R=32, JL=2, JACCARD, k-sliced, tight> (32x128 tiles, chunks split over 4 waves)");
        PairLaunch t = a;
        t.knobs.tile32_min = -1;           // SKL_TILE32_MIN=-1: never
        CHECK_EQ(plan_pair_shape(t).shape, 165);
        t = launch_of(PLAN_MODE_COUNTS, true, 99, 100, 2, true);
        CHECK_EQ(plan_pair_shape(t).shape, 165);
        t.knobs.tile32_min = 0;            // 0: always
        CHECK_EQ(plan_pair_shape(t).shape, 325);
    }
    {   // row 3 -- fused all-k core/accessory: 9 000 genomes, 40 495 500 pairs x 5
        const PairShape s = plan_pair_shape(launch_of(PLAN_MODE_COREACC, true, 8999, 9000, 5, false));
        CHECK_EQ(s.shape, 325);
        CHECK(!s.sliced_launch);
        CHECK_NAME(s, true, "skl::pair_kernel_kslice<R=32, JL=2, COREACC, all k, tight> (32x128 tiles, chunks split over 4 waves)");
        CHECK(!plan_pair_shape(launch_of(PLAN_MODE_COREACC, true, 99, 100, 5, true)).sliced_launch);   // never sliced in this mode
    }
    {   // row 4 -- beyond 1 023 chunks the k-sliced form whatever the size; bin-match launches otherwise only below 8 Mi pairs
        PairLaunch a = launch_of(PLAN_MODE_COUNTS, true, 4999, 5000, 5, false);   // 12 497 500 pairs
        CHECK(!plan_pair_shape(a).sliced_launch && !plan_pair_shape(a).big_sketch);
        CHECK_NAME(plan_pair_shape(a), true, "skl::pair_kernel_kslice<R=32, JL=2, COUNTS, all k, tight> (32x128 tiles, chunks split over 4 waves)");
        a.ss64 = 1023;
        CHECK(!plan_pair_shape(a).sliced_launch);
        a.ss64 = 1024;
        CHECK(plan_pair_shape(a).sliced_launch && plan_pair_shape(a).big_sketch);
        CHECK_NAME(plan_pair_shape(a), true, "skl::pair_kernel_kslice<R=32, JL=2, COUNTS, k-sliced, tight> (32x128 tiles, chunks split over 4 waves; segments of 1016 chunks)");
        CHECK(plan_pair_shape(launch_of(PLAN_MODE_COUNTS, true, 4095, 4096, 5, false)).sliced_launch);    // 4 095 x 4 096 / 2 = 8 386 560 < 8 388 608
        CHECK(!plan_pair_shape(launch_of(PLAN_MODE_COUNTS, true, 4096, 4096, 5, false)).sliced_launch);   // 8 388 608
        CHECK_EQ(SMALL_LAUNCH_PAIRS, 8388608);
    }
    {   // the mid band forces 32-row tiles below the threshold: 1 500 genomes x 5 lengths = 5 621 250 evaluations, last round in 2 slices
        PairLaunch a = launch_of(PLAN_MODE_COUNTS, true, 1499, 1500, 5, true);
        CHECK_EQ(plan_pair_shape(a).shape, 165);
        a.mid_band = true;
        a.tail_slices = 2;
        const PairShape s = plan_pair_shape(a);
        CHECK_EQ(s.shape, 325);
        CHECK_EQ(s.tile_rows, 32);
        CHECK_EQ(s.tail_resident, 128);
        CHECK_NAME(s, true, "skl::pair_kernel_kslice<R=32, JL=2, COUNTS, k-sliced, tight> (32x128 tiles, chunks split over 4 waves; 2 chunk slices per unit in the last round of workgroups)");
    }
    {   // the A/B build's forms.  3254 = round 2's k-sliced 32-row form, 3255 its all-k form: 3 waves per SIMD = 3 workgroups per CU
        // in THAT form, 4 in the other; 1651 / 1652 the 16-row forms
        PairLaunch a = launch_of(PLAN_MODE_COUNTS, true, 999, 1000, 5, true);
        CHECK_EQ(plan_pair_shape(a).shape, 165);             // the switches at their defaults, which the product library never leaves (tests/test_knobs_cpu.py)
        a.knobs.kslice_shape = 3254;
        a.tail_slices = 4;
        PairShape s = plan_pair_shape(a);
        CHECK_EQ(s.shape, 3254);
        CHECK_EQ(s.tile_rows, 32);
        CHECK_EQ(s.wg_per_cu, 3);
        CHECK_EQ(s.round_size, 96);                          // 3 x 256 / 8
        CHECK_EQ(s.tail_resident, 96);
        CHECK_NAME(s, true, "skl::pair_kernel_kslice<R=32, JL=2, COUNTS, k-sliced, tight> (32x128 tiles, chunks split over 4 waves; 4 chunk slices per unit in the last round of workgroups)");
        a.knobs.kslice_shape = 3255;
        CHECK_EQ(plan_pair_shape(a).wg_per_cu, 4);           // sliced launch in the all-k shape
        PairLaunch f = launch_of(PLAN_MODE_COREACC, true, 999, 1000, 5, false);
        f.knobs.kslice_shape = 3255;
        s = plan_pair_shape(f);
        CHECK_EQ(s.wg_per_cu, 3);
        CHECK_EQ(s.round_size, 96);
        CHECK_EQ(s.tail_resident, 0);
        CHECK_NAME(s, true, "skl::pair_kernel_kslice<R=32, JL=2, COREACC, all k, tight> (32x128 tiles, chunks split over 4 waves)");
        f.knobs.kslice_shape = 3254;
        CHECK_EQ(plan_pair_shape(f).wg_per_cu, 4);
        f.knobs.kslice_shape = 1652;
        CHECK_EQ(plan_pair_shape(f).tile_rows, 16);
        CHECK_NAME(plan_pair_shape(f), true, "skl::pair_kernel_kslice<R=16, JL=2, COREACC, all k, tight> (16x128 tiles, chunks split over 4 waves)");
        f.knobs.kslice_shape = 0;
        f.knobs.kslice_ablate = 2;
        CHECK_EQ(plan_pair_shape(f).ablate, 2);
        f.knobs.kernel = 3;                                     // SKL_KERNEL=ksplit: the chunk-split kernel is not asked
        f.knobs.ksplit_rows = 4;
        s = plan_pair_shape(f);
        CHECK(!s.try_kslice);
        CHECK_EQ(s.ksplit_rows, 4);
        CHECK_NAME(s, true, "skl::pair_kernel_ksplit<R=4, COREACC> (4x64 tiles, chunks split over 4 waves)");
    }
}

// plan_host_bands: four calls cut by hand, then what every cut must satisfy
static void host_bands(size_t n_cases)
{
    {   // cross, 1 000 columns, 8-byte records, rows [0, 10), 24 000 B per band = 3 rows
        const HostBands h = plan_host_bands(false, 1000, 0, 10, 8, 24000);
        CHECK_EQ(h.bands.size(), 4);
        CHECK_EQ(h.band_alloc, 24000);
        CHECK_EQ(h.second_alloc, 24000);
        const uint64_t r1[] = {3, 6, 9, 10}, pairs[] = {3000, 3000, 3000, 1000};
        for (size_t b = 0; b < h.bands.size() && b < 4; ++b) {
            CHECK_EQ(h.bands[b].r0, b ? r1[b - 1] : 0);
            CHECK_EQ(h.bands[b].r1, r1[b]);
            CHECK_EQ(h.bands[b].pairs, pairs[b]);
            CHECK_EQ(h.bands[b].buf, b & 1);
            CHECK(!h.bands[b].own_buffer);
        }
    }
    {   // the same call under a bound it fits: one band, the second buffer a token
        const HostBands h = plan_host_bands(false, 1000, 0, 10, 8, 1u << 30);
        CHECK_EQ(h.bands.size(), 1);
        CHECK_EQ(h.band_alloc, 80000);
        CHECK_EQ(h.second_alloc, 16);
        CHECK(h.bands.size() == 1 && h.bands[0].r0 == 0 && h.bands[0].r1 == 10 && h.bands[0].pairs == 10000 && !h.bands[0].own_buffer);
    }
    {   // a single row (8 000 B) wider than a band (4 000 B): every row its own band and its own buffer
        const HostBands h = plan_host_bands(false, 1000, 2, 5, 8, 4000);
        CHECK_EQ(h.bands.size(), 3);
        CHECK_EQ(h.band_alloc, 4000);
        for (size_t b = 0; b < h.bands.size(); ++b) {
            CHECK(h.bands[b].own_buffer && h.bands[b].r1 == h.bands[b].r0 + 1 && h.bands[b].pairs == 1000);
            CHECK_EQ(h.bands[b].r0, 2 + b);
        }
    }
    {   // the triangle of 10 samples: rows hold 9, 8, ..., 1 pairs; 136 B = 17 pairs per band: 9 + 8 | 7 + 6 (+ 5 = 18) | 5 + 4 + 3 + 2 + 1 = 15
        const HostBands h = plan_host_bands(true, 10, 0, 9, 8, 136);
        CHECK_EQ(h.bands.size(), 3);
        CHECK_EQ(h.band_alloc, 136);
        if (h.bands.size() == 3) {
            CHECK(h.bands[0].r0 == 0 && h.bands[0].r1 == 2 && h.bands[0].pairs == 17);
            CHECK(h.bands[1].r0 == 2 && h.bands[1].r1 == 4 && h.bands[1].pairs == 13);
            CHECK(h.bands[2].r0 == 4 && h.bands[2].r1 == 9 && h.bands[2].pairs == 15);
            CHECK(h.bands[2].buf == 0 && !h.bands[0].own_buffer && !h.bands[2].own_buffer);
        }
    }
    std::mt19937_64 rng(0xB05DBA9D);
    for (size_t it = 0; it < n_cases; ++it) {
        const bool self = (rng() & 1) != 0;
        const uint64_t n = 2 + rng() % 5000;
        const uint64_t row_limit = self ? n - 1 : 1 + rng() % 300;
        const uint64_t r0 = rng() % row_limit, r1 = r0 + 1 + rng() % (row_limit - r0);
        const size_t recs[] = {4, 8, 20};   // single k, core/accessory, bin-match counts of 5 lengths
        const size_t rec = recs[rng() % 3];
        const size_t band_bytes = 64 + (size_t)(rng() % (it % 4 == 0 ? 4000 : 4000000));
        const HostBands h = plan_host_bands(self, n, r0, r1, rec, band_bytes);
        const uint64_t all = self ? self_rows_pairs(r0, r1, n) : (r1 - r0) * n;
        CHECK_EQ(h.band_alloc, std::min<uint64_t>(band_bytes, all * rec));
        CHECK_EQ(h.second_alloc, all * rec > band_bytes ? h.band_alloc : 16);
        CHECK(!h.bands.empty() && h.bands.front().r0 == r0 && h.bands.back().r1 == r1);
        uint64_t sum = 0;
        for (size_t b = 0; b < h.bands.size(); ++b) {
            const HostBand &B = h.bands[b];
            CHECK(B.r0 < B.r1);
            if (b) CHECK_EQ(B.r0, h.bands[b - 1].r1);   // [r0, r1) once, in order
            CHECK_EQ(B.buf, b & 1);
            DenseCall c;
            c.self_mode = self;
            c.n_cols = n;
            CHECK_EQ(B.pairs, pairs_by_rows(c, B.r0, B.r1));
            const bool single = B.r1 - B.r0 == 1;
            CHECK(B.pairs * rec <= band_bytes || single);          // within the bound unless it is a single row ...
            CHECK_EQ(B.own_buffer, B.pairs * rec > h.band_alloc);  // ... which is then flagged
            CHECK(!B.own_buffer || single);
            // the band is full: the next row would not have fitted
            if (B.r1 < r1) CHECK((B.pairs + (self ? n - 1 - B.r1 : n)) * rec > band_bytes);
            sum += B.pairs;
        }
        CHECK_EQ(sum, all);   // (self mode: = self_rows_pairs(r0, r1, n))
    }
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "pinned";
    const size_t n = argc > 2 ? strtoull(argv[2], nullptr, 10) : 4000;
    if (!strcmp(what, "pinned")) pinned();
    else if (!strcmp(what, "bands")) bands(n);
    else if (!strcmp(what, "consistency")) consistency(n);
    else if (!strcmp(what, "shape")) shape();
    else if (!strcmp(what, "hostbands")) host_bands(n);
    else return 2;
    if (g_failed) printf("FAILED %ld of %ld\n", g_failed, g_checks);
    else printf("ok %ld\n", g_checks);
    return g_failed ? 1 : 0;
}
