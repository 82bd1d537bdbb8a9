// knn_plan_check.cpp -- CPU check of csrc/knn_plan.hpp, the plan of the kNN band drivers (test infrastructure).
// Host compiler only: no HIP header, no device, the library is never loaded.
//   knn_plan_check pinned       : band heights and panels derived BY HAND from the rules (the arithmetic stands beside each case)
//   knn_plan_check coverage N   : over N seeded calls of each form: every pair once, ascending arrival, buffers hold their views
//   knn_plan_check agreement N  : the multi-GPU drivers' band height equals the symmetric height under the fixed budget
// Prints one line per failed check and "ok <checks>" / "FAILED <failures> of <checks>"; the exit status says which.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../sketchlib.rust_amd/csrc/knn_plan.hpp"

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

constexpr size_t GiB = 1ull << 30;

// rows [r0, r1) against n_cand candidates on a device with 256 GiB free: default switches, 5 k-mer lengths, 4 096 bins
static KnnRowsCall rows_call(size_t n_cand, size_t r0, size_t r1, size_t knn, bool self_mode, bool coreacc = false)
{
    KnnRowsCall c;
    c.n_cand = n_cand;
    c.r0 = r0;
    c.r1 = r1;
    c.knn = knn;
    c.self_mode = self_mode;
    c.coreacc = coreacc;
    c.nk = 5;
    c.ss64 = 64;
    c.free_bytes = 256 * GiB;
    return c;
}

static void pinned()
{
    // With 256 GiB free: the key bands take min(free / 4, 8 GiB) = 8 GiB, two of them; the symmetric budget is
    // min(free / 2, 32 GiB) = 32 GiB for single-k keys, min(free / 2, 96 GiB) = 96 GiB for core/accessory keys, four buffers.
    {   // cfg 5: 1 M samples, single k, knn 50.  Row by row: 4 GiB / (10^6 x 4) = 1 073.  Symmetric: budget rows
        // 8 GiB / 4 000 000 = 2 147 -> 2 144 (multiple of 16); wanted max(up16(125 000) = 125 008, up16(33 + 1) = 48); the smaller: 2 144
        CHECK_EQ(symmetric_band_rows(1000000, 4, 32 * GiB, 1), 2144);
        const KnnRowsPlan P = plan_knn_rows(rows_call(1000000, 0, 1000000, 50, true));
        CHECK(P.symmetric);
        CHECK_EQ(P.band_rows, 2144);
        CHECK(P.overlap);
        KnnRowsCall off = rows_call(1000000, 0, 1000000, 50, true);
        off.knobs.knn_symmetric = false;   // row by row: the two-band height
        CHECK(!plan_knn_rows(off).symmetric);
        CHECK_EQ(plan_knn_rows(off).band_rows, 1073);
        KnnRowsCall part = rows_call(1000000, 1000, 1000000, 50, true);   // not the whole matrix: row by row
        CHECK(!plan_knn_rows(part).symmetric);
        CHECK_EQ(plan_knn_rows(part).band_rows, 1073);
    }
    {   // ... its core/accessory leg: the budget counts 8 + 4 bytes per pair (record + the early break's counts, 5 lengths, fused form):
        // 96 GiB / 4 = 24 GiB / 12 000 000 = 2 147 -> 2 144
        CHECK_EQ(coreacc_rec_with_counts(true, 5, true), 12);
        CHECK_EQ(coreacc_rec_with_counts(true, 2, true), 8);    // fewer than 3 lengths: no early break, no counts
        CHECK_EQ(coreacc_rec_with_counts(true, 5, false), 8);
        CHECK_EQ(coreacc_rec_with_counts(false, 5, true), 4);
        const KnnRowsPlan P = plan_knn_rows(rows_call(1000000, 0, 1000000, 50, true, true));
        CHECK(P.symmetric);
        CHECK_EQ(P.band_rows, 2144);
        CHECK(P.overlap);
        KnnRowsCall unfused = rows_call(1000000, 0, 1000000, 50, true, true);
        unfused.fused_coreacc_ok = false;   // no symmetric form: 4 GiB / (10^6 x 8) = 536 rows
        CHECK(!plan_knn_rows(unfused).symmetric);
        CHECK_EQ(plan_knn_rows(unfused).band_rows, 536);
        // free memory unknown: BAND_BYTES (512 MiB) on both sides: 128 MiB / 12 000 000 = 11 -> 0 -> at least 16 rows
        KnnRowsCall blind = rows_call(1000000, 0, 1000000, 50, true, true);
        blind.free_bytes = 0;
        CHECK(plan_knn_rows(blind).symmetric);
        CHECK_EQ(plan_knn_rows(blind).band_rows, 16);
    }
    {   // too small for the symmetric form: a band wants 32 Mi pairs.  n = 1 000: up16(33 554 + 1) = 33 568 >= n: refused, one band
        const KnnRowsPlan P = plan_knn_rows(rows_call(1000, 0, 1000, 10, true));
        CHECK(!P.symmetric);
        CHECK_EQ(P.band_rows, 1000);
        CHECK(!P.overlap);
        // the threshold: n = 5 793: 33 554 432 / 5 793 = 5 792 + 1 = 5 793 -> 5 808 >= n: refused;
        // n = 5 808: 5 777 + 1 -> 5 792 < n (and up16(726) = 736 below it): taken, two bands
        CHECK(!plan_knn_rows(rows_call(5793, 0, 5793, 10, true)).symmetric);
        const KnnRowsPlan Q = plan_knn_rows(rows_call(5808, 0, 5808, 10, true));
        CHECK(Q.symmetric);
        CHECK_EQ(Q.band_rows, 5792);
        CHECK(Q.overlap);
        CHECK(!plan_knn_rows(rows_call(5808, 0, 5808, 10, false)).symmetric);   // a cross call never is
    }
    {   // SKL_KNN_BAND_ROWS = 100 on n = 1 000: the height of either form, so the symmetric form is taken (100 < n)
        KnnRowsCall c = rows_call(1000, 0, 1000, 10, true);
        c.knobs.knn_band_rows = 100;
        CHECK(plan_knn_rows(c).symmetric);
        CHECK_EQ(plan_knn_rows(c).band_rows, 100);
        CHECK(plan_knn_rows(c).overlap);
        c.knobs.knn_overlap = false;
        CHECK(!plan_knn_rows(c).overlap);
        c.r0 = 200;   // row by row, clipped to the rows there are
        c.r1 = 260;
        CHECK(!plan_knn_rows(c).symmetric);
        CHECK_EQ(plan_knn_rows(c).band_rows, 60);
        CHECK_EQ(knn_shared_band_rows(1000, 4, c.knobs, 4), 100);
        CHECK_EQ(knn_shared_band_rows(80, 4, c.knobs, 4), 80);
    }
    {   // knn = 3 000 > 2 048: row by row whatever else holds; 50 000 query rows against 10 000 candidates: 4 GiB / 40 000 = 107 374
        // -> 50 000 rows; per row max(4 096 x 8 = 32 768, 3 x 3 001 x 4 = 36 012) bytes within 1 GiB: 29 816 rows
        CHECK_EQ(plan_items_pitch(3000), 4096);
        CHECK_EQ(plan_items_pitch(2048), 2048);
        const KnnRowsPlan P = plan_knn_rows(rows_call(10000, 0, 50000, 3000, false));
        CHECK(!P.symmetric);
        CHECK_EQ(P.band_rows, 29816);
        CHECK(P.overlap);
        CHECK(!plan_knn_rows(rows_call(1000000, 0, 1000000, 3000, true)).symmetric);
        KnnRowsCall ref = rows_call(10000, 0, 50000, 2048, false);   // the LDS forms: no cap, in either tie rule
        ref.ref_ties = true;
        CHECK_EQ(plan_knn_rows(ref).band_rows, 50000);
    }
    {   // column panels: max(32 768, up128(n_cand / 8)) columns; from 4 panels and rows x panel >= 16 Mi on
        KnnRowsCall c = rows_call(131072, 0, 512, 10, false);   // 131 072 / 8 = 16 384 -> 32 768 = n_cand / 4; 512 x 32 768 = 16 Mi
        CHECK_EQ(plan_knn_rows(c).band_rows, 512);              // (4 GiB / 524 288 = 8 192, clipped to the 512 rows)
        KnnPanels P = plan_knn_panels(c, 512);
        CHECK_EQ(P.panel, 32768);
        CHECK(P.eligible);
        CHECK_EQ(P.rows_per, 512);                              // min(512, 512 x 131 072 / 32 768 = 2 048) in whole 32s
        c.r1 = 511;
        CHECK(!plan_knn_panels(c, 511).eligible);               // 511 x 32 768 < 16 Mi
        c.r1 = 512;
        c.n_cand = 131071;
        CHECK_EQ(plan_knn_panels(c, 512).panel, 32768);
        CHECK(!plan_knn_panels(c, 512).eligible);               // fewer than 4 panels
        KnnRowsCall big = rows_call(1000000, 0, 100000, 10, false);   // 125 000 -> 125 056 columns; 4 GiB / 4 000 000 = 1 073 rows
        P = plan_knn_panels(big, 1073);
        CHECK_EQ(P.panel, 125056);
        CHECK(P.eligible);
        CHECK_EQ(P.rows_per, 8576);                             // 1 073 x 10^6 / 125 056 = 8 580 -> 8 576
        big.coreacc = true;
        CHECK(!plan_knn_panels(big, 1073).eligible);
        big.coreacc = false;
        big.both_comp = true;
        CHECK(!plan_knn_panels(big, 1073).eligible);
        big.both_comp = false;
        big.knn = 2049;
        CHECK(!plan_knn_panels(big, 1073).eligible);
        big.knn = 10;
        big.knobs.knn_prune = false;
        CHECK(!plan_knn_panels(big, 1073).eligible);
        // forced: SKL_KNN_PANEL = 300 -> 256 columns, any size with more candidates than one panel
        KnnRowsCall f = rows_call(1000, 0, 100, 10, false);
        f.knobs.knn_panel = 300;
        P = plan_knn_panels(f, 100);
        CHECK_EQ(P.panel, 256);
        CHECK(P.eligible);
        CHECK_EQ(P.rows_per, 96);                               // min(100, 100 x 1 000 / 256 = 390) -> 96
        f.knobs.knn_band_rows = 48;
        CHECK_EQ(plan_knn_panels(f, 48).rows_per, 48);
        f.n_cand = 257;
        CHECK(plan_knn_panels(f, 48).eligible);
        f.n_cand = 256;
        CHECK(!plan_knn_panels(f, 48).eligible);
        f.knobs.knn_panel = 100;                                // below one 128-column block: not forced, the size rule again
        CHECK_EQ(plan_knn_panels(f, 48).panel, 32768);
        CHECK(!plan_knn_panels(f, 48).eligible);
    }
}

// ---------------------------------------------------------------------------
// coverage: the planned merges replayed on the CPU
// ---------------------------------------------------------------------------
struct Replay {
    size_t n_rows, n_cols;
    std::vector<uint32_t> got;      // [row][col]: times row was fed candidate col
    std::vector<long long> last;    // per row: the last id it was fed
    bool ascending = true;
    Replay(size_t rows, size_t cols) : n_rows(rows), n_cols(cols), got(rows * cols, 0), last(rows, -1) {}
    void feed(const KnnMerge &m)
    {
        for (uint32_t r = 0; r < m.rows; ++r) {
            const size_t row = (size_t)m.state_row_base + r;
            if (row >= n_rows) {
                ascending = false;   // (a row that does not exist: reported through the same flag)
                continue;
            }
            for (uint32_t q = 0; q < m.cols; ++q) {
                const uint32_t id = m.id_base + q;
                if (id < m.skip_below) continue;
                if (m.self_id_base != 0xFFFFFFFFu && id == m.self_id_base + r) continue;
                if (id >= n_cols || (long long)id <= last[row]) ascending = false;
                else ++got[row * n_cols + id];
                last[row] = id;
            }
        }
    }
};

static KnnCall random_call(std::mt19937_64 &rng, KnnForm form, size_t n_rows, size_t n_cols, size_t band_rows)
{
    KnnCall c;
    c.form = form;
    c.n_rows = n_rows;
    c.n_cols = n_cols;
    c.band_rows = band_rows;
    c.knn = 1 + rng() % 40;
    c.win_hi = n_cols;
    c.row_hi = n_rows;
    c.coreacc = rng() % 2;
    c.ref = rng() % 2;
    c.overlap = rng() % 2;
    c.nk = 5;
    c.ss64 = 64;
    c.has_comp = rng() % 4 == 0;
    c.knobs.knn_row_flags = rng() % 8 != 0;
    c.knobs.knn_prune = rng() % 8 != 0;
    return c;
}

// every band of the call: the views fit the planned buffers; the merges go to `rp` in the planned order
static void run_call(const KnnCall &c, const std::vector<uint32_t> &bands, Replay &rp)
{
    const KnnCallPlan P = plan_knn_call(c);
    const size_t rec = c.rec();
    const int eb_lengths = P.eb_may_ask ? 3 : 0;
    CHECK_EQ(P.t_stride % 32, 0);
    CHECK(P.t_stride >= c.band_rows);
    size_t it = 0;
    for (const uint32_t band : bands) {
        const KnnBand B = plan_knn_band(c, P, band, it, eb_lengths);
        if (B.skip) continue;
        const size_t rows = B.b1 - B.b0;
        CHECK(B.b0 < B.b1 && B.b1 <= c.n_rows && rows <= c.band_rows);
        CHECK(B.col0 % 64 == 0 && B.col0 <= B.c_first && B.c_first < c.win_hi);
        CHECK_EQ(B.col0 + B.nB, c.win_hi);
        CHECK(rows * B.nB * rec <= P.key_band_bytes);
        CHECK(((size_t)B.nB / 64 + 1 + 31) / 32 <= P.bit_words);
        CHECK(c.band_rows * P.bit_words * sizeof(uint32_t) * (c.overlap ? 2 : 1) <= P.row_bits_bytes);
        CHECK((P.flags_half + c.win_hi) * sizeof(uint32_t) <= P.flags_bytes);   // flags indexed by column number, up to win_hi
        CHECK_EQ(B.has_turned, P.turned && B.t_first < c.win_hi);
        if (B.has_turned) {
            CHECK((c.win_hi - B.t_first) * P.t_stride * rec <= P.turned_band_bytes);
            CHECK(rows <= P.t_stride && rows <= (size_t)P.tbit_words * 32 * 32);   // a column's line and its marks hold the band's rows
            if (c.knobs.knn_row_flags) CHECK((P.turned_bits_half + c.win_hi * P.tbit_words) * sizeof(uint32_t) <= P.turned_bits_bytes);
        }
        if (P.prune) CHECK((P.prune_cols_at + (c.cross() ? B.col0 + B.nB : 0) + (c.cross() ? 0 : c.n_rows)) * sizeof(uint32_t) <= P.prune_bounds_bytes);
        CHECK_EQ(B.flag_value, it + 1);
        CHECK_EQ(B.eb_band, eb_lengths > 0 && (it >= 1 || c.lists_hold_knn));
        if (B.eb_band) CHECK(rows * B.nB * (size_t)eb_lengths * sizeof(uint16_t) <= knn_eb_counts_bytes(c, eb_lengths));
        if (B.plain_marks_nothing) CHECK(c.lists_hold_knn || it * c.band_rows >= c.knn);
        // the order of the tie mode: heaps take the turned copy first
        CHECK_EQ(B.merge[0].turned, c.ref);
        CHECK_EQ(B.merge[1].turned, !c.ref);
        for (const KnnMerge &m : B.merge) {
            CHECK_EQ(m.row_flags, m.turned);
            CHECK_EQ(m.stride, m.turned ? P.t_stride : (size_t)B.nB);
            CHECK(m.cols <= m.stride);
            rp.feed(m);
        }
        ++it;
    }
}

static void coverage(long cases)
{
    std::mt19937_64 rng(20261016);
    for (long x = 0; x < cases; ++x) {
        const size_t n = 2 + rng() % 330;
        const size_t band_rows = 1 + rng() % (x % 3 == 0 ? 20 : n + 10);
        const size_t total_bands = (n + band_rows - 1) / band_rows;
        std::vector<uint32_t> all(total_bands);
        for (size_t b = 0; b < total_bands; ++b) all[b] = (uint32_t)b;
        {   // SYMMETRIC, whole matrix: every row is fed every other sample once, in ascending order
            KnnCall c = random_call(rng, KNN_SYMMETRIC, n, n, band_rows);
            c.n_bands = total_bands;
            Replay rp(n, n);
            run_call(c, all, rp);
            bool once = true;
            for (size_t i = 0; i < n; ++i) for (size_t j = 0; j < n; ++j) once = once && rp.got[i * n + j] == (i == j ? 0u : 1u);
            CHECK(once);
            CHECK(rp.ascending);
        }
        {   // COLUMN WINDOWS cut on band boundaries (the last one ends at n), one (window, band) per call
            KnnCall c = random_call(rng, KNN_WINDOW, n, n, band_rows);
            c.ref = true;
            c.overlap = false;
            c.n_bands = 1;
            std::vector<size_t> cuts(1, 0);
            for (size_t b = 1; b < total_bands; ++b) if (rng() % 3 == 0) cuts.push_back(b * band_rows);
            cuts.push_back(n);
            Replay rp(n, n);
            for (size_t w = 0; w + 1 < cuts.size(); ++w) {
                c.win_lo = cuts[w];
                c.win_hi = cuts[w + 1];
                for (size_t b = 0; b < total_bands; ++b) {
                    c.lists_hold_knn = b >= 1 && band_rows >= c.knn;
                    run_call(c, std::vector<uint32_t>(1, (uint32_t)b), rp);
                }
            }
            bool once = true;
            for (size_t i = 0; i < n; ++i) for (size_t j = 0; j < n; ++j) once = once && rp.got[i * n + j] == (i == j ? 0u : 1u);
            CHECK(once);
            CHECK(rp.ascending);
        }
        {   // CROSS PANELS: rows [r0, r1) of n_rows against n columns, panel after panel
            const bool self_rows = rng() % 2;
            const size_t n_rows = self_rows ? n : 1 + rng() % 200;
            const size_t r0 = rng() % n_rows, r1 = r0 + 1 + rng() % (n_rows - r0);
            const size_t rows_per = 1 + rng() % (x % 2 ? 40 : n_rows + 5);
            const size_t panel = x % 4 == 0 ? 128 * (1 + rng() % 3) : 1 + rng() % (n + 20);   // (any width: the rule cuts 128s)
            std::vector<uint32_t> bands;
            for (size_t b = r0 / rows_per; b * rows_per < r1; ++b) bands.push_back((uint32_t)b);
            KnnCall c = random_call(rng, KNN_CROSS_PANEL, n_rows, n, rows_per);
            c.coreacc = false;
            c.self_rows = self_rows;
            c.row_lo = r0;
            c.row_hi = r1;
            c.n_bands = bands.size();
            c.overlap = c.overlap && bands.size() > 1;
            Replay rp(n_rows, n);
            for (size_t c0 = 0; c0 < n; c0 += panel) {
                c.win_lo = c0;
                c.win_hi = std::min(n, c0 + panel);
                run_call(c, bands, rp);
            }
            bool once = true;
            for (size_t i = 0; i < n_rows; ++i) {
                for (size_t j = 0; j < n; ++j) {
                    const uint32_t want = (i >= r0 && i < r1 && !(self_rows && i == j)) ? 1u : 0u;
                    once = once && rp.got[i * n + j] == want;
                }
            }
            CHECK(once);
            CHECK(rp.ascending);
        }
    }
}

static void agreement(long cases)
{
    std::mt19937_64 rng(7);
    Knobs knobs;
    for (long x = 0; x < cases; ++x) {
        const size_t n = 2 + rng() % (x % 2 ? 3000000 : 50000);
        const bool coreacc = rng() % 2;
        const size_t nk = 1 + rng() % 9;
        const size_t rec = coreacc_rec_with_counts(coreacc, nk, true);
        const size_t parts = 1 + rng() % 8;
        const size_t shared = knn_shared_band_rows(n, rec, knobs, parts);
        CHECK_EQ(shared, std::min(n, symmetric_band_rows(n, rec, KNN_SHARED_BUDGET, parts)));
        // one participant, single-k keys, 64 GiB free: the symmetric budget of plan_knn_rows() is min(32 GiB, 32 GiB), the fixed one
        if (!coreacc) {
            KnnRowsCall c = rows_call(n, 0, n, 1, true);
            c.free_bytes = 64 * GiB;
            const KnnRowsPlan P = plan_knn_rows(c);
            const size_t one = knn_shared_band_rows(n, rec, knobs, 1);
            CHECK_EQ(P.symmetric, one < n);
            if (P.symmetric) CHECK_EQ(P.band_rows, one);
        }
    }
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "pinned";
    const long count = argc > 2 ? atol(argv[2]) : 200;
    if (!strcmp(what, "pinned")) pinned();
    else if (!strcmp(what, "coverage")) coverage(count);
    else if (!strcmp(what, "agreement")) agreement(count);
    else {
        printf("usage: knn_plan_check pinned | coverage N | agreement N\n");
        return 2;
    }
    if (g_failed) {
        printf("FAILED %ld of %ld\n", g_failed, g_checks);
        return 1;
    }
    printf("ok %ld\n", g_checks);
    return 0;
}
