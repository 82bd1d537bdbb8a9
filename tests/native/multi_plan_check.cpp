// multi_plan_check.cpp -- CPU check of csrc/host/multi_plan.hpp, the plan of the multi-device drivers (test infrastructure).
// Host compiler only: the header alone, no HIP header, no library, no device.
//   multi_plan_check pinned : cuts, deal, sizes and the order of the kNN forms derived BY HAND (the arithmetic stands beside each case)
//   multi_plan_check grid   : what every partition must satisfy, over n in 2..299 + {1000, 2829, 16000, 100003}, W in 1..8 and
//                             band_rows in {1, 2, 3, 16, 64, 100, 256, 1024}
//   multi_plan_check print  : the partitions of that grid, one per line, for tests/test_multi_plan_cpu.py to hold against
//                             multi_gpu.py:  C n band_rows W cuts.. | S n parts bounds.. | E n parts bounds.. | D n_bands W d bands..
// pinned and grid print one line per failed check and "ok <checks>" / "FAILED <failures> of <checks>"; the exit status says which.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>

#include "../../sketchlib.rust_amd/csrc/host/multi_plan.hpp"

using namespace skl_host::multi_plan;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                               \
    do {                                                                          \
        ++g_checks;                                                               \
        if (!(cond)) {                                                            \
            ++g_failed;                                                           \
            if (g_failed <= 40) printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                         \
    } while (0)

template <class T>
static bool is(const std::vector<T> &got, std::initializer_list<long long> want)
{
    if (got.size() != want.size()) return false;
    size_t i = 0;
    for (const long long w : want) {
        if ((long long)got[i++] != w) return false;
    }
    return true;
}

static void pinned()
{
    // cut r = round(n * sqrt(r / W) / band_rows) * band_rows, halves away from zero, held in [previous cut, n]
    // 257 * sqrt(.2, .4, .6, .8) = 114.9, 162.5, 199.1, 229.9; / 16 = 7.18, 10.16, 12.44, 14.37 -> 7, 10, 12, 14 bands
    CHECK(is(knn_window_cuts(257, 16, 5), {0, 112, 160, 192, 224, 257}));
    // 40 * sqrt(..) = 17.9, 25.3, 31.0, 35.8; / 16 = 1.12, 1.58, 1.94, 2.24 -> 1, 2, 2, 2: two empty windows in the middle
    CHECK(is(knn_window_cuts(40, 16, 5), {0, 16, 32, 32, 32, 40}));
    // 33 * sqrt(1/3, 2/3) = 19.1, 26.9; / 16 = 1.19, 1.68 -> 1, 2: the last window is the one row 32
    CHECK(is(knn_window_cuts(33, 16, 3), {0, 16, 32, 33}));
    // 47 * sqrt(r / 8) = 16.6, 23.5, 28.8, 33.2, 37.2, 40.7, 44.0; / 16 = 1.04, 1.47, 1.80, 2.08, 2.32, 2.54, 2.75
    // -> 1, 1, 2, 2, 2, 3, 3 bands; 3 bands = 48 > 47: clamped to n, so the windows of devices 6 and 7 are [47, 47), off a boundary
    CHECK(is(knn_window_cuts(47, 16, 8), {0, 16, 16, 32, 32, 32, 47, 47, 47}));
    // 5 * sqrt(1/4, 2/4, 3/4) = 2.5 (exactly), 3.54, 4.33 -> 3 (Python's round gives 2), 4, 4
    CHECK(is(knn_window_cuts(5, 1, 4), {0, 3, 4, 4, 5}));
    CHECK(is(knn_window_cuts(100, 16, 1), {0, 100}));

    // 7 bands over 3 devices: 0 1 2 go out, 3 4 5 come back (to devices 2 1 0), 6 goes out again
    CHECK(is(knn_band_deal(7, 3, 0), {0, 5, 6}));
    CHECK(is(knn_band_deal(7, 3, 1), {1, 4}));
    CHECK(is(knn_band_deal(7, 3, 2), {2, 3}));
    CHECK(knn_band_deal(2, 3, 2).empty());

    // 10 samples hold 45 pairs, rows of 9, 8, .., 1, 0; targets ceil(45 w / 3) = 15, 30: rows 0-1 hold 17, rows 0-3 hold 30
    CHECK(is(self_row_bounds(10, 3), {0, 2, 4, 10}));
    CHECK(is(even_bounds(10, 4), {0, 2, 5, 7, 10}));

    // sizes
    CHECK(knn_log_cap(1) == 64 && knn_log_cap(4) == 64 && knn_log_cap(5) == 80 && knn_log_cap(2048) == 32768);
    CHECK(knn_log_record_width(true) == 2 && knn_log_record_width(false) == 1);
    CHECK(knn_heap_wire_words(7, true) == 23 && knn_heap_wire_words(7, false) == 16);   // 3 x 7 + 2, 2 x 7 + 2
    // the host budget: n x cap x (width + 1) x 4 B <= 4 GiB = 4 294 967 296 B.  knn = 4: cap 64
    CHECK(knn_logs_fit_host(8388608, 4, false));     // single k: 512 B per row; 2^23 rows are 2^32 B exactly
    CHECK(!knn_logs_fit_host(8388609, 4, false));
    CHECK(knn_logs_fit_host(5592405, 4, true));      // core/accessory: 768 B per row; 5 592 405 rows are 4 294 967 040 B
    CHECK(!knn_logs_fit_host(5592406, 4, true));     // 4 294 967 808 B
    CHECK(knn_logs_fit_host(2097152, 16, false) && !knn_logs_fit_host(2097153, 16, false));   // cap 256: 2 048 B per row, 2^21 rows

    // the order of the forms.  first_knn_form(reference ties, knn, n, W, core/accessory, decoupled allowed)
    const KnnForm D = KnnForm::Decoupled, T = KnnForm::Travelling, B = KnnForm::Dealt, R = KnnForm::RowShards;
    const KnnGaveUp no_form = KnnGaveUp::NoForm, overflow = KnnGaveUp::LogOverflow;
    // reference ties: decoupled -> travelling (whatever the reason) -> row shards
    CHECK(first_knn_form(true, 10, 1000, 4, true, true) == D);
    CHECK(first_knn_form(true, 10, 1000, 4, false, true) == D);
    CHECK(next_knn_form(D, overflow) == T);
    CHECK(next_knn_form(D, no_form) == T);
    CHECK(next_knn_form(T, no_form) == R);
    CHECK(first_knn_form(true, 10, 1000, 4, true, false) == T);    // SKL_KNN_DECOUPLED=0
    CHECK(first_knn_form(true, 4, 8388608, 2, false, true) == D);  // the logs just fit ...
    CHECK(first_knn_form(true, 4, 8388609, 2, false, true) == T);  // ... and just do not
    CHECK(first_knn_form(true, 4, 5592405, 2, true, true) == D);
    CHECK(first_knn_form(true, 4, 5592406, 2, true, true) == T);
    // canonical ties: dealt -> row shards; the decoupled switch means nothing to them
    CHECK(first_knn_form(false, 10, 1000, 4, true, true) == B);
    CHECK(first_knn_form(false, 10, 1000, 4, false, false) == B);
    CHECK(next_knn_form(B, no_form) == R);
    // beyond 2 048 neighbours: row shards under either rule (reference ties are NOT offered the dealt form)
    CHECK(first_knn_form(true, 2048, 5000, 4, true, true) == D);   // 5 000 x 32 768 x 3 x 4 B = 1.97e9 B: fits
    CHECK(first_knn_form(true, 2048, 5000, 4, true, false) == T);
    CHECK(first_knn_form(false, 2048, 5000, 4, true, true) == B);
    CHECK(first_knn_form(true, 2049, 5000, 4, true, true) == R);
    CHECK(first_knn_form(true, 2049, 5000, 4, true, false) == R);
    CHECK(first_knn_form(false, 2049, 5000, 4, true, true) == R);
    // fewer than two samples under reference ties: row shards
    CHECK(first_knn_form(true, 1, 1, 2, true, true) == R);
    CHECK(first_knn_form(true, 1, 0, 2, false, false) == R);
    CHECK(first_knn_form(true, 1, 2, 2, true, true) == D);
    CHECK(first_knn_form(false, 1, 1, 2, true, true) == B);        // (the dealt form finds out for itself)
    // one device shares nothing
    CHECK(first_knn_form(true, 10, 1000, 1, true, true) == R);
    CHECK(first_knn_form(false, 10, 1000, 1, true, true) == R);
}

static const size_t BIG_N[] = {1000, 2829, 16000, 100003}, BAND_ROWS[] = {1, 2, 3, 16, 64, 100, 256, 1024};
template <class F>
static void over_grid(F f)
{
    for (size_t i = 2; i < 300 + sizeof BIG_N / sizeof *BIG_N; ++i) {
        const size_t n = i < 300 ? i : BIG_N[i - 300];
        for (size_t W = 1; W <= 8; ++W) {
            for (const size_t band_rows : BAND_ROWS) f(n, band_rows, W);
        }
    }
}

template <class T>
static bool ascending_to(const std::vector<T> &v, size_t parts, size_t n)
{
    if (v.size() != parts + 1 || v.front() != 0 || v.back() != n) return false;
    for (size_t i = 1; i < v.size(); ++i) {
        if (v[i] < v[i - 1]) return false;
    }
    return true;
}

static void grid()
{
    over_grid([](size_t n, size_t band_rows, size_t W) {
        const std::vector<size_t> cut = knn_window_cuts(n, band_rows, W);
        CHECK(ascending_to(cut, W, n));
        bool on_boundaries = true;
        for (size_t r = 1; r < W && r < cut.size(); ++r) on_boundaries = on_boundaries && (cut[r] % band_rows == 0 || cut[r] == n);
        CHECK(on_boundaries);
        // every band to one device, each device's bands ascending
        const size_t n_bands = (n + band_rows - 1) / band_rows;
        std::vector<int> owners(n_bands, 0);
        bool in_order = true;
        for (size_t d = 0; d < W; ++d) {
            const std::vector<uint32_t> mine = knn_band_deal(n_bands, W, d);
            for (size_t x = 0; x < mine.size(); ++x) {
                in_order = in_order && mine[x] < n_bands && (x == 0 || mine[x] > mine[x - 1]);
                if (mine[x] < n_bands) ++owners[mine[x]];
            }
        }
        CHECK(in_order);
        bool once = true;
        for (const int o : owners) once = once && o == 1;
        CHECK(once);
        if (band_rows == BAND_ROWS[0]) {
            CHECK(ascending_to(self_row_bounds(n, W), W, n));
            CHECK(ascending_to(even_bounds(n, W), W, n));
        }
    });
}

template <class T>
static void print_line(const char *head, const std::vector<T> &v)
{
    fputs(head, stdout);
    for (const T x : v) printf(" %" PRIu64, (uint64_t)x);
    putchar('\n');
}

static void print()
{
    std::set<std::pair<size_t, size_t>> dealt;
    over_grid([&](size_t n, size_t band_rows, size_t W) {
        char head[96];
        snprintf(head, sizeof head, "C %zu %zu %zu", n, band_rows, W);
        print_line(head, knn_window_cuts(n, band_rows, W));
        if (band_rows == BAND_ROWS[0]) {
            snprintf(head, sizeof head, "S %zu %zu", n, W);
            print_line(head, self_row_bounds(n, W));
            snprintf(head, sizeof head, "E %zu %zu", n, W);
            print_line(head, even_bounds(n, W));
        }
        const size_t n_bands = (n + band_rows - 1) / band_rows;
        if (!dealt.insert({n_bands, W}).second) return;   // (the deal depends on these two alone)
        for (size_t d = 0; d < W; ++d) {
            snprintf(head, sizeof head, "D %zu %zu %zu", n_bands, W, d);
            print_line(head, knn_band_deal(n_bands, W, d));
        }
    });
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "pinned";
    if (!strcmp(what, "print")) {
        print();
        return 0;
    }
    if (!strcmp(what, "pinned")) pinned();
    else if (!strcmp(what, "grid")) grid();
    else return 2;
    if (g_failed) printf("FAILED %ld of %ld\n", g_failed, g_checks);
    else printf("ok %ld\n", g_checks);
    return g_failed ? 1 : 0;
}
