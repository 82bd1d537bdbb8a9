// hist_check.cpp -- csrc/hist_plan.hpp alone (no HIP header, no library): the grid's validation, the cell rule, and
// hist_host(), the sequential restatement of csrc/hist.hip's two kernels, against a plain loop over the array written here
// without the header's helpers.  Built by tests/test_hist_plan_cpu.py with the host compiler under AddressSanitizer and UBSan
// and run directly.
//   consts   threads, chunk, LDS cells, cell limit, LDS workgroups, global workgroups, scratch head bytes, peel rounds
//   grid     every refusal of hist_grid_make, and what an accepted grid holds                    -> "ok <cases>"
//   cell     the cell rule: the ends, one step beyond them, a monotone sweep, NaN, +-inf          -> "ok <cases>"
//   host     hist_host against the plain loop: 1 and 2 columns, both kernels' forms, every length  -> "ok <cases>"
#include "hist_plan.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

using namespace skl;

static size_t g_failed = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            ++g_failed;                                    \
            fprintf(stderr, "FAILED line %d: ", __LINE__); \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                         \
        }                                                  \
    } while (0)

static const double DNAN = std::numeric_limits<double>::quiet_NaN(), DINF = std::numeric_limits<double>::infinity();
static const float FNAN = std::numeric_limits<float>::quiet_NaN(), FINF = std::numeric_limits<float>::infinity();

static int run_grid()
{
    size_t cases = 0;
    const HistGrid untouched;   // (the defaults)
    auto refused = [&](double lo0, double hi0, uint32_t n0, double lo1, double hi1, uint32_t n1, uint32_t ncols, const char *what) {
        HistGrid g;
        CHECK(!hist_grid_make(lo0, hi0, n0, lo1, hi1, n1, ncols, &g), "%s accepted", what);
        CHECK(!memcmp(&g, &untouched, sizeof g), "%s: the grid was written", what);
        ++cases;
    };
    refused(0, 1, 0, 0, 1, 4, 2, "n0 == 0");
    refused(0, 1, 0, 0, 1, 4, 1, "n0 == 0, one column");
    refused(0, 1, 4, 0, 1, 0, 2, "n1 == 0 with two columns");
    for (uint32_t ncols = 1; ncols <= 2; ++ncols) {
        refused(DNAN, 1, 4, 0, 1, 4, ncols, "lo0 NaN");
        refused(0, DNAN, 4, 0, 1, 4, ncols, "hi0 NaN");
        refused(-DINF, 1, 4, 0, 1, 4, ncols, "lo0 -inf");
        refused(0, DINF, 4, 0, 1, 4, ncols, "hi0 +inf");
        refused(0, 1e39, 4, 0, 1, 4, ncols, "hi0 infinite as a float");
        refused(1, 1, 4, 0, 1, 4, ncols, "hi0 == lo0");
        refused(1, 0, 4, 0, 1, 4, ncols, "hi0 < lo0");
        refused(1.0, 1.0 + 1e-12, 4, 0, 1, 4, ncols, "hi0 == lo0 after rounding to float");
        refused(0, 1e-44, 1u << 20, 0, 1, 1, ncols, "a scale that is no finite float");
    }
    refused(0, 1, 4, DNAN, 1, 4, 2, "lo1 NaN");
    refused(0, 1, 4, 0, DNAN, 4, 2, "hi1 NaN");
    refused(0, 1, 4, -DINF, 1, 4, 2, "lo1 -inf");
    refused(0, 1, 4, 0, DINF, 4, 2, "hi1 +inf");
    refused(0, 1, 4, 1, 1, 4, 2, "hi1 == lo1");
    refused(0, 1, 4, 2, 1, 4, 2, "hi1 < lo1");
    refused(0, 1, 4, 0.5, 0.5 + 1e-12, 4, 2, "hi1 == lo1 after rounding to float");
    refused(0, 1, 1025, 0, 1, 1024, 2, "2^20 + 1024 cells");
    refused(0, 1, (1u << 20) + 1u, 0, 1, 1, 1, "2^20 + 1 cells in one column");
    refused(0, 1, 0xFFFFFFFFu, 0, 1, 0xFFFFFFFFu, 2, "2^64 - 2^33 + 1 cells (no wrap-around of the product)");

    HistGrid g;
    CHECK(hist_grid_make(0, 1, 1024, 0, 1, 1024, 2, &g) && hist_cells(g) == HIST_MAX_CELLS && !hist_in_lds(hist_cells(g)), "1024 x 1024 refused");
    CHECK(hist_grid_make(0, 1, 1u << 20, 0, 1, 1, 1, &g) && hist_cells(g) == HIST_MAX_CELLS, "2^20 x 1 refused");
    CHECK(hist_grid_make(0, 1, 128, 0, 1, 128, 2, &g) && hist_in_lds(hist_cells(g)), "128 x 128 is an LDS grid");
    CHECK(hist_grid_make(0, 1, 128, 0, 1, 129, 2, &g) && !hist_in_lds(hist_cells(g)), "128 x 129 is a global grid");
    // one column: the second column's fields are not looked at, whatever they hold
    CHECK(hist_grid_make(0.25, 0.75, 7, DNAN, -DINF, 0, 1, &g), "one column: garbage in the second column's fields refused");
    CHECK(g.ncols == 1 && g.n0 == 7 && g.n1 == 1 && hist_cells(g) == 7, "one column: n1 counts as 1");
    // bounds are rounded to float once, the scale's quotient is formed in double and rounded once
    CHECK(hist_grid_make(0.1, 0.7, 13, -0.05, 1.05, 9, 2, &g), "a plain grid refused");
    CHECK(g.lo0 == 0.1f && g.hi0 == 0.7f && g.scale0 == (float)(13.0 / ((double)0.7f - (double)0.1f)), "first column's floats");
    CHECK(g.lo1 == -0.05f && g.hi1 == 1.05f && g.scale1 == (float)(9.0 / ((double)1.05f - (double)-0.05f)) && g.n1 == 9 && g.ncols == 2, "second column's floats");
    cases += 8;
    if (g_failed) return 1;
    printf("ok %zu\n", cases);
    return 0;
}

static int run_cell()
{
    size_t cases = 0;
    struct Axis {
        double lo, hi;
        uint32_t n;
    };
    for (const Axis &ax : {Axis{0, 1, 8}, Axis{0, 1, 1}, Axis{-0.05, 1.05, 7}, Axis{0, 0.1, 16}, Axis{0.25, 0.26, 4096}, Axis{0, 1, 1u << 20},
                           Axis{-3e38, 3e38, 5}, Axis{1e-30, 2e-30, 3}}) {
        for (uint32_t ncols = 1; ncols <= 2; ++ncols) {
            // the axis under test is the first column, or the second beside a first column of one cell around 0.5
            for (uint32_t tested = 0; tested < ncols; ++tested) {
                HistGrid g;
                const bool made = tested == 0 ? hist_grid_make(ax.lo, ax.hi, ax.n, 0, 1, 1, ncols, &g) : hist_grid_make(0, 1, 1, ax.lo, ax.hi, ax.n, 2, &g);
                CHECK(made, "[%g, %g] / %u refused", ax.lo, ax.hi, ax.n);
                auto cell = [&](float v) { return tested == 0 ? hist_cell(g, v, 0.5f) : hist_cell(g, 0.5f, v); };
                const float lo = (float)ax.lo, hi = (float)ax.hi;
                CHECK(cell(lo) == 0u, "lo is not cell 0");
                CHECK(cell(hi) == ax.n - 1u, "hi is not the last cell: %u", cell(hi));
                CHECK(cell(std::nextafter(lo, -FINF)) == HIST_OUTSIDE && cell(std::nextafter(hi, FINF)) == HIST_OUTSIDE, "one step beyond an end is inside");
                CHECK(cell(std::nextafter(lo, FINF)) < ax.n && cell(std::nextafter(hi, -FINF)) < ax.n, "one step inside an end is outside");
                CHECK(cell(FINF) == HIST_OUTSIDE && cell(-FINF) == HIST_OUTSIDE, "an infinite value is inside");
                CHECK(cell(FNAN) == HIST_NAN, "a NaN is not counted as one");
                // monotone over a sweep of 1e5 values, every cell index below n, first 0 and last n - 1
                uint32_t before = 0;
                for (uint32_t x = 0; x <= 100000u; ++x) {
                    const float v = (float)((double)lo + ((double)hi - (double)lo) * (x / 100000.0));
                    const uint32_t c = cell(v < lo ? lo : (v > hi ? hi : v));
                    if (c >= ax.n || c < before) {
                        CHECK(false, "[%g, %g] / %u: value %u of the sweep gives cell %u after %u", ax.lo, ax.hi, ax.n, x, c, before);
                        break;
                    }
                    before = c;
                }
                CHECK(before == ax.n - 1u, "the sweep ends in cell %u", before);
                ++cases;
            }
        }
    }
    {   // two columns: the index is c0 * n1 + c1; a NaN in either column is a NaN, and wins over off-grid in the other
        HistGrid g;
        CHECK(hist_grid_make(0, 1, 8, 0, 2, 4, 2, &g), "grid refused");
        CHECK(hist_cell(g, 0.5f, 1.0f) == 4u * 4u + 2u && hist_cell(g, 1.0f, 2.0f) == 31u && hist_cell(g, 0.0f, 0.0f) == 0u, "c0 * n1 + c1");
        CHECK(hist_cell(g, 0.126f, 0.49f) == 1u * 4u + 0u && hist_cell(g, 0.124f, 0.51f) == 0u * 4u + 1u, "c0 * n1 + c1");
        CHECK(hist_cell(g, FNAN, 0.5f) == HIST_NAN && hist_cell(g, 0.5f, FNAN) == HIST_NAN && hist_cell(g, FNAN, FNAN) == HIST_NAN, "NaN in a column");
        CHECK(hist_cell(g, FNAN, 7.0f) == HIST_NAN && hist_cell(g, -3.0f, FNAN) == HIST_NAN && hist_cell(g, FINF, FNAN) == HIST_NAN, "NaN wins over off-grid");
        CHECK(hist_cell(g, 0.5f, 2.5f) == HIST_OUTSIDE && hist_cell(g, 1.5f, 1.0f) == HIST_OUTSIDE && hist_cell(g, -FINF, FINF) == HIST_OUTSIDE, "off-grid");
        // one column: the second value is not looked at
        CHECK(hist_grid_make(0, 1, 8, 0, 0, 0, 1, &g) && hist_cell(g, 0.5f, FNAN) == 4u && hist_cell(g, 0.5f, 99.0f) == 4u, "one column reads the second value");
        cases += 6;
    }
    if (g_failed) return 1;
    printf("ok %zu\n", cases);
    return 0;
}

// the plain loop: the header's cell rule written out again for one position, no helper of the header in sight
static void plain_loop(const std::vector<float> &dense, uint64_t m, uint32_t ncols, double lo0, double hi0, uint32_t n0, double lo1, double hi1,
                       uint32_t n1, std::vector<uint64_t> *counts, uint64_t *outside)
{
    const double lo[2] = {lo0, lo1}, hi[2] = {hi0, hi1};
    const uint32_t n[2] = {n0, ncols == 2 ? n1 : 1u};
    counts->assign((size_t)n[0] * n[1], 0u);
    outside[0] = outside[1] = 0;
    for (uint64_t p = 0; p < m; ++p) {
        bool nan = false, off = false;
        uint32_t c[2] = {0, 0};
        for (uint32_t x = 0; x < ncols; ++x) {
            const float v = dense[p * ncols + x], l = (float)lo[x], h = (float)hi[x];
            const float scale = (float)((double)n[x] / ((double)h - (double)l));
            if (std::isnan(v)) nan = true;
            else if (v < l || v > h) off = true;
            else {
                volatile float d = v - l;   // (volatile: two f32 operations, never one fused or widened one)
                volatile float s = d * scale;
                const float t = s;
                c[x] = t >= (float)n[x] ? n[x] - 1u : (uint32_t)t;
            }
        }
        if (nan) ++outside[1];
        else if (off) ++outside[0];
        else ++(*counts)[(size_t)c[0] * n[1] + c[1]];
    }
}

static int run_host()
{
    size_t cases = 0;
    std::mt19937_64 rng(20241021);
    std::uniform_real_distribution<float> wide(-0.2f, 1.2f);
    struct Grid {
        double lo0, hi0;
        uint32_t n0;
        double lo1, hi1;
        uint32_t n1;
    };
    // LDS grids (1 x 1, 8 x 8, exactly HIST_LDS_CELLS) and global ones (one column more, HIST_MAX_CELLS)
    const Grid grids[] = {{0, 1, 1, 0, 1, 1}, {0, 1, 8, 0, 1, 8}, {0, 0.1, 16, 0, 0.5, 4}, {0, 1, 128, 0, 1, 128}, {0, 1, 128, 0, 1, 129}, {0, 1, 1024, 0, 1, 1024}};
    const uint64_t lengths[] = {0, 1, 2, HIST_CHUNK - 1u, HIST_CHUNK, HIST_CHUNK + 1u, 3u * HIST_CHUNK + 7u};
    enum Fill { RANDOM, ONE_CELL, ENDS, WITH_NANS, FILLS };
    for (uint32_t ncols = 1; ncols <= 2; ++ncols) {
        for (const Grid &gr : grids) {
            HistGrid g;
            CHECK(hist_grid_make(gr.lo0, gr.hi0, gr.n0, gr.lo1, gr.hi1, gr.n1, ncols, &g), "grid refused");
            const uint64_t cells = hist_cells(g);
            CHECK(cells == (uint64_t)gr.n0 * (ncols == 2 ? gr.n1 : 1u), "cells");
            for (const uint64_t m : lengths) {
                for (int fill = 0; fill < FILLS; ++fill) {
                    std::vector<float> dense(m * ncols);
                    for (uint64_t p = 0; p < m; ++p) {
                        for (uint32_t x = 0; x < ncols; ++x) {
                            float v = wide(rng);
                            if (fill == ONE_CELL) v = 1.0f;                                   // the (1, 1) spike: all one cell (or all outside on the narrow grid)
                            if (fill == ENDS) v = (float)(p % 3 == 0 ? (x ? gr.lo1 : gr.lo0) : (p % 3 == 1 ? (x ? gr.hi1 : gr.hi0) : 0.05f));
                            if (fill == WITH_NANS && (p * 7u + x) % 5u == 0u) v = FNAN;
                            if (fill == WITH_NANS && (p * 3u + x) % 11u == 0u) v = p % 2 ? FINF : -FINF;
                            dense[p * ncols + x] = v;
                        }
                    }
                    std::vector<uint64_t> want;
                    uint64_t want_out[2];
                    plain_loop(dense, m, ncols, gr.lo0, gr.hi0, gr.n0, gr.lo1, gr.hi1, gr.n1, &want, want_out);
                    std::vector<uint64_t> got(cells + 1u, 0u);
                    got[cells] = 0xDEADBEEFull;   // (the element behind the counts)
                    uint64_t got_out[2] = {0, 0};
                    hist_host(dense.data(), m, g, got.data(), got_out);
                    CHECK(got[cells] == 0xDEADBEEFull, "the element behind the counts was written");
                    got.pop_back();
                    CHECK(got == want && got_out[0] == want_out[0] && got_out[1] == want_out[1], "ncols %u, %u x %u, m = %llu, fill %d: differs from the plain loop",
                          ncols, gr.n0, gr.n1, (unsigned long long)m, fill);
                    const uint64_t sum = std::accumulate(got.begin(), got.end(), (uint64_t)0);
                    CHECK(sum + got_out[0] + got_out[1] == m, "sum + outside + nan = %llu of %llu", (unsigned long long)(sum + got_out[0] + got_out[1]), (unsigned long long)m);
                    if (fill == ONE_CELL && m && gr.hi0 >= 1.0) CHECK(got[cells - 1u] == m, "the spike is not all in the last cell");
                    if (fill == WITH_NANS && m >= HIST_CHUNK - 1u) CHECK(got_out[1] > 0 && got_out[0] > 0 && sum > 0, "the NaN array holds none, or nothing else");
                    // hist_host ADDS: a second band doubles everything
                    hist_host(dense.data(), m, g, got.data(), got_out);
                    bool doubled = got_out[0] == 2 * want_out[0] && got_out[1] == 2 * want_out[1];
                    for (uint64_t x = 0; x < cells && doubled; ++x) doubled = got[x] == 2 * want[x];
                    CHECK(doubled, "a second band is not added");
                    ++cases;
                }
            }
        }
    }
    // the launch numbers: never more workgroups than chunks, bounded above, and the chunks of the lengths above
    CHECK(hist_chunks(0) == 0 && hist_chunks(1) == 1 && hist_chunks(HIST_CHUNK) == 1 && hist_chunks(HIST_CHUNK + 1u) == 2 && hist_chunks(3u * HIST_CHUNK + 7u) == 4, "chunks");
    CHECK(hist_groups(0, true) == 0 && hist_groups(3, true) == 3 && hist_groups(1u << 20, true) == HIST_LDS_GROUPS && hist_groups(1u << 20, false) == HIST_GLOBAL_GROUPS, "workgroups");
    CHECK(hist_scratch_bytes(0) == HIST_SCRATCH_HEAD_BYTES && hist_scratch_bytes(64) == HIST_SCRATCH_HEAD_BYTES + 512, "scratch bytes");
    if (g_failed) return 1;
    printf("ok %zu\n", cases);
    return 0;
}

int main(int argc, char **argv)
{
    const char *cmd = argc > 1 ? argv[1] : "";
    if (!strcmp(cmd, "consts")) {
        printf("%u %u %u %u %u %u %zu %u\n", HIST_THREADS, HIST_CHUNK, HIST_LDS_CELLS, HIST_MAX_CELLS, HIST_LDS_GROUPS, HIST_GLOBAL_GROUPS, HIST_SCRATCH_HEAD_BYTES,
               HIST_PEEL_ROUNDS);
        return 0;
    }
    if (!strcmp(cmd, "grid")) return run_grid();
    if (!strcmp(cmd, "cell")) return run_cell();
    if (!strcmp(cmd, "host")) return run_host();
    fprintf(stderr, "usage: hist_check consts | grid | cell | host\n");
    return 2;
}
