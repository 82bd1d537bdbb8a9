// within_check.cpp -- csrc/within_plan.hpp alone (no HIP header, no library): the numbers the pairs-within-a-cap filter launches
// with, its predicate, the (i, j) of a pair position, and within_select_host() -- the host restatement of csrc/within.hip's
// three kernels -- against a plain loop over the array.  Built by tests/test_within_plan_cpu.py with the host compiler under
// AddressSanitizer and UBSan and run directly.
//   consts                 chunk, wave span, scan step, threads, scan threads, band pair limit
//   plan M...              per M: chunks, scan steps, scratch bytes, accepted (1/0), band bytes at 2 columns and at 1
//   select                 the selection on random and special arrays  -> "ok <cases>"
//   locate                 (i, j) recovery                             -> "ok <positions>"
#include "within_plan.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

struct Rec {
    uint32_t i, j;
    float d0, d1;
};

// the plain loop: predicate as the header states it, (i, j) by walking the rows from the start of the pair space
static std::vector<Rec> plain(const std::vector<float> &dense, uint64_t m, uint32_t ncols, bool self_mode, uint64_t n, uint64_t first,
                              double max_first, double max_second, bool ani)
{
    std::vector<Rec> out;
    uint64_t i = 0, at = 0;   // row i starts at position `at`
    auto row_len = [&](uint64_t r) { return self_mode ? n - 1 - r : n; };
    for (uint64_t p = 0; p < m; ++p) {
        const uint64_t flat = first + p;
        while (flat >= at + row_len(i)) at += row_len(i++);
        const float v0 = dense[p * ncols], v1 = ncols == 2 ? dense[p * ncols + 1] : 0.0f;
        bool keep = ani ? v0 >= (float)(1.0 - max_first) : v0 <= (float)max_first;
        if (ncols == 2 && !std::isinf(max_second)) keep = keep && v1 <= (float)max_second;
        if (!keep) continue;
        const uint64_t pos = flat - at;
        out.push_back({(uint32_t)i, (uint32_t)(self_mode ? i + 1 + pos : pos), v0, v1});
    }
    return out;
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void one_select(const std::vector<float> &dense, uint64_t m, uint32_t ncols, bool self_mode, uint64_t n, uint64_t first,
                       double max_first, double max_second, bool ani, const char *what)
{
    const std::vector<Rec> want = plain(dense, m, ncols, self_mode, n, first, max_first, max_second, ani);
    WithinPred q;
    CHECK(within_pred_make(max_first, max_second, ani, ncols, &q), "%s: caps refused", what);
    const uint64_t caps[] = {0, want.size(), want.size() ? want.size() - 1 : 0, want.size() + 100, want.size() / 2};
    for (uint64_t cap : caps) {
        const float SENT = -77.0f;
        std::vector<uint32_t> oi(cap + 1, 0xABCDEF01u), oj(cap + 1, 0xABCDEF01u), counts;
        std::vector<float> od((cap + 1) * ncols, SENT);
        std::vector<uint64_t> offsets;
        const uint64_t found = within_select_host(dense.data(), m, ncols, self_mode, n, first, q, cap, oi.data(), oj.data(), od.data(), &counts, &offsets);
        CHECK(found == want.size(), "%s cap %llu: found %llu, expected %zu", what, (unsigned long long)cap, (unsigned long long)found, want.size());
        CHECK(counts.size() == within_chunks(m) && offsets.size() == counts.size(), "%s: %zu counts", what, counts.size());
        uint64_t sum = 0;
        for (size_t c = 0; c < counts.size(); ++c) {
            CHECK(offsets[c] == sum, "%s: offset of chunk %zu", what, c);
            sum += counts[c];
        }
        CHECK(sum == found, "%s: counts sum", what);
        const uint64_t written = std::min<uint64_t>(cap, found);
        for (uint64_t r = 0; r < written; ++r) {
            const bool ok = oi[r] == want[r].i && oj[r] == want[r].j && same_bits(od[r * ncols], want[r].d0) &&
                            (ncols == 1 || same_bits(od[r * ncols + 1], want[r].d1));
            CHECK(ok, "%s cap %llu: record %llu = (%u, %u), expected (%u, %u)", what, (unsigned long long)cap, (unsigned long long)r, oi[r], oj[r],
                  want[r].i, want[r].j);
            if (!ok) break;
        }
        for (uint64_t r = written; r < cap + 1; ++r) {   // nothing beyond the records is touched
            CHECK(oi[r] == 0xABCDEF01u && oj[r] == 0xABCDEF01u && od[r * ncols] == SENT && od[r * ncols + ncols - 1] == SENT, "%s cap %llu: slot %llu touched", what,
                  (unsigned long long)cap, (unsigned long long)r);
        }
    }
}

static int run_select()
{
    std::mt19937_64 rng(7);
    size_t cases = 0;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    struct Shape {
        bool self_mode;
        uint64_t n, r0, r1;   // rows [r0, r1) of the pair space
    };
    const Shape shapes[] = {{true, 2, 0, 1},     {true, 3, 0, 2},      {true, 65, 0, 64},   {true, 65, 0, 65 - 2}, {true, 66, 0, 65},
                            {true, 300, 17, 250}, {true, 300, 298, 299}, {false, 1, 0, 700},  {false, 63, 0, 40},    {false, 64, 3, 67},
                            {false, 65, 0, 100},  {true, 2100, 0, 2099}, {true, 2100, 0, 1}, {true, 2100, 5, 6}};
    for (const Shape &s : shapes) {
        auto before = [&](uint64_t r) { return s.self_mode ? r * s.n - r * (r + 1) / 2 : r * s.n; };
        const uint64_t first = before(s.r0), m = before(s.r1) - first;
        for (uint32_t ncols = 1; ncols <= 2; ++ncols) {
            std::vector<float> dense(m * ncols);
            std::uniform_real_distribution<float> u(0.0f, 1.0f);
            for (int kind = 0; kind < 6; ++kind) {
                for (float &x : dense) x = u(rng);
                double cap1 = 0.1, cap2 = INFINITY;
                if (kind == 1) cap1 = 2.0;                        // all pass
                if (kind == 2) cap1 = 0.0;                        // none pass (values are > 0 almost surely; 0 would be kept)
                if (kind == 3) {                                  // NaN-bearing: a NaN never passes, whichever column holds it
                    for (size_t x = 0; x < dense.size(); x += 5) dense[x] = nan;
                    cap1 = 0.5;
                    cap2 = ncols == 2 ? 0.5 : INFINITY;
                }
                if (kind == 4 && m) {                             // the cap equals a stored value: kept
                    cap1 = (double)dense[(m / 2) * ncols];
                    cap2 = 0.7;
                }
                if (kind == 5) {                                  // clustered: most chunks empty, a few full
                    for (float &x : dense) x = 1.0f;
                    for (uint64_t c = 0; c < within_chunks(m); c += 3) {
                        for (uint64_t p = c * WITHIN_CHUNK; p < m && p < (c + 1) * WITHIN_CHUNK; ++p) dense[p * ncols] = 0.01f, dense[p * ncols + ncols - 1] = 0.01f;
                    }
                    cap2 = 0.02;
                }
                char what[96];
                snprintf(what, sizeof what, "%s n=%llu rows [%llu, %llu) ncols=%u kind=%d", s.self_mode ? "self" : "cross", (unsigned long long)s.n,
                         (unsigned long long)s.r0, (unsigned long long)s.r1, ncols, kind);
                one_select(dense, m, ncols, s.self_mode, s.n, first, cap1, cap2, false, what);
                if (ncols == 1) one_select(dense, m, ncols, s.self_mode, s.n, first, kind == 1 ? 2.0 : 0.35, INFINITY, true, what);   // ANI: the test turns round
                cases += ncols == 1 ? 2 : 1;
            }
        }
    }
    // caps: NaN and a negative first cap are refused, a negative second cap is a cap nothing meets, infinity switches the column off
    WithinPred q;
    CHECK(!within_pred_make(NAN, 1.0, false, 2, &q) && !within_pred_make(0.1, NAN, false, 2, &q) && !within_pred_make(-1e-9, 1.0, false, 2, &q), "bad caps accepted");
    CHECK(within_pred_make(0.0, -1.0, false, 2, &q) && q.test_second == 1 && !within_keep(q, 0.0f, 0.0f), "negative second cap");
    CHECK(within_pred_make(0.25, INFINITY, false, 2, &q) && q.test_second == 0 && within_keep(q, 0.25f, nan) && !within_keep(q, nan, 0.0f), "second column off");
    CHECK(within_pred_make(0.25, INFINITY, false, 1, &q) && q.test_second == 0, "one column");
    CHECK(within_pred_make(0.1, 0.5, true, 1, &q) && q.ani == 1 && same_bits(q.first, (float)(1.0 - 0.1)) && within_keep(q, q.first, 0.0f) &&
              !within_keep(q, std::nextafter(q.first, 0.0f), 0.0f) && !within_keep(q, nan, 0.0f), "ANI bound");
    if (g_failed) return 1;
    printf("ok %zu\n", cases);
    return 0;
}

static size_t check_position(bool self_mode, uint64_t n, uint64_t flat, uint64_t want_i, uint64_t want_j)
{
    uint32_t row, pos, i, j;
    within_locate(self_mode, flat, n, &row, &pos);
    within_step(self_mode, n, row, pos, 0, &i, &j);
    CHECK(i == want_i && j == want_j, "n=%llu flat=%llu: (%u, %u), expected (%llu, %llu)", (unsigned long long)n, (unsigned long long)flat, i, j,
          (unsigned long long)want_i, (unsigned long long)want_j);
    return 1;
}

static int run_locate()
{
    size_t checked = 0;
    for (uint64_t n : {2ull, 3ull, 64ull, 65ull, 1000ull}) {
        // every row start and end (position 0 and the last position among them), and every step a wave can take from a start
        for (uint64_t i = 0; i + 1 < n; ++i) {
            const uint64_t start = within_row_start(i, n), len = n - 1 - i;
            checked += check_position(true, n, start, i, i + 1);
            checked += check_position(true, n, start + len - 1, i, n - 1);
        }
        const uint64_t pairs = n * (n - 1) / 2;
        for (uint64_t flat = 0; flat < pairs; flat += n < 100 ? 1 : 97) {   // stepping ahead from `flat` agrees with locating there
            uint32_t row, pos;
            within_locate(true, flat, n, &row, &pos);
            for (uint32_t ahead : {1u, 2u, 63u, 64u, 127u, WITHIN_WAVE_SPAN - 1u}) {
                if (flat + ahead >= pairs) continue;
                uint32_t i, j, r2, p2;
                within_step(true, n, row, pos, ahead, &i, &j);
                within_locate(true, flat + ahead, n, &r2, &p2);
                CHECK(i == r2 && j == r2 + 1 + p2, "n=%llu flat=%llu ahead=%u", (unsigned long long)n, (unsigned long long)flat, ahead);
                ++checked;
            }
        }
    }
    {   // a million samples: positions near 5e11, beyond what a float or a u32 holds
        const uint64_t n = 1000003;
        for (uint64_t i : {0ull, 1ull, 499999ull, 500000ull, 707107ull, 999990ull, 1000000ull, 1000001ull}) {   // (the last two: n - 3, n - 2)
            const uint64_t start = within_row_start(i, n), len = n - 1 - i;
            checked += check_position(true, n, start, i, i + 1);
            checked += check_position(true, n, start + len - 1, i, n - 1);
            checked += check_position(true, n, start + len / 2, i, i + 1 + len / 2);
            if (i + 2 < n) {   // a step across the row's end
                uint32_t row, pos, a, b;
                within_locate(true, start + len - 1, n, &row, &pos);
                within_step(true, n, row, pos, 1, &a, &b);
                CHECK(a == i + 1 && b == i + 2, "n=%llu row %llu: step into the next row", (unsigned long long)n, (unsigned long long)i);
                ++checked;
            }
        }
        CHECK(within_row_start(n - 2, n) + 1 == n * (n - 1) / 2 && n * (n - 1) / 2 > 500000000000ull, "the last position");
    }
    for (uint64_t nq : {1ull, 63ull, 64ull, 65ull, 1000003ull}) {   // cross: rows of nq
        for (uint64_t i : {0ull, 1ull, 77ull, 1999999ull}) {
            checked += check_position(false, nq, i * nq, i, 0);
            checked += check_position(false, nq, i * nq + nq - 1, i, nq - 1);
            uint32_t row, pos, a, b;
            within_locate(false, i * nq, nq, &row, &pos);
            within_step(false, nq, row, pos, WITHIN_WAVE_SPAN - 1, &a, &b);
            CHECK(a == i + (WITHIN_WAVE_SPAN - 1) / nq && b == (WITHIN_WAVE_SPAN - 1) % nq, "cross nq=%llu row %llu: a wave's last step", (unsigned long long)nq,
                  (unsigned long long)i);
            ++checked;
        }
    }
    if (g_failed) return 1;
    printf("ok %zu\n", checked);
    return 0;
}

int main(int argc, char **argv)
{
    const char *cmd = argc > 1 ? argv[1] : "";
    if (!strcmp(cmd, "consts")) {
        printf("%u %u %u %u %u %llu\n", WITHIN_CHUNK, WITHIN_WAVE_SPAN, WITHIN_SCAN_STEP, WITHIN_THREADS, WITHIN_SCAN_THREADS,
               (unsigned long long)WITHIN_BAND_PAIR_LIMIT);
        return 0;
    }
    if (!strcmp(cmd, "plan")) {
        for (int x = 2; x < argc; ++x) {
            const uint64_t m = strtoull(argv[x], nullptr, 10);
            const uint64_t chunks = within_chunks(m);
            printf("%llu %llu %llu %zu %d %zu %zu\n", (unsigned long long)m, (unsigned long long)chunks, (unsigned long long)within_scan_steps(chunks),
                   within_scratch_bytes(chunks), within_band_ok(m) ? 1 : 0, within_band_bytes(m, 2), within_band_bytes(m, 1));
        }
        return 0;
    }
    if (!strcmp(cmd, "select")) return run_select();
    if (!strcmp(cmd, "locate")) return run_locate();
    fprintf(stderr, "usage: within_check consts | plan M... | select | locate\n");
    return 2;
}
