// dist_tables_check.cpp -- csrc/dist_tables.hpp alone (no HIP header, no library): the samebits -> Jaccard / ln J / distance / ANI
// tables every dense output rests on, against their defining properties and, bit for bit, against the oracle's C restatement of
// the reference's arithmetic (oracle/sketchlib_oracle.c, linked in by tests/test_dist_tables_cpu.py).  Build with -ffp-contract=off,
// as the library is.   dist_tables_check <ss64>...   prints "ok <checks>" or one line per failed check.
#include "../../sketchlib.rust_amd/csrc/dist_tables.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" {
#include "../../oracle/sketchlib_oracle.h"
}

using namespace skl;

static size_t g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                                 \
    do {                                                                 \
        ++g_checks;                                                      \
        if (!(cond)) {                                                   \
            if (++g_failed <= 40) {                                      \
                printf("line %d: %s: ", __LINE__, #cond);                \
                printf(__VA_ARGS__);                                     \
                printf("\n");                                            \
            }                                                            \
        }                                                                \
    } while (0)

static uint64_t bits(double x)
{
    uint64_t u;
    memcpy(&u, &x, sizeof u);
    return u;
}
static uint32_t bits(float x)
{
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return u;
}

static void check_size(size_t ss64)
{
    const size_t m = 64 * ss64 + 1;
    const uint32_t chance = (uint32_t)(64 * ss64) >> SKO_BBITS;   // matches two unrelated sketches are expected to share
    CHECK(TABLE_BBITS == SKO_BBITS, "%d", TABLE_BBITS);

    // the tolerance: ln(2 / (64 * 64 * ss64)), jaccard.rs:75
    const double tol = break_tolerance(ss64);
    CHECK(bits(tol) == bits(std::log(2.0 / (64.0 * 64.0 * (double)ss64))), "ss64 %zu: tolerance %a", ss64, tol);
    if (ss64 == 1) CHECK(bits(tol) == bits(std::log(1.0 / 2048.0)), "%a", tol);

    // ln J: its size, -inf up to the chance level, the oracle's J through the host's logarithm everywhere
    const LnjTable t = lnj_table(ss64);
    CHECK(t.lnj.size() == m, "ss64 %zu: %zu entries, expected %zu", ss64, t.lnj.size(), m);
    if (t.lnj.size() != m) return;
    for (size_t b = 0; b < m; ++b) {
        const double j = sko_jaccard_from_samebits((uint32_t)b, ss64, 0, 0.0, 0.0, 0.0);
        CHECK(bits(host_jaccard((uint32_t)b, ss64)) == bits(j), "ss64 %zu count %zu: J %a, oracle %a", ss64, b, host_jaccard((uint32_t)b, ss64), j);
        volatile double jv = j;   // a run-time call into libm
        CHECK(bits(t.lnj[b]) == bits(std::log(jv)), "ss64 %zu count %zu: ln J %a, expected %a", ss64, b, t.lnj[b], std::log(jv));
        if (b <= chance) CHECK(std::isinf(t.lnj[b]) && t.lnj[b] < 0.0, "ss64 %zu count %zu at or below chance (%u): %a", ss64, b, chance, t.lnj[b]);
        else CHECK(std::isfinite(t.lnj[b]) && t.lnj[b] <= 0.0, "ss64 %zu count %zu above chance (%u): %a", ss64, b, chance, t.lnj[b]);
        if (b > 0) CHECK(!(t.lnj[b] < t.lnj[b - 1]), "ss64 %zu count %zu: the table falls", ss64, b);
    }
    CHECK(t.lnj[m - 1] == 0.0, "ss64 %zu: every bin matches, ln J = %a", ss64, t.lnj[m - 1]);

    // min_alive: the first count whose entry is not below the tolerance, and no later entry is below it either
    size_t first = m;
    for (size_t b = 0; b < m; ++b) {
        if (!(t.lnj[b] < tol)) {
            first = b;
            break;
        }
    }
    CHECK(first < m && first > chance, "ss64 %zu: first count in the running %zu", ss64, first);
    CHECK(t.min_alive == (uint32_t)first, "ss64 %zu: min_alive %u, expected %zu", ss64, t.min_alive, first);
    for (size_t b = first; b < m; ++b) CHECK(!(t.lnj[b] < tol), "ss64 %zu count %zu: below the tolerance after min_alive", ss64, b);
    for (size_t b = 0; b < first; ++b) CHECK(t.lnj[b] < tol, "ss64 %zu count %zu: not below the tolerance before min_alive", ss64, b);

    // distance = 1 - J
    const std::vector<float> dist = dist_table(TABLE_JOUT_DIST, 21.0, ss64);
    CHECK(dist.size() == m, "ss64 %zu: %zu entries", ss64, dist.size());
    for (size_t b = 0; b < m && b < dist.size(); ++b) {
        const double j = sko_jaccard_from_samebits((uint32_t)b, ss64, 0, 0.0, 0.0, 0.0);
        CHECK(bits(dist[b]) == bits((float)(1.0 - j)), "ss64 %zu count %zu: distance %a", ss64, b, (double)dist[b]);
    }
    CHECK(dist[0] == 1.0f && dist[m - 1] == 0.0f, "ss64 %zu: distance ends %a %a", ss64, (double)dist[0], (double)dist[m - 1]);
    CHECK(dist_table(TABLE_JOUT_DIST, 31.0, ss64) == dist, "ss64 %zu: the distance does not depend on k", ss64);

    // ANI and its kNN key 1 - ANI, at three k-mer lengths: the oracle's ani_pois, clamped at 0
    for (const double k : {13.0, 21.0, 31.0}) {
        const std::vector<float> ani = dist_table(TABLE_JOUT_ANI, k, ss64), key = dist_table(2, k, ss64);
        CHECK(ani.size() == m && key.size() == m, "ss64 %zu k %g: %zu %zu entries", ss64, k, ani.size(), key.size());
        bool clamp_seen = false;
        for (size_t b = 0; b < m && b < ani.size() && b < key.size(); ++b) {
            const double a = sko_ani_pois(sko_jaccard_from_samebits((uint32_t)b, ss64, 0, 0.0, 0.0, 0.0), k);
            CHECK(bits(ani[b]) == bits((float)a), "ss64 %zu k %g count %zu: ANI %a, oracle %a", ss64, k, b, (double)ani[b], a);
            CHECK(bits(key[b]) == bits((float)(1.0 - a)), "ss64 %zu k %g count %zu: key %a", ss64, k, b, (double)key[b]);
            CHECK(ani[b] >= 0.0f && ani[b] <= 1.0f, "ss64 %zu k %g count %zu: ANI %a out of [0, 1]", ss64, k, b, (double)ani[b]);
            if (b <= chance) CHECK(bits(ani[b]) == bits(0.0f), "ss64 %zu k %g count %zu at or below chance: ANI %a", ss64, k, b, (double)ani[b]);
            // the unclamped form is negative here: the clamp, not the formula, gives the 0
            const double j = host_jaccard((uint32_t)b, ss64);
            if (1.0 + 1.0 / k * std::log((2.0 * j) / (1.0 + j)) < 0.0) {
                clamp_seen = true;
                CHECK(bits(ani[b]) == bits(0.0f) && bits(key[b]) == bits(1.0f), "ss64 %zu k %g count %zu: ANI %a not clamped", ss64, k, b, (double)ani[b]);
            }
        }
        CHECK(clamp_seen, "ss64 %zu k %g: no count reaches the clamp", ss64, k);
        CHECK(ani[m - 1] == 1.0f && key[m - 1] == 0.0f, "ss64 %zu k %g: identical sketches %a", ss64, k, (double)ani[m - 1]);
    }
}

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; ++i) check_size((size_t)strtoull(argv[i], nullptr, 10));
    if (g_failed) {
        printf("FAILED %zu of %zu\n", g_failed, g_checks);
        return 1;
    }
    printf("ok %zu\n", g_checks);
    return 0;
}
