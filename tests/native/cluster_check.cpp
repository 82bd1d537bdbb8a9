// cluster_check.cpp -- csrc/cluster_plan.hpp alone (no HIP header, no library): cluster_labels_host(), the sequential
// restatement of csrc/cluster.hip's union, flatten and count kernels, the label check and the merge, against a brute-force
// component search over the band's passing pairs.  Built by tests/test_cluster_plan_cpu.py with the host compiler under
// AddressSanitizer and UBSan and run directly.
//   consts     threads of the per-sample kernels, scratch head bytes, sample limit
//   labels     bands of 1 and 2 columns: random graphs, all-pass, none-pass, star, paths in three orders, two paths joined by
//              their far ends, row ranges inside the triangle, chained ranges against the whole call   -> "ok <cases>"
//   merge      the merge and the label check                                                              -> "ok <cases>"
#include "cluster_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <utility>
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

typedef std::vector<std::pair<uint32_t, uint32_t>> Edges;
static const float PASS = 0.01f, FAIL = 0.9f;
static const double CAP = 0.05;

// brute force: relax label[i] = label[j] = min over every edge until nothing changes -- no union-find in sight
static std::vector<uint32_t> components(uint64_t n, const Edges &edges, std::vector<uint32_t> start = {})
{
    std::vector<uint32_t> lab(n);
    std::iota(lab.begin(), lab.end(), 0u);
    Edges all = edges;
    for (uint64_t i = 0; i < start.size(); ++i) all.push_back({(uint32_t)i, start[i]});
    for (bool changed = true; changed;) {
        changed = false;
        for (const auto &e : all) {
            const uint32_t lo = std::min(lab[e.first], lab[e.second]);
            if (lab[e.first] != lo || lab[e.second] != lo) {
                lab[e.first] = lab[e.second] = lo;
                changed = true;
            }
        }
    }
    return lab;
}

static uint64_t row_start(uint64_t r, uint64_t n) { return r * n - r * (r + 1) / 2; }   // (r <= n - 1)

// the dense band of rows [r0, r1) of n samples in which exactly `edges` pass (those of other rows are not in the band);
// two columns: the second passes everywhere, or fails on about every third edge when the second cap is tested
static std::vector<float> band_of(uint64_t n, uint64_t r0, uint64_t r1, uint32_t ncols, const Edges &edges, Edges *in_band, bool second_fails)
{
    const uint64_t first = row_start(r0, n), m = row_start(r1, n) - first;
    std::vector<float> dense(m * ncols, FAIL);
    if (ncols == 2) {
        for (uint64_t p = 0; p < m; ++p) dense[p * 2 + 1] = PASS;
    }
    for (const auto &e : edges) {
        const uint32_t i = std::min(e.first, e.second), j = std::max(e.first, e.second);
        if (i == j || i < r0 || i >= r1) continue;
        const uint64_t p = row_start(i, n) + (j - i - 1) - first;
        if (ncols == 2 && second_fails && (i * 31u + j) % 3u == 2u) {   // (a property of the pair, whatever band it is seen in)
            dense[p * 2] = PASS;
            dense[p * 2 + 1] = FAIL;      // the first column passes, the second does not: not an edge
            continue;
        }
        dense[p * ncols] = PASS;
        in_band->push_back({i, j});
    }
    return dense;
}

static size_t one_case(const char *what, uint64_t n, const Edges &edges)
{
    size_t cases = 0;
    const uint64_t rows = n ? n - 1 : 0;
    const uint64_t ranges[][2] = {{0, rows}, {rows / 3, rows}, {rows / 2, rows / 2 + 1}, {1, rows > 2 ? rows - 1 : rows}};
    for (uint32_t ncols = 1; ncols <= 2; ++ncols) {
        for (int second = 0; second < (ncols == 2 ? 2 : 1); ++second) {
            WithinPred q;
            CHECK(within_pred_make(CAP, second ? CAP : (double)INFINITY, false, ncols, &q), "%s: caps refused", what);
            for (const auto &rg : ranges) {
                const uint64_t r0 = std::min(rg[0], rows), r1 = std::max(r0, std::min(rg[1], rows));
                Edges in_band;
                const std::vector<float> dense = band_of(n, r0, r1, ncols, edges, &in_band, second != 0);
                const std::vector<uint32_t> want = components(n, in_band);
                std::vector<uint32_t> got(n + 1, 0xABCDEF01u);
                cluster_init_host(got.data(), n);
                const uint64_t count = cluster_labels_host(dense.data(), dense.size() / ncols, ncols, n, row_start(r0, n), q, got.data());
                uint64_t roots = 0;
                for (uint64_t i = 0; i < n; ++i) roots += want[i] == i;
                CHECK(std::equal(want.begin(), want.end(), got.begin()), "%s n=%llu ncols=%u rows [%llu, %llu): labels differ", what, (unsigned long long)n, ncols,
                      (unsigned long long)r0, (unsigned long long)r1);
                CHECK(count == roots, "%s: %llu clusters, expected %llu", what, (unsigned long long)count, (unsigned long long)roots);
                CHECK(got[n] == 0xABCDEF01u, "%s: the element after the labels was touched", what);
                CHECK(cluster_labels_ok_host(got.data(), n), "%s: the output fails the label check", what);
                ++cases;
            }
            // chained ranges give the whole call's labels, and the same ranges from the identity, merged, do too
            Edges all_in;
            const std::vector<float> whole = band_of(n, 0, rows, ncols, edges, &all_in, second != 0);
            const std::vector<uint32_t> want = components(n, all_in);
            std::vector<uint32_t> chained(n), merged(n);
            cluster_init_host(chained.data(), n);
            cluster_init_host(merged.data(), n);
            const uint64_t cuts[] = {0, rows / 5, rows / 5 + (rows > 1 ? 1 : 0), rows / 2, rows};
            uint64_t count = n, merged_count = n;
            for (int c = 0; c < 4; ++c) {
                const uint64_t r0 = cuts[c], r1 = std::max(cuts[c], cuts[c + 1]);
                Edges unused;
                const std::vector<float> dense = band_of(n, r0, r1, ncols, edges, &unused, second != 0);
                count = cluster_labels_host(dense.data(), dense.size() / ncols, ncols, n, row_start(r0, n), q, chained.data());
                std::vector<uint32_t> part(n);
                cluster_init_host(part.data(), n);
                cluster_labels_host(dense.data(), dense.size() / ncols, ncols, n, row_start(r0, n), q, part.data());
                CHECK(cluster_merge_host(merged.data(), part.data(), n, &merged_count), "%s: merge refused an output", what);
            }
            uint64_t roots = 0;
            for (uint64_t i = 0; i < n; ++i) roots += want[i] == i;
            CHECK(chained == want && count == roots, "%s n=%llu ncols=%u: chained ranges differ from the whole call", what, (unsigned long long)n, ncols);
            CHECK(merged == want && merged_count == roots, "%s n=%llu ncols=%u: merged ranges differ from the whole call", what, (unsigned long long)n, ncols);
            ++cases;
        }
    }
    return cases;
}

static Edges path(const std::vector<uint32_t> &order)
{
    Edges e;
    for (size_t k = 0; k + 1 < order.size(); ++k) e.push_back({order[k], order[k + 1]});
    return e;
}

static int run_labels()
{
    std::mt19937_64 rng(11);
    size_t cases = 0;
    for (uint64_t n : {2ull, 3ull, 65ull, 300ull, 2100ull}) {       // (2 100: rows wider than a chunk, bands of several chunks)
        Edges all, star;
        for (uint32_t i = 0; i < n; ++i) {
            for (uint32_t j = i + 1; j < n; ++j) all.push_back({i, j});
        }
        for (uint32_t j = 0; j < n; ++j) {
            if (j != n / 2) star.push_back({(uint32_t)(n / 2), j});   // the hub is not the lowest index
        }
        if (n <= 300) cases += one_case("all-pass", n, all);
        cases += one_case("none-pass", n, {});
        cases += one_case("star", n, star);
        for (double density : {0.3 / (double)n, 1.0 / (double)n, 3.0 / (double)n}) {
            Edges random;
            std::bernoulli_distribution coin(density);
            for (const auto &e : all) {
                if (coin(rng)) random.push_back(e);
            }
            cases += one_case("random", n, random);
        }
        std::vector<uint32_t> up(n), down(n), perm(n);
        std::iota(up.begin(), up.end(), 0u);
        down.assign(up.rbegin(), up.rend());
        perm = up;
        std::shuffle(perm.begin(), perm.end(), rng);
        cases += one_case("path ascending", n, path(up));
        cases += one_case("path descending", n, path(down));
        cases += one_case("path permuted", n, path(perm));
        if (n >= 65) {   // two paths, 0 .. h-1 and h .. n-1 in permuted order, joined by their far ends
            const uint32_t h = (uint32_t)(n / 2);
            std::vector<uint32_t> a(perm.begin(), perm.begin() + h), b(perm.begin() + h, perm.end());
            Edges two = path(a);
            const Edges second = path(b);
            two.insert(two.end(), second.begin(), second.end());
            two.push_back({a.back(), b.back()});
            cases += one_case("two paths joined", n, two);
        }
    }
    {   // n = 1 and n = 0: no pair space; the labels are finished and counted all the same
        uint32_t one[2] = {0, 0xABCDEF01u};
        WithinPred q;
        within_pred_make(CAP, INFINITY, false, 1, &q);
        CHECK(cluster_labels_host(nullptr, 0, 1, 1, 0, q, one) == 1 && one[0] == 0 && one[1] == 0xABCDEF01u, "n = 1");
        CHECK(cluster_labels_host(nullptr, 0, 2, 0, 0, q, nullptr) == 0, "n = 0");
        cases += 2;
    }
    if (g_failed) return 1;
    printf("ok %zu\n", cases);
    return 0;
}

static int run_merge()
{
    size_t cases = 0;
    {   // A links (0,1) and (2,3), B links (1,2): one cluster
        std::vector<uint32_t> a = {0, 0, 2, 2, 4}, b = {0, 1, 1, 3, 4};
        uint64_t count = 0;
        CHECK(cluster_merge_host(a.data(), b.data(), 4, &count) && count == 1, "A (0,1)(2,3) + B (1,2): %llu clusters", (unsigned long long)count);
        CHECK(a == (std::vector<uint32_t>{0, 0, 0, 0, 4}), "A (0,1)(2,3) + B (1,2): labels");   // (the fifth element lies outside n)
        ++cases;
    }
    {   // identity on either side; a partition with itself
        std::vector<uint32_t> id = {0, 1, 2, 3, 4, 5}, part = {0, 0, 2, 0, 2, 5};
        std::vector<uint32_t> x = id, y = part, z = part;
        uint64_t c1 = 0, c2 = 0, c3 = 0;
        CHECK(cluster_merge_host(x.data(), part.data(), 6, &c1) && x == part && c1 == 3, "identity + P");
        CHECK(cluster_merge_host(y.data(), id.data(), 6, &c2) && y == part && c2 == 3, "P + identity");
        CHECK(cluster_merge_host(z.data(), part.data(), 6, &c3) && z == part && c3 == 3, "P + P");
        cases += 3;
    }
    {   // random partitions in unflattened form (labels[i] <= i, chains allowed) against the brute force over both edge sets
        std::mt19937_64 rng(5);
        for (uint64_t n : {1ull, 2ull, 7ull, 64ull, 1000ull}) {
            for (int rep = 0; rep < 6; ++rep) {
                std::vector<uint32_t> a(n), b(n);
                for (uint64_t i = 0; i < n; ++i) {
                    a[i] = rng() % 3 ? (uint32_t)i : (uint32_t)(rng() % (i + 1));
                    b[i] = rng() % 4 ? (uint32_t)i : (uint32_t)(rng() % (i + 1));
                }
                CHECK(cluster_labels_ok_host(a.data(), n) && cluster_labels_ok_host(b.data(), n), "a valid input was refused");
                const std::vector<uint32_t> want = components(n, {}, a);
                Edges eb;
                for (uint64_t i = 0; i < n; ++i) eb.push_back({(uint32_t)i, b[i]});
                const std::vector<uint32_t> both = components(n, eb, a);
                std::vector<uint32_t> got = a;
                uint64_t count = 0, roots = 0;
                CHECK(cluster_merge_host(got.data(), b.data(), n, &count), "merge refused a valid input");
                for (uint64_t i = 0; i < n; ++i) roots += both[i] == i;
                CHECK(got == both && count == roots, "merge n=%llu rep %d", (unsigned long long)n, rep);
                // flatten alone gives the input's own components
                std::vector<uint32_t> flat = a;
                cluster_finish_host(flat.data(), n);
                CHECK(flat == want, "flatten n=%llu rep %d", (unsigned long long)n, rep);
                ++cases;
            }
        }
    }
    {   // the label check refuses labels[0] = 1, labels[3] = 7 and a value >= n, and the merge leaves both arrays untouched
        const uint64_t n = 8;
        const std::vector<uint32_t> good = {0, 0, 2, 2, 0, 5, 5, 7};
        struct Bad {
            uint32_t at, value;
        };
        for (const Bad &bad : {Bad{0, 1}, Bad{3, 7}, Bad{5, (uint32_t)n}, Bad{7, 0xFFFFFFFFu}}) {
            std::vector<uint32_t> broken = good;
            broken[bad.at] = bad.value;
            CHECK(!cluster_labels_ok_host(broken.data(), n), "labels[%u] = %u accepted", bad.at, bad.value);
            std::vector<uint32_t> a = broken, b = good;
            uint64_t count = 77;
            CHECK(!cluster_merge_host(a.data(), b.data(), n, &count) && a == broken && b == good && count == 77, "merge with a bad labels array");
            a = good, b = broken;
            CHECK(!cluster_merge_host(a.data(), b.data(), n, &count) && a == good && b == broken && count == 77, "merge with a bad other array");
            ++cases;
        }
        CHECK(cluster_labels_ok_host(good.data(), n) && cluster_labels_ok_host(nullptr, 0), "a valid array was refused");
    }
    if (g_failed) return 1;
    printf("ok %zu\n", cases);
    return 0;
}

int main(int argc, char **argv)
{
    const char *cmd = argc > 1 ? argv[1] : "";
    if (!strcmp(cmd, "consts")) {
        printf("%u %zu %llu\n", CLUSTER_THREADS, CLUSTER_SCRATCH_HEAD_BYTES, (unsigned long long)CLUSTER_MAX_SAMPLES);
        return 0;
    }
    if (!strcmp(cmd, "labels")) return run_labels();
    if (!strcmp(cmd, "merge")) return run_merge();
    fprintf(stderr, "usage: cluster_check consts | labels | merge\n");
    return 2;
}
