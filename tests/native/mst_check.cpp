// mst_check.cpp -- csrc/mst_plan.hpp alone (no HIP header, no library): mst_forest_host(), the sequential restatement of a whole
// skl_self_mst call (csrc/mst.hip's min-edge kernel chunk by chunk and wave by wave, the two offers, the append, the hook, the
// round loop), against a plain Kruskal over the edges sorted by (w, i, j) with a union-find of its own.  Built by
// tests/test_mst_plan_cpu.py with the host compiler under AddressSanitizer and UBSan and run directly.
//   consts     empty word, round limit, scratch head bytes, the layout of n = 1000
//   keys       the key map: monotone, -0.0f == +0.0f, the way back                                          -> "ok <cases>"
//   forest     n in {0, 1, 2, 3, 65, 300, 2100}, one and two columns, both columns: random weights, three distinct values,
//              all equal (the star at 0), -0.0f among +0.0f, NaNs scattered, a cap that leaves a forest, a cap below every
//              weight, the path whose weights force the most rounds                                          -> "ok <cases>"
//   edges      mst_clusters_from_edges_host on prefixes of a tree, and its refusal of an index >= n          -> "ok <cases>"
#include "mst_plan.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
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

static const uint32_t SENT = 0xABCDEF01u;

struct Ref {
    std::vector<MstEdge> edges;
    std::vector<uint32_t> labels;
};

// Kruskal, plainly: every edge (not NaN, <= cap) sorted by (w, i, j) -- float comparison, under which -0.0f == +0.0f -- and taken
// when its ends are in different trees of a parent-array union-find; labels: the lowest index of each tree
static Ref kruskal(const std::vector<float> &dense, uint64_t n, uint32_t ncols, uint32_t column, float cap)
{
    std::vector<MstEdge> all;
    uint64_t p = 0;
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t j = i + 1; j < n; ++j, ++p) {
            const float w = dense[p * ncols + column];
            if (w <= cap) all.push_back(MstEdge{i, j, w});   // (false for a NaN)
        }
    }
    std::sort(all.begin(), all.end(), [](const MstEdge &a, const MstEdge &b) {
        if (a.w < b.w) return true;
        if (b.w < a.w) return false;
        return a.i != b.i ? a.i < b.i : a.j < b.j;
    });
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    Ref ref;
    for (const MstEdge &e : all) {
        const uint32_t a = find(e.i), b = find(e.j);
        if (a == b) continue;
        parent[a] = b;
        ref.edges.push_back(e);
    }
    std::vector<uint32_t> lowest(n, 0xFFFFFFFFu);
    for (uint32_t x = 0; x < n; ++x) lowest[find(x)] = std::min(lowest[find(x)], x);
    ref.labels.resize(n);
    for (uint32_t x = 0; x < n; ++x) ref.labels[x] = lowest[find(x)];
    return ref;
}

static uint32_t ceil_log2(uint64_t n)
{
    uint32_t r = 0;
    while ((1ull << r) < n) ++r;
    return r;
}

// one call against Kruskal; returns the rounds
static uint32_t one_call(const char *what, const std::vector<float> &dense, uint64_t n, uint32_t ncols, uint32_t column, double cap)
{
    MstPred q;
    CHECK(mst_pred_make(cap, column, &q), "%s: cap refused", what);
    const Ref ref = kruskal(dense, n, ncols, column, (float)cap);
    std::vector<MstEdge> got(n ? n : 1, MstEdge{SENT, SENT, -7.0f});   // room for n - 1 and a sentinel
    std::vector<uint32_t> labels(n + 1, SENT);
    uint64_t n_edges = 77;
    uint32_t rounds = 77;
    CHECK(mst_forest_host(dense.data(), n, ncols, q, got.data(), labels.data(), &n_edges, &rounds), "%s n=%llu: gave up", what, (unsigned long long)n);
    CHECK(n_edges == ref.edges.size(), "%s n=%llu ncols=%u column=%u: %llu edges, expected %zu", what, (unsigned long long)n, ncols, column,
          (unsigned long long)n_edges, ref.edges.size());
    bool same = n_edges == ref.edges.size();
    for (uint64_t r = 0; same && r < n_edges; ++r) {
        same = got[r].i == ref.edges[r].i && got[r].j == ref.edges[r].j && got[r].w == ref.edges[r].w && got[r].i < got[r].j;
        if (r && same) same = mst_edge_less(got[r - 1], got[r]);   // strictly ascending
    }
    CHECK(same, "%s n=%llu ncols=%u column=%u: the edge list differs from Kruskal's", what, (unsigned long long)n, ncols, column);
    uint64_t roots = 0;
    for (uint64_t x = 0; x < n; ++x) roots += labels[x] == x;
    CHECK(n_edges + roots == n, "%s: %llu edges + %llu components != %llu", what, (unsigned long long)n_edges, (unsigned long long)roots, (unsigned long long)n);
    CHECK(std::equal(ref.labels.begin(), ref.labels.end(), labels.begin()), "%s n=%llu: labels differ", what, (unsigned long long)n);
    CHECK(labels[n] == SENT, "%s: the element after the labels was touched", what);
    CHECK(n < 1 || n_edges == n - 1 || (got[n_edges].i == SENT && got[n_edges].w == -7.0f), "%s: a record beyond n_edges was touched", what);
    CHECK(rounds <= ceil_log2(n ? n : 1), "%s n=%llu: %u rounds", what, (unsigned long long)n, rounds);
    CHECK((rounds == 0) == (n_edges == 0), "%s: %u rounds for %llu edges", what, rounds, (unsigned long long)n_edges);
    return rounds;
}

// a dense array whose column `column` holds weight(i, j); the other column (two columns) holds noise with NaNs
template <typename F>
static std::vector<float> dense_of(uint64_t n, uint32_t ncols, uint32_t column, std::mt19937_64 &rng, F weight)
{
    const uint64_t m = n ? n * (n - 1) / 2 : 0;
    std::vector<float> d(m * ncols);
    std::uniform_real_distribution<float> noise(-1.0f, 1.0f);
    uint64_t p = 0;
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t j = i + 1; j < n; ++j, ++p) {
            for (uint32_t c = 0; c < ncols; ++c) d[p * ncols + c] = c == column ? weight(i, j) : (rng() % 5 ? noise(rng) : NAN);
        }
    }
    return d;
}

static int run_forest()
{
    std::mt19937_64 rng(2024);
    size_t cases = 0;
    const double INF = INFINITY;
    for (uint64_t n : {0ull, 1ull, 2ull, 3ull, 65ull, 300ull, 2100ull}) {
        for (uint32_t ncols = 1; ncols <= 2; ++ncols) {
            for (uint32_t column = 0; column < ncols; ++column) {
                std::uniform_real_distribution<float> uni(0.0f, 1.0f);
                const float three[3] = {0.25f, 0.5f, 0.75f};
                std::vector<float> d;
                d = dense_of(n, ncols, column, rng, [&](uint32_t, uint32_t) { return uni(rng); });
                one_call("random", d, n, ncols, column, INF);
                one_call("random, a cap that leaves a forest", d, n, ncols, column, 1.0 / (double)(n ? n : 1));
                one_call("random, a cap equal to a weight", d, n, ncols, column, d.empty() ? 0.5 : (double)d[(d.size() / ncols / 2) * ncols + column]);
                d = dense_of(n, ncols, column, rng, [&](uint32_t, uint32_t) { return 0.5f + 0.5f * uni(rng); });
                CHECK(one_call("a cap below every weight", d, n, ncols, column, 0.25) == 0, "a cap below every weight: rounds");
                d = dense_of(n, ncols, column, rng, [&](uint32_t, uint32_t) { return three[rng() % 3]; });
                one_call("three values", d, n, ncols, column, INF);
                one_call("three values, capped", d, n, ncols, column, 0.5);
                d = dense_of(n, ncols, column, rng, [&](uint32_t, uint32_t) { return 0.125f; });
                one_call("all equal", d, n, ncols, column, INF);
                if (n >= 2) {   // the star at sample 0, in one round
                    MstPred q;
                    mst_pred_make(INF, column, &q);
                    std::vector<MstEdge> got(n);
                    std::vector<uint32_t> labels(n);
                    uint64_t n_edges = 0;
                    uint32_t rounds = 0;
                    mst_forest_host(d.data(), n, ncols, q, got.data(), labels.data(), &n_edges, &rounds);
                    bool star = n_edges == n - 1 && rounds == 1;
                    for (uint64_t r = 0; star && r < n_edges; ++r) star = got[r].i == 0 && got[r].j == r + 1 && got[r].w == 0.125f;
                    CHECK(star, "all equal n=%llu: not the star at 0 in one round", (unsigned long long)n);
                }
                d = dense_of(n, ncols, column, rng, [&](uint32_t, uint32_t) { return rng() % 2 ? -0.0f : 0.0f; });
                one_call("signed zeros", d, n, ncols, column, INF);
                d = dense_of(n, ncols, column, rng, [&](uint32_t, uint32_t) { return rng() % 4 ? (rng() % 2 ? -0.0f : 0.0f) : three[rng() % 3] - 0.5f; });
                one_call("signed zeros among other values", d, n, ncols, column, INF);
                one_call("signed zeros among other values, cap 0", d, n, ncols, column, 0.0);
                d = dense_of(n, ncols, column, rng, [&](uint32_t, uint32_t) { return rng() % 3 ? uni(rng) : NAN; });
                one_call("NaNs scattered", d, n, ncols, column, INF);
                d = dense_of(n, ncols, column, rng, [&](uint32_t i, uint32_t j) { return (i + j) % 7 == 3 || i % 11 == 5 ? NAN : three[rng() % 3]; });
                one_call("NaN rows and diagonals", d, n, ncols, column, INF);
                d = dense_of(n, ncols, column, rng, [&](uint32_t, uint32_t) { return NAN; });
                CHECK(one_call("all NaN", d, n, ncols, column, INF) == 0, "all NaN: rounds");
                // the path 0 - 1 - ... - n-1 with w(k, k + 1) = the trailing zeros of k + 1: round r can only join blocks of 2^(r-1)
                // samples (and a shorter one at the end), so the call takes floor(log2 n) rounds -- the most any input can: a round
                // that adds an edge at least doubles the smallest component that still has an outgoing edge
                auto ruler = [](uint32_t i, uint32_t j) { return j == i + 1 ? (float)__builtin_ctz(j) : 100.0f; };
                d = dense_of(n, ncols, column, rng, ruler);
                for (double cap : {50.0, INF}) {
                    const uint32_t rounds = one_call("ruler path", d, n, ncols, column, cap);
                    const uint32_t most = n < 2 ? 0 : ceil_log2(n + 1) - 1;   // floor(log2 n)
                    CHECK(rounds == most, "ruler path n=%llu: %u rounds, expected %u", (unsigned long long)n, rounds, most);
                }
                cases += 16;
            }
        }
    }
    if (g_failed) return 1;
    printf("ok %zu\n", cases);
    return 0;
}

static int run_keys()
{
    size_t cases = 0;
    const float v[] = {-INFINITY, -3.0e38f, -1.0f, -1.0e-38f, -1.0e-45f, -0.0f, 0.0f, 1.0e-45f, 1.0e-38f, 0.5f, 1.0f, 3.0e38f, INFINITY};
    const size_t nv = sizeof v / sizeof v[0];
    for (size_t a = 0; a < nv; ++a) {
        for (size_t b = 0; b < nv; ++b) {
            CHECK((mst_key(v[a]) < mst_key(v[b])) == (v[a] < v[b]) && (mst_key(v[a]) == mst_key(v[b])) == (v[a] == v[b]), "key order of %g, %g", v[a], v[b]);
            ++cases;
        }
        CHECK(mst_key_weight(mst_key(v[a])) == v[a], "the way back of %g", v[a]);
        CHECK(mst_offer(mst_key(v[a]), 0xFFFFFFFEu) < MST_EMPTY, "an offer at %g reaches the empty word", v[a]);
    }
    const float back = mst_key_weight(mst_key(-0.0f));
    uint32_t bits;
    memcpy(&bits, &back, sizeof bits);
    CHECK(bits == 0u, "-0.0f comes back as +0.0f");
    std::mt19937_64 rng(3);
    for (int k = 0; k < 100000; ++k) {
        const uint32_t ua = (uint32_t)rng(), ub = (uint32_t)rng();
        float a, b;
        memcpy(&a, &ua, sizeof a);
        memcpy(&b, &ub, sizeof b);
        if (a != a || b != b) continue;
        CHECK((mst_key(a) < mst_key(b)) == (a < b) && (mst_key(a) == mst_key(b)) == (a == b), "key order of bits %08x, %08x", ua, ub);
        CHECK(mst_key_weight(mst_key(a)) == a, "the way back of bits %08x", ua);
        ++cases;
    }
    MstPred q;
    CHECK(!mst_pred_make(NAN, 0, &q) && !mst_pred_make(-1e-9, 0, &q) && mst_pred_make(0.0, 0, &q) && mst_pred_make(INFINITY, 1, &q), "caps");
    CHECK(mst_keep(q, NAN, 1.0f) && !mst_keep(q, 1.0f, NAN), "the predicate reads the chosen column alone");
    if (g_failed) return 1;
    printf("ok %zu\n", cases);
    return 0;
}

static int run_edges()
{
    std::mt19937_64 rng(9);
    size_t cases = 0;
    for (uint64_t n : {1ull, 2ull, 65ull, 300ull}) {
        std::uniform_real_distribution<float> uni(0.0f, 1.0f);
        const std::vector<float> d = dense_of(n, 1, 0, rng, [&](uint32_t, uint32_t) { return uni(rng); });
        const Ref tree = kruskal(d, n, 1, 0, INFINITY);
        for (double t : {-1.0, 0.0, 0.01, 0.05, 0.5, 2.0}) {
            std::vector<uint32_t> ei, ej;
            for (const MstEdge &e : tree.edges) {
                if (e.w <= (float)t) ei.push_back(e.i), ej.push_back(e.j);
            }
            const Ref want = kruskal(d, n, 1, 0, (float)t);   // the components of ALL pairs within t
            std::vector<uint32_t> labels(n + 1, SENT);
            uint64_t count = 0, roots = 0;
            CHECK(mst_clusters_from_edges_host(ei.data(), ej.data(), ei.size(), n, labels.data(), &count), "a valid edge list was refused");
            for (uint64_t x = 0; x < n; ++x) roots += want.labels[x] == x;
            CHECK(std::equal(want.labels.begin(), want.labels.end(), labels.begin()) && count == roots && labels[n] == SENT,
                  "n=%llu t=%g: the tree's prefix gives other clusters than all pairs within t", (unsigned long long)n, t);
            ++cases;
        }
        std::vector<uint32_t> ei = {0, (uint32_t)n}, ej = {0, 0}, labels(n, SENT);
        uint64_t count = 77;
        CHECK(!mst_clusters_from_edges_host(ei.data(), ej.data(), 2, n, labels.data(), &count) && count == 77 && labels[0] == SENT, "an index equal to n was accepted");
        CHECK(!mst_clusters_from_edges_host(ej.data(), ei.data(), 2, n, labels.data(), &count) && count == 77 && labels[0] == SENT, "an index equal to n was accepted (j)");
        ++cases;
    }
    if (g_failed) return 1;
    printf("ok %zu\n", cases);
    return 0;
}

int main(int argc, char **argv)
{
    const char *cmd = argc > 1 ? argv[1] : "";
    if (!strcmp(cmd, "consts")) {
        const MstLayout l = mst_layout(1000);
        printf("%d %u %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", MST_EMPTY == ~0ull, MST_MAX_ROUNDS, MST_SCRATCH_HEAD_BYTES, l.labels, l.best, l.comp_min,
               l.comp_hi, l.rec_i, l.rec_j, l.rec_w, l.bytes, l.fill_at, l.fill_bytes);
        return 0;
    }
    if (!strcmp(cmd, "keys")) return run_keys();
    if (!strcmp(cmd, "forest")) return run_forest();
    if (!strcmp(cmd, "edges")) return run_edges();
    fprintf(stderr, "usage: mst_check consts | keys | forest | edges\n");
    return 2;
}
