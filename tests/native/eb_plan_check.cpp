// eb_plan_check.cpp -- CPU check of csrc/eb_plan.hpp, the early break's decision (test infrastructure).
// Host compiler only: no device header, no device, the library is never loaded.
//   eb_plan_check pinned       : geometry, costs, eb_best_lengths and eb_decide on inputs whose answer is derived BY HAND from the
//                                rules (the arithmetic stands beside each case)
//   eb_plan_check properties N : what every decision must satisfy, over N seeded random histograms
// Prints one line per failed check and "ok <checks>" / "FAILED <failures> of <checks>"; the exit status says which.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../sketchlib.rust_amd/csrc/eb_plan.hpp"

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

// Histograms of a whole geometry: block (r, c) is hist[(r * blk_cols + c) * 9 ...]; h[m] = sampled pairs that pass the test at
// exactly their first m lengths.
struct Hist {
    EbGeometry g;
    std::vector<uint32_t> v;
    explicit Hist(const EbGeometry &geo) : g(geo), v((size_t)geo.n_blocks() * EB_HIST, 0u) {}
    uint32_t *at(uint32_t r, uint32_t c) { return &v[((size_t)r * g.blk_cols + c) * EB_HIST]; }
    // a block between unrelated genomes: `alive` of its samples pass every one of the nk lengths, the rest none
    void cold(uint32_t r, uint32_t c, size_t nk, uint32_t alive)
    {
        at(r, c)[0] = g.samples - alive;
        at(r, c)[nk] = alive;
    }
    // a block within one species: every sampled pair passes every length
    void hot(uint32_t r, uint32_t c, size_t nk) { at(r, c)[nk] = g.samples; }
};

static void check_geometry(uint64_t n_rows, uint64_t n_cols, bool self, uint32_t shift_r, uint32_t shift_c, uint32_t blk_rows, uint32_t blk_cols,
                           uint32_t live, uint32_t samples)
{
    const EbGeometry g = eb_geometry(n_rows, n_cols, self);
    CHECK_EQ(g.self_mode, self);
    CHECK_EQ(g.shift_r, shift_r);
    CHECK_EQ(g.shift_c, shift_c);
    CHECK_EQ(g.blk_rows, blk_rows);
    CHECK_EQ(g.blk_cols, blk_cols);
    CHECK_EQ(g.live_blocks, live);
    CHECK_EQ(g.samples, samples);
}

static void pinned()
{
    // ---- applicability: switched on, 3..8 k-mer lengths, n_rows x n_cols >= 65 536
    CHECK(!eb_applicable(0, 5, 1000, 1000));
    CHECK(eb_applicable(1, 5, 1000, 1000) && eb_applicable(2, 5, 1000, 1000) && eb_applicable(7, 5, 1000, 1000));
    CHECK(!eb_applicable(1, 2, 1000, 1000) && eb_applicable(1, 3, 1000, 1000) && eb_applicable(1, 8, 1000, 1000) && !eb_applicable(1, 9, 1000, 1000));
    CHECK(eb_applicable(1, 5, 256, 256));      // 65 536
    CHECK(!eb_applicable(1, 5, 255, 256));     // 65 280
    CHECK(eb_applicable(1, 5, 1, 65536) && !eb_applicable(1, 5, 1, 65535));
    CHECK_EQ(EB_PLANS_KEPT, 8);

    // ---- the cost of a completion: 60 beyond 1 023 chunks, 12 from 48 Mi = 50 331 648 pairs, else 20
    CHECK(eb_cost(1024, 1000, 1000, true) == 60.0 && eb_cost(1563, 100000, 100000, false) == 60.0);
    CHECK(eb_cost(1023, 10033, 10033, true) == 20.0);   // 10 033 x 10 032 / 2 = 50 325 528 < 50 331 648
    CHECK(eb_cost(1023, 10034, 10034, true) == 12.0);   // 10 034 x 10 033 / 2 = 50 335 561
    CHECK(eb_cost(64, 8192, 6144, false) == 12.0);      // 8 192 x 6 144 = 50 331 648 exactly
    CHECK(eb_cost(64, 8192, 6143, false) == 20.0);
    CHECK(eb_cost(64, 8192, 8192, true) == 20.0);       // the triangle of 8 192: 33 550 336

    // ---- geometry.  shift: the smallest s >= 8 with ceil(n / 2^s) <= 64; samples = max(128, ceil(4 096 / live blocks))
    check_geometry(256, 256, true, 8, 8, 1, 1, 1, 4096);          // one block: 4 096 samples
    check_geometry(256, 256, false, 8, 8, 1, 1, 1, 4096);
    check_geometry(257, 257, true, 8, 8, 2, 2, 3, 1366);          // 2 x 3 / 2 = 3 live; ceil(4 096 / 3) = 1 366
    check_geometry(257, 257, false, 8, 8, 2, 2, 4, 1024);
    check_geometry(1024, 1024, true, 8, 8, 4, 4, 10, 410);        // ceil(4 096 / 10) = 410
    check_geometry(16384, 16384, true, 8, 8, 64, 64, 2080, 128);  // 64 x 65 / 2 = 2 080 live; ceil(4 096 / 2 080) = 2 -> 128
    check_geometry(16384, 16384, false, 8, 8, 64, 64, 4096, 128);
    check_geometry(16385, 16385, true, 9, 9, 33, 33, 561, 128);   // 65 blocks of 256 > 64: 512 per block, ceil(16 385 / 512) = 33; 33 x 34 / 2
    check_geometry(16385, 16385, false, 9, 9, 33, 33, 1089, 128);
    check_geometry(1000000, 1000000, true, 14, 14, 62, 62, 1953, 128);   // 2^13: 123 blocks; 2^14 = 16 384: ceil(1 000 000 / 16 384) = 62; 62 x 63 / 2
    check_geometry(1000000, 1000000, false, 14, 14, 62, 62, 3844, 128);
    check_geometry(1000, 20000, false, 8, 9, 4, 40, 160, 128);    // each side its own shift: ceil(20 000 / 256) = 79 > 64, ceil(20 000 / 512) = 40
    check_geometry(1024, 2048, false, 8, 8, 4, 8, 32, 128);       // 4 096 / 32 = 128 exactly
    check_geometry(512, 768, false, 8, 8, 2, 3, 6, 683);          // ceil(4 096 / 6) = 683

    // ---- eb_best_lengths: ke of {2, 3, 4} below nk minimising ke + cost x share(ke), share(ke) = (h[ke] + ... + h[8]) / total, taken if
    // at most 0.9 nk; ties go to the later ke (<=).  The completion cost is a parameter: 16 makes every figure below exact in binary.
    {
        const uint32_t none[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        double share = -1.0;
        CHECK_EQ(eb_best_lengths(none, 0, 5, 20.0, &share), 0);   // an empty histogram decides nothing
        CHECK(share == -1.0);
    }
    {   // nk = 3: only ke = 2 is below nk.  total 128, 4 alive at 3 lengths: 2 + 16 x 4 / 128 = 2.5 <= 2.7
        const uint32_t h[9] = {124, 0, 0, 4, 0, 0, 0, 0, 0};
        double share = -1.0;
        CHECK_EQ(eb_best_lengths(h, 128, 3, 16.0, &share), 2);
        CHECK(share == 0.03125);
        const uint32_t h2[9] = {120, 0, 0, 8, 0, 0, 0, 0, 0};   // 2 + 16 x 8 / 128 = 3.0 > 2.7: every length
        CHECK_EQ(eb_best_lengths(h2, 128, 3, 16.0, nullptr), 0);
    }
    {   // an exact tie of ke = 2 and ke = 3 (nk = 5): h[2] = 8 of 128: cost(2) = 2 + 16 x 8 / 128 = 3.0, cost(3) = 3 + 0 = 3.0: the later wins
        const uint32_t h[9] = {120, 0, 8, 0, 0, 0, 0, 0, 0};
        double share = -1.0;
        CHECK_EQ(eb_best_lengths(h, 128, 5, 16.0, &share), 3);
        CHECK(share == 0.0);
        const uint32_t h7[9] = {121, 0, 7, 0, 0, 0, 0, 0, 0};   // cost(2) = 2.875 < cost(3) = 3.0
        CHECK_EQ(eb_best_lengths(h7, 128, 5, 16.0, &share), 2);
        CHECK(share == 0.0546875);   // 7 / 128
    }
    {   // the 0.9 nk margin at nk = 5: 4.5.  Cost 20: 16 of 128 alive at all 5 lengths: 2 + 20 x 0.125 = 4.5, taken (<=); cost(3) = 5.5
        const uint32_t at[9] = {112, 0, 0, 0, 0, 16, 0, 0, 0};
        CHECK_EQ(eb_best_lengths(at, 128, 5, 20.0, nullptr), 2);
        const uint32_t above[9] = {111, 0, 0, 0, 0, 17, 0, 0, 0};   // 2 + 20 x 17 / 128 = 4.65625 > 4.5
        CHECK_EQ(eb_best_lengths(above, 128, 5, 20.0, nullptr), 0);
    }
    {   // `preferred` (the blocks' common choice) stands within 0.5 of the block's own best.  Cost 16, total 128, nk = 5:
        // h[2] = 6, h[5] = 2: cost(2) = 2 + 16 x 8 / 128 = 3.0, cost(3) = 3 + 16 x 2 / 128 = 3.25, cost(4) = 4.25: own best 2
        const uint32_t h[9] = {120, 0, 6, 0, 0, 2, 0, 0, 0};
        double share = -1.0;
        CHECK_EQ(eb_best_lengths(h, 128, 5, 16.0, &share), 2);
        CHECK_EQ(eb_best_lengths(h, 128, 5, 16.0, &share, nullptr, 0.0, 3), 3);   // 3.25 <= 3.0 + 0.5
        CHECK(share == 0.0625);                                                     // (the share reported stays the own best's: 8 / 128)
        CHECK_EQ(eb_best_lengths(h, 128, 5, 16.0, nullptr, nullptr, 0.0, 4), 2);  // 4.25 > 3.5: refused
        CHECK_EQ(eb_best_lengths(h, 128, 5, 16.0, nullptr, nullptr, 0.0, 5), 2);  // not a choice at all (> 4, and not below nk)
        const uint32_t at[9] = {120, 0, 4, 0, 0, 4, 0, 0, 0};     // cost(2) = 3.0, cost(3) = 3 + 16 x 4 / 128 = 3.5: exactly 0.5 away, taken
        CHECK_EQ(eb_best_lengths(at, 128, 5, 16.0, nullptr, nullptr, 0.0, 3), 3);
        const uint32_t beyond[9] = {120, 0, 3, 0, 0, 5, 0, 0, 0}; // cost(2) = 3.0, cost(3) = 3.625
        CHECK_EQ(eb_best_lengths(beyond, 128, 5, 16.0, nullptr, nullptr, 0.0, 3), 2);
        // refused when its own cost exceeds 0.9 nk, however close: nk = 4 (3.6): h[2] = 4, h[4] = 6: cost(2) = 2 + 16 x 10 / 128 = 3.25,
        // cost(3) = 3 + 16 x 6 / 128 = 3.75 <= 3.25 + 0.5 but > 3.6
        const uint32_t dear[9] = {118, 0, 4, 0, 6, 0, 0, 0, 0};
        CHECK_EQ(eb_best_lengths(dear, 128, 4, 16.0, &share, nullptr, 0.0, 3), 2);
        CHECK(share == 0.078125);   // 10 / 128
    }

    // ---- the forced decision: that many lengths when below nk, else none; never a table
    CHECK(eb_forced(3, 5).lengths == 3 && eb_forced(2, 3).lengths == 2 && eb_forced(5, 5).lengths == 0 && eb_forced(7, 5).lengths == 0);
    CHECK(!eb_forced(3, 5).mixed && eb_forced(3, 5).block_ke.empty() && eb_forced(3, 5).alive_share == 0.0);

    // ---- eb_decide.  nk = 5, cost 20 unless stated.
    {   // one live block (n = 256): the pooled decision is the decision.  40 of 4 096 alive: 2 + 20 x 40 / 4 096 = 2.195; cost(3) the same + 1
        Hist h(eb_geometry(256, 256, true));
        h.cold(0, 0, 5, 40);
        const EbDecision d = eb_decide(h.g, 5, 20.0, h.v.data());
        CHECK_EQ(d.lengths, 2);
        CHECK(!d.mixed && d.block_ke.empty());
        CHECK(d.alive_share == 0.009765625);   // 40 / 4 096
    }
    {   // all blocks unrelated (n = 1 024: 4 x 4, 10 live, 410 samples): 4 alive per block: 2 + 20 x 4 / 410 = 2.195 everywhere: one mind
        Hist h(eb_geometry(1024, 1024, true));
        for (uint32_t r = 0; r < 4; ++r) {
            for (uint32_t c = r; c < 4; ++c) h.cold(r, c, 5, 4);
        }
        const EbDecision d = eb_decide(h.g, 5, 20.0, h.v.data());
        CHECK_EQ(d.lengths, 2);
        CHECK(!d.mixed && d.block_ke.empty());
        CHECK(d.alive_share == 40.0 / 4100.0);   // pooled: 40 of 4 100
    }
    {   // all related: every sampled pair passes every length: 2 + 20 x 1 = 22 > 4.5 in every block and pooled: every length
        Hist h(eb_geometry(1024, 1024, true));
        for (uint32_t r = 0; r < 4; ++r) {
            for (uint32_t c = r; c < 4; ++c) h.hot(r, c, 5);
        }
        const EbDecision d = eb_decide(h.g, 5, 20.0, h.v.data());
        CHECK_EQ(d.lengths, 0);
        CHECK(!d.mixed && d.block_ke.empty() && d.alive_share == 0.0);
    }
    {   // half one species, (512, -512) at 256 per block: 4 x 4.  Blocks (0, 0), (0, 1), (1, 1) lie within the species, the other
        // 7 live blocks do not (4 of 410 alive).  Pass 1: the 7 take the break, the 3 do not.  Pool of the 7: common choice 2.  Pass 2,
        // a species block pulled towards the pool: (410 + 410 x 4 / 410) / 820 = 0.505: 2 + 20 x 0.505 = 12.1 > 4.5: every length.
        // Pooled over all 10: (3 x 410 + 28) / 4 100 = 0.307: 8.1 > 4.5: the kNN drivers' answer is "no early break".
        Hist h(eb_geometry(1024, 1024, true));
        for (uint32_t r = 0; r < 4; ++r) {
            for (uint32_t c = r; c < 4; ++c) {
                if (c < 2) h.hot(r, c, 5); else h.cold(r, c, 5, 4);
            }
        }
        const EbDecision d = eb_decide(h.g, 5, 20.0, h.v.data());
        CHECK(d.mixed);
        CHECK_EQ(d.lengths, 0);
        const uint8_t expect[16] = {5, 5, 2, 2,
                                    5, 5, 2, 2,    // (1, 0) mirrors (0, 1)
                                    2, 2, 2, 2,    // below the diagonal: the mirror of the blocks above
                                    2, 2, 2, 2};
        CHECK_EQ(d.block_ke.size(), 16);
        if (d.block_ke.size() == 16) {
            CHECK(memcmp(d.block_ke.data(), expect, 16) == 0);
            for (uint32_t r = 0; r < 4; ++r) {
                for (uint32_t c = 0; c < 4; ++c) CHECK_EQ(d.block_ke[r * 4 + c], d.block_ke[c * 4 + r]);
            }
        }
    }
    {   // cross mode, 512 x 768: 2 x 3 blocks, all live, 683 samples; block (1, 0) within a species: no mirror, (0, 1) keeps its own
        Hist h(eb_geometry(512, 768, false));
        for (uint32_t r = 0; r < 2; ++r) {
            for (uint32_t c = 0; c < 3; ++c) h.cold(r, c, 5, 6);   // 2 + 20 x 6 / 683 = 2.18
        }
        h.at(1, 0)[0] = 0;
        h.at(1, 0)[5] = 0;
        h.hot(1, 0, 5);
        const EbDecision d = eb_decide(h.g, 5, 20.0, h.v.data());
        const uint8_t expect[6] = {2, 2, 2, 5, 2, 2};
        CHECK(d.mixed && d.block_ke.size() == 6 && memcmp(d.block_ke.data(), expect, 6) == 0);
        // a block the sampler found no pair for decides nothing: every length, and so the blocks differ
        Hist z(eb_geometry(512, 768, false));
        for (uint32_t r = 0; r < 2; ++r) {
            for (uint32_t c = 0; c < 3; ++c) z.cold(r, c, 5, 6);
        }
        z.at(0, 2)[0] = 0;
        z.at(0, 2)[5] = 0;
        const EbDecision e = eb_decide(z.g, 5, 20.0, z.v.data());
        const uint8_t expect_z[6] = {2, 2, 5, 2, 2, 2};
        CHECK(e.mixed && e.block_ke.size() == 6 && memcmp(e.block_ke.data(), expect_z, 6) == 0);
        CHECK_EQ(e.lengths, 2);   // (pooled over the 5 blocks with samples)
        // no sample anywhere: no early break, one mind
        const Hist none(eb_geometry(512, 768, false));
        const EbDecision n = eb_decide(none.g, 5, 20.0, none.v.data());
        CHECK(!n.mixed && n.lengths == 0 && n.block_ke.empty());
    }
    {   // the prior.  1 024 x 2 048 cross: 32 blocks of 128 samples.  31 blocks: 1 pair alive at all lengths (2 + 20 / 128 = 2.16: ke 2).
        // One block: 9 of 128 (7 %) alive at exactly 2 lengths: by itself cost(2) = 2 + 20 x 9 / 128 = 3.41, cost(3) = 3 + 0: ke 3.
        // Every block takes the break, so the pool is all 4 096 samples: shares 9 / 4 096 at m = 2, 31 / 4 096 at m = 5; common
        // choice 2 (2 + 20 x 40 / 4 096 = 2.20 against 3 + 20 x 31 / 4 096 = 3.15).  Pulled with weight 128: share(2) = (9 + 128 x 40 / 4 096)
        // / 256 = 10.25 / 256: cost 2.80; share(3) = (0 + 128 x 31 / 4 096) / 256: cost 3.08: the block takes 2 like the rest.
        Hist h(eb_geometry(1024, 2048, false));
        for (uint32_t r = 0; r < 4; ++r) {
            for (uint32_t c = 0; c < 8; ++c) h.cold(r, c, 5, 1);
        }
        uint32_t *odd = h.at(2, 5);
        odd[0] = 119;
        odd[5] = 0;
        odd[2] = 9;
        CHECK_EQ(eb_best_lengths(odd, 128, 5, 20.0, nullptr), 3);   // by its own sample
        const EbDecision d = eb_decide(h.g, 5, 20.0, h.v.data());
        CHECK(!d.mixed && d.block_ke.empty());
        CHECK_EQ(d.lengths, 2);
        CHECK(d.alive_share == 0.009765625);   // pooled: 40 / 4 096
        // ... but a block that really differs keeps its own mind: 64 of 128 alive at exactly 2 lengths: pulled share(2) = (64 + 1.25) / 256:
        // cost(2) = 7.1 > 4.5; share(3) = 0.97 / 256: cost(3) = 3.08: ke 3 where the others take 2
        odd[0] = 64;
        odd[2] = 64;
        const EbDecision e = eb_decide(h.g, 5, 20.0, h.v.data());
        CHECK(e.mixed && e.block_ke.size() == 32);
        for (size_t b = 0; b < e.block_ke.size(); ++b) CHECK_EQ(e.block_ke[b], b == 2 * 8 + 5 ? 3 : 2);
    }
}

static void properties(size_t n_cases)
{
    std::mt19937_64 rng(0xEB91A4);
    const uint64_t sizes[] = {256, 300, 512, 700, 1024, 3000, 16384, 16385, 70000};
    for (size_t it = 0; it < n_cases; ++it) {
        const bool self = (rng() & 1) != 0;
        const uint64_t n_rows = sizes[rng() % 9], n_cols = self ? n_rows : sizes[rng() % 9];
        const size_t nk = 3 + rng() % 6;
        const EbGeometry g = eb_geometry(n_rows, n_cols, self);
        CHECK(g.shift_r >= 8 && g.shift_c >= 8 && g.blk_rows >= 1 && g.blk_rows <= EB_BLOCKS_MAX && g.blk_cols >= 1 && g.blk_cols <= EB_BLOCKS_MAX);
        CHECK(((uint64_t)g.blk_rows << g.shift_r) >= n_rows && ((uint64_t)(g.blk_rows - 1) << g.shift_r) < n_rows);
        CHECK(((uint64_t)g.blk_cols << g.shift_c) >= n_cols && ((uint64_t)(g.blk_cols - 1) << g.shift_c) < n_cols);
        CHECK(g.samples >= EB_SAMPLES_MIN && (uint64_t)g.samples * g.live_blocks >= EB_SAMPLES_TOTAL);
        // blocks of three kinds (unrelated, related, anything), some without a sample; below the diagonal nothing is sampled
        std::vector<uint32_t> hist((size_t)g.n_blocks() * EB_HIST, 0u);
        const int style = (int)(rng() % 4);
        for (uint32_t b = 0; b < g.n_blocks(); ++b) {
            if (self && b % g.blk_cols < b / g.blk_cols) continue;
            uint32_t *h = &hist[(size_t)b * EB_HIST];
            const int kind = style == 3 ? (int)(rng() % 4) : style;
            if (kind == 0) {
                const uint32_t alive = (uint32_t)(rng() % (g.samples / 8 + 1));
                h[rng() % 2] = g.samples - alive;
                for (uint32_t i = 0; i < alive; ++i) ++h[2 + rng() % (nk - 1)];
            } else if (kind == 1) {
                h[nk] = g.samples;
            } else if (kind == 2) {
                for (uint32_t i = 0; i < g.samples; ++i) ++h[rng() % (nk + 1)];
            }   // (3: no sample)
        }
        const EbDecision d = eb_decide(g, nk, eb_cost(64, n_rows, n_cols, self), hist.data());
        CHECK(d.lengths == 0 || (d.lengths >= 2 && d.lengths <= 4 && d.lengths < (int)nk));
        CHECK(d.alive_share >= 0.0 && d.alive_share <= 1.0);
        if (!d.mixed) {
            CHECK(d.block_ke.empty());
            continue;
        }
        CHECK_EQ(d.block_ke.size(), g.n_blocks());
        if (d.block_ke.size() != g.n_blocks()) continue;
        bool differ = false;
        int first = -1;
        for (uint32_t r = 0; r < g.blk_rows; ++r) {
            for (uint32_t c = 0; c < g.blk_cols; ++c) {
                const uint8_t ke = d.block_ke[(size_t)r * g.blk_cols + c];
                CHECK(ke == nk || (ke >= 2 && ke <= 4 && ke < nk));
                if (self) CHECK_EQ(ke, d.block_ke[(size_t)c * g.blk_cols + r]);
                if (self && c < r) continue;   // live blocks only
                if (first < 0) first = ke;
                else if (ke != first) differ = true;
            }
        }
        CHECK(differ);   // mixed <=> two live blocks differ (not mixed: there is no table to differ in)
    }
}

int main(int argc, char **argv)
{
    const char *what = argc > 1 ? argv[1] : "pinned";
    const size_t n = argc > 2 ? strtoull(argv[2], nullptr, 10) : 4000;
    if (!strcmp(what, "pinned")) pinned();
    else if (!strcmp(what, "properties")) properties(n);
    else return 2;
    if (g_failed) printf("FAILED %ld of %ld\n", g_failed, g_checks);
    else printf("ok %ld\n", g_checks);
    return g_failed ? 1 : 0;
}
