// eb_plan.hpp -- the EARLY BREAK's decision for one (row slab, column slab) pair, as data computed by pure functions.
//
// capi_eb.cpp early_break_plan() asks eb_applicable(), cuts the pair space with eb_geometry(), runs the sampler on the device,
// hands its histograms to eb_decide() and keeps the answer (EbPlan, capi_internal.hpp).  Nothing here touches a device: no
// device header, plain C++17 (tests/native/eb_plan_check.cpp builds it with the host compiler alone).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "dense_plan.hpp"   // BLOCKED_MIN_PAIRS, PLAN_MAX_U16_CHUNKS

namespace skl {

// EARLY BREAK.  core_acc_dist leaves its loop over the k-mer lengths at the first one whose ln J lies below the tolerance
// (jaccard.rs:89-91: J = 0, i.e. no more shared bins than chance -- expected_samebits, :26-31) and a fit over fewer than three
// lengths is (1, 1) (:117): a pair that fails the test at one of its first lengths is decided by them alone, and between
// unrelated genomes that is nearly every pair (a chance match at each of three lengths: 1.1 % of pairs at 4 096 bins,
// 0.2-0.4 % at 2 048).  The counts + epilogue form can then count only the first ke lengths and let the epilogue complete the
// pairs still in the running (epilogue.hip).  Whether that pays depends on the data -- completing a pair costs EB_COST x what
// the tile kernel spends on a pair and length (a whole column slice read for ONE pair), and between close relatives every
// pair stays in the running -- so the first dense call of a slab against a column slab SAMPLES the pair space: it is cut
// into blocks of (row >> shift, column >> shift) sample ids (up to 64 x 64 of them, each a multiple of 256 samples), a few
// dozen pairs of every block run the reference's loop, and every block takes the ke of {2, 3, 4} that minimises
//     ke + EB_COST x share_alive(ke)      if that is at most 0.9 x nk,
// else every length.  A database that is half one species therefore takes the early break between the species and skips
// it within (round 5 decided once per slab pair).  Blocks of one mind give a plain launch; otherwise the pair kernel's
// (tile, k index) workgroups look their block up and leave when k index >= its ke.
// EB_COST, measured (profiles/r06_early_break_forced_lengths.md: whole calls with 2 / 3 lengths forced, T(3) - T(2) = one length's
// kernel time - EB_COST x the difference of the alive shares): 15-22.  Beyond 65 535 bins a completion is a run of thousands of
// dependent trips of one wave and comes to ~60: there the early break is taken only where hardly a pair stays in the running.
// Pair spaces large enough for the blocked epilogue order (dense_plan.hpp) complete a pair for ~12-15: cfg 3 with 2 / 3 lengths 642 / 733
// ms, n = 16 000 17.2 / 19.3.
constexpr double EB_COST = 20.0, EB_COST_BLOCKED = 12.0, EB_COST_BIG = 60.0;
inline double eb_cost(uint32_t ss64, uint64_t n_rows, uint64_t n_cols, bool self_mode)
{
    if (ss64 > PLAN_MAX_U16_CHUNKS) return EB_COST_BIG;
    const uint64_t pairs = self_mode ? n_rows * (n_rows - 1) / 2 : n_rows * n_cols;
    return pairs >= BLOCKED_MIN_PAIRS ? EB_COST_BLOCKED : EB_COST;
}

constexpr uint32_t EB_BLOCKS_MAX = 64;      // blocks per side
constexpr uint32_t EB_SAMPLES_MIN = 128;    // sampled pairs per block
constexpr uint32_t EB_SAMPLES_TOTAL = 4096; // ... and at least this many in all
constexpr size_t EB_NK_MIN = 3, EB_NK_MAX = 8;   // k-mer lengths: a fit needs three; the sampler's histogram has 9 bins (0..8 lengths passed)
constexpr uint64_t EB_MIN_PAIR_SPACE = 65536;    // n_rows x n_cols below which no decision is worth a sample
constexpr size_t EB_PLANS_KEPT = 8;              // decisions a context keeps (the oldest goes)
constexpr int EB_HIST = 9;                       // histogram entries per block: pairs that pass the test at exactly their first m lengths, m = 0..8

// knob: SKL_EARLY_BREAK (0 off, 1 sampled, 2..7 forced)
inline bool eb_applicable(int knob, size_t nk, uint64_t n_rows, uint64_t n_cols)
{
    if (knob == 0 || nk < EB_NK_MIN || nk > EB_NK_MAX) return false;
    return n_rows * n_cols >= EB_MIN_PAIR_SPACE;
}

// The pair space cut into blocks of (row >> shift_r, column >> shift_c) sample ids, and what the sampler is asked for.
struct EbGeometry {
    bool self_mode = false;
    uint32_t shift_r = 31, shift_c = 31, blk_rows = 1, blk_cols = 1;   // (as a forced decision reports them: one block)
    uint32_t live_blocks = 1;   // blocks that hold a pair (self mode: on or above the diagonal)
    uint32_t samples = 0;       // sampled pairs per block
    uint32_t n_blocks() const { return blk_rows * blk_cols; }
};
inline EbGeometry eb_geometry(uint64_t n_rows, uint64_t n_cols, bool self_mode)
{
    EbGeometry g;
    g.self_mode = self_mode;
    // blocks: a power of two of samples per side, at least 256, at most EB_BLOCKS_MAX per side
    auto shift_for = [](uint64_t n) {
        uint32_t sh = 8;
        while (((n + ((uint64_t)1 << sh) - 1) >> sh) > EB_BLOCKS_MAX) ++sh;
        return sh;
    };
    g.shift_r = shift_for(n_rows);
    g.shift_c = self_mode ? g.shift_r : shift_for(n_cols);
    g.blk_rows = (uint32_t)((n_rows + ((uint64_t)1 << g.shift_r) - 1) >> g.shift_r);
    g.blk_cols = (uint32_t)((n_cols + ((uint64_t)1 << g.shift_c) - 1) >> g.shift_c);
    g.live_blocks = self_mode ? g.blk_rows * (g.blk_rows + 1) / 2 : g.n_blocks();
    g.samples = std::max(EB_SAMPLES_MIN, (EB_SAMPLES_TOTAL + g.live_blocks - 1) / g.live_blocks);
    return g;
}

// ke of {2, 3, 4} with the lowest modelled cost for a histogram of `total` sampled pairs (hist[m]: pairs that pass the test at
// exactly their first m lengths), or 0 when counting every length is cheaper.  `prior` (9 shares, or null) and its weight:
// the block's estimate is pulled towards the pooled sample of the blocks that take the early break -- 128 pairs a block cannot
// tell a 5 % share from a 9 % one, ten thousand can -- so that only a block that really differs decides differently.
inline int eb_best_lengths(const uint32_t *hist, uint32_t total, size_t nk, double eb_cost, double *share_out, const double *prior = nullptr,
                           double weight = 0.0, int preferred = 0)
{
    int best_ke = 0;
    double best = 0.9 * (double)nk, cost_of[5] = {0, 0, 0, 0, 0};
    if (total == 0) return 0;
    // (two lengths decide nothing by themselves -- a fit needs three -- but a pair that fails the test at one of them is
    // decided all the same: (1, 1); ke = 2 leaves more pairs to complete and pays where few share a bin at all: 2 048 bins)
    for (int ke = 2; ke <= 4 && ke < (int)nk; ++ke) {
        double still = 0.0, prior_still = 0.0;
        for (int m = ke; m <= 8; ++m) {
            still += hist[m];
            if (prior) prior_still += prior[m];
        }
        const double share = (still + weight * prior_still) / ((double)total + weight), cost = (double)ke + eb_cost * share;
        cost_of[ke] = cost;
        if (cost <= best) {
            best = cost;
            best_ke = ke;
            if (share_out) *share_out = share;
        }
    }
    // (the blocks' common choice stands unless this block's own is clearly better: the costs of 2 and 3 lengths are often a
    // quarter of a length apart, and a plan whose blocks disagree pays for its table)
    if (preferred >= 2 && preferred <= 4 && preferred < (int)nk && best_ke != preferred && cost_of[preferred] <= 0.9 * (double)nk &&
        cost_of[preferred] <= best + 0.5) {
        best_ke = preferred;
    }
    return best_ke;
}

// How many k-mer lengths the pair kernel counts before the epilogue completes the pairs still in the running.
struct EbDecision {
    int lengths = 0;                    // pooled decision: lengths to count (0: all of them, no early break)
    double alive_share = 0.0;           // sampled share of the pairs still in the running after them
    bool mixed = false;                 // the blocks disagree: block_ke holds each block's count (nk: all of them)
    std::vector<uint8_t> block_ke;      // [blk_rows * blk_cols] when mixed, else empty
};

// SKL_EARLY_BREAK = 2..7: that many lengths whatever the data (A/B build, tests)
inline EbDecision eb_forced(int knob, size_t nk)
{
    EbDecision d;
    d.lengths = knob < (int)nk ? knob : 0;
    return d;
}

// hist: [g.n_blocks()][EB_HIST] as the sampler left it
inline EbDecision eb_decide(const EbGeometry &g, size_t nk, double eb_cost, const uint32_t *hist)
{
    EbDecision d;
    const uint32_t n_blocks = g.n_blocks();
    // the pooled decision (the kNN drivers' and the one-block case's)
    uint32_t pooled[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, pooled_n = 0;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        for (int m = 0; m <= 8; ++m) {
            pooled[m] += hist[(size_t)b * 9 + m];
            pooled_n += hist[(size_t)b * 9 + m];
        }
    }
    d.lengths = eb_best_lengths(pooled, pooled_n, nk, eb_cost, &d.alive_share);
    if (g.live_blocks > 1) {
        // per block.  Pass 1: every block's own sample decides whether it takes the early break at all; pass 2: the blocks that
        // do are pooled, and every block decides again with its estimate pulled towards that pool (weight: one block's sample).
        const uint8_t all = (uint8_t)nk;
        std::vector<uint8_t> ke(n_blocks, all);
        std::vector<uint32_t> tot(n_blocks, 0u);
        double cold[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cold_n = 0.0;
        for (uint32_t b = 0; b < n_blocks; ++b) {
            for (int m = 0; m <= 8; ++m) tot[b] += hist[(size_t)b * 9 + m];
            if (eb_best_lengths(&hist[(size_t)b * 9], tot[b], nk, eb_cost, nullptr) > 0) {
                for (int m = 0; m <= 8; ++m) cold[m] += hist[(size_t)b * 9 + m];
                cold_n += tot[b];
            }
        }
        int common = 0;
        if (cold_n > 0.0) {
            uint32_t cold_u[9];
            for (int m = 0; m <= 8; ++m) cold_u[m] = (uint32_t)std::min(cold[m], 4.0e9);
            common = eb_best_lengths(cold_u, (uint32_t)std::min(cold_n, 4.0e9), nk, eb_cost, nullptr);
            for (int m = 0; m <= 8; ++m) cold[m] /= cold_n;
        }
        bool differ = false;
        uint8_t first = 0;
        for (uint32_t b = 0; b < n_blocks; ++b) {
            if (g.self_mode && b % g.blk_cols < b / g.blk_cols) continue;   // below the diagonal: no pair
            const int own = eb_best_lengths(&hist[(size_t)b * 9], tot[b], nk, eb_cost, nullptr, cold_n > 0.0 ? cold : nullptr, cold_n > 0.0 ? (double)g.samples : 0.0, common);
            ke[b] = own > 0 ? (uint8_t)own : all;
            if (first == 0) first = ke[b];
            else if (ke[b] != first) differ = true;
        }
        if (differ) {
            if (g.self_mode) {   // (mirror: a tile on the diagonal may look a block up from either side)
                for (uint32_t r = 0; r < g.blk_rows; ++r) {
                    for (uint32_t c = 0; c < r && c < g.blk_cols; ++c) ke[(size_t)r * g.blk_cols + c] = ke[(size_t)c * g.blk_cols + r];
                }
            }
            d.mixed = true;
            d.block_ke = ke;
        } else {
            d.lengths = first == all ? 0 : (int)first;   // one mind: a plain launch
        }
    }
    return d;
}

}  // namespace skl
