// within_plan.hpp -- HOW the pairs within a distance cap are picked out of a dense band on the device (within.hip, DESIGN.md
// §4.9): the numbers of the three launches (chunk size, chunks of a band, steps of the scan, scratch bytes, the band's pair
// limit), the predicate, the (i, j) of a pair position, and within_select_host(), the plain C++ form of the three kernels
// that tests/native/within_check.cpp checks against a loop over the array.  The kernels take every one of these from here.
// No HIP header.
//
// A band is `m` consecutive positions of a dense call's pair space (skl_self_dists_rows / skl_cross_dists_rows order), its
// values `ncols` f32 per position (2: core, acc; 1: the single-k distance or ANI), the first one at position `first` of the
// whole pair space.
//   1. COUNT: a workgroup of WITHIN_THREADS threads owns a CHUNK of WITHIN_CHUNK consecutive positions, a wave a quarter of it;
//      a lane reads 16 bytes (2 or 4 positions) per trip.  One u32 per chunk: the positions that pass.
//   2. SCAN: ONE workgroup walks the chunk counts in steps of WITHIN_SCAN_STEP, the running total carried from step to step:
//      offset[c] = base + the counts of the chunks before c, as u64, where base is the total the bands before this one left in
//      device memory; the new total goes back to the same word.  Nothing waits for another workgroup anywhere.
//   3. SCATTER: the chunking of the count.  A position's slot is the chunk's offset + the totals of the waves before its own +
//      its rank among the wave's positions that pass (ballots, in position order).  Slots at or beyond `capacity` are skipped.
//      The wave's first position becomes (i, j) once -- f64 guess, integer fix-up -- and a lane that keeps a pair steps forward
//      from there by whole rows.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define SKL_WITHIN_HD __host__ __device__
#else
#define SKL_WITHIN_HD
#endif

namespace skl {

constexpr uint32_t WITHIN_THREADS = 256;            // one workgroup per chunk: 4 waves
constexpr uint32_t WITHIN_WAVES = WITHIN_THREADS / 64u;
constexpr uint32_t WITHIN_CHUNK = 2048;             // pair positions per chunk: 16 KiB of (core, acc), 8 KiB of single values
constexpr uint32_t WITHIN_WAVE_SPAN = WITHIN_CHUNK / WITHIN_WAVES;   // consecutive positions of one wave
constexpr uint32_t WITHIN_SCAN_THREADS = 256;       // the scan's one workgroup ...
constexpr uint32_t WITHIN_SCAN_STEP = 4u * WITHIN_SCAN_THREADS;      // ... takes this many chunk counts per step, 4 a thread
constexpr uint64_t WITHIN_BAND_PAIR_LIMIT = 1ull << 32;              // a band holds fewer pairs: its counts and ranks are u32
static_assert(WITHIN_WAVE_SPAN % (64u * 4u) == 0u, "a wave's span is whole trips of 64 lanes x 4 positions (and x 2)");

// positions a lane reads per 16-byte load, and the trips of a wave over its span
SKL_WITHIN_HD inline uint32_t within_lane_positions(uint32_t ncols) { return ncols == 2u ? 2u : 4u; }
SKL_WITHIN_HD inline uint32_t within_trips(uint32_t ncols) { return WITHIN_WAVE_SPAN / (64u * within_lane_positions(ncols)); }

inline bool within_band_ok(uint64_t m) { return m < WITHIN_BAND_PAIR_LIMIT; }
inline uint64_t within_chunks(uint64_t m) { return (m + WITHIN_CHUNK - 1u) / WITHIN_CHUNK; }
inline uint64_t within_scan_steps(uint64_t chunks) { return (chunks + WITHIN_SCAN_STEP - 1u) / WITHIN_SCAN_STEP; }
// the dense band's buffer: whole 16-byte loads up to the last position, so the last load of an odd band stays inside
inline size_t within_band_bytes(uint64_t m, uint32_t ncols) { return (size_t)((m * ncols * sizeof(float) + 15u) / 16u * 16u); }
// scratch beside it: the running total (u64, in a 16-byte slot), the chunk offsets (u64), the chunk counts (u32)
constexpr size_t WITHIN_SCRATCH_TOTAL_BYTES = 16;
inline size_t within_scratch_offsets_at() { return WITHIN_SCRATCH_TOTAL_BYTES; }
inline size_t within_scratch_counts_at(uint64_t chunks) { return WITHIN_SCRATCH_TOTAL_BYTES + (size_t)chunks * sizeof(uint64_t); }
inline size_t within_scratch_bytes(uint64_t chunks) { return within_scratch_counts_at(chunks) + (size_t)chunks * sizeof(uint32_t); }

// THE PREDICATE, on the f32 values the dense call stores.  first column: v0 <= first (a distance) or, for ANI, v0 >= first with
// first = (float)(1 - cap); second column (core/accessory only, unless switched off): v1 <= second.  Every comparison is false
// for a NaN, so a NaN in a tested column never passes.
struct WithinPred {
    float first = 0.0f, second = 0.0f;
    uint32_t ani = 0;           // the first column is an identity: the test turns round
    uint32_t test_second = 0;   // core/accessory with a finite (or -inf) second cap
};
// false: a cap is NaN or max_first is negative (the caller's SKL_ERR_INVALID_ARG)
inline bool within_pred_make(double max_first, double max_second, bool ani, uint32_t ncols, WithinPred *q)
{
    if (max_first != max_first || max_second != max_second || max_first < 0.0) return false;
    q->ani = ani ? 1u : 0u;
    q->first = ani ? (float)(1.0 - max_first) : (float)max_first;   // (the bound is formed in double and rounded once)
    q->test_second = ncols == 2u && max_second != (double)INFINITY ? 1u : 0u;
    q->second = (float)max_second;
    return true;
}
SKL_WITHIN_HD inline bool within_keep(const WithinPred &q, float v0, float v1)
{
    const bool a = q.ani ? v0 >= q.first : v0 <= q.first;
    return a && (!q.test_second || v1 <= q.second);
}

// first condensed index of row i of n samples (distance_matrix.rs:11-14 at j = i + 1)
SKL_WITHIN_HD inline uint64_t within_row_start(uint64_t i, uint64_t n) { return n * i - ((i * (i + 1u)) >> 1); }

// The row and the position in it of `flat`.  Self: flat is a condensed index of n >= 2 samples, row i holds n - 1 - i pairs
// (epilogue.hip's locator restated for host and device: the f64 guess of distance_matrix.rs:46-51 put right by a search).
// Cross: rows of n pairs each, the quotient from the f64 product (flat < 2^53 is exact in a double) put right by one step.
SKL_WITHIN_HD inline void within_locate(bool self_mode, uint64_t flat, uint64_t n, uint32_t *row, uint32_t *pos)
{
    if (self_mode) {
        const double nn = (double)n;
        const double guess = nn - 2.0 - ::floor(::sqrt(-8.0 * (double)flat + 4.0 * nn * (nn - 1.0) - 7.0) / 2.0 - 0.5);
        uint64_t i = guess > 0.0 ? (uint64_t)guess : 0u;   // (false for a NaN too)
        if (i > n - 2u) i = n - 2u;
        while (i > 0u && within_row_start(i, n) > flat) --i;
        while (i + 2u < n && within_row_start(i + 1u, n) <= flat) ++i;
        *row = (uint32_t)i;
        *pos = (uint32_t)(flat - within_row_start(i, n));
    } else {
        uint64_t q = (uint64_t)((double)flat * (1.0 / (double)n));
        int64_t r = (int64_t)(flat - q * n);
        while (r < 0) {
            --q;
            r += (int64_t)n;
        }
        while (r >= (int64_t)n) {
            ++q;
            r -= (int64_t)n;
        }
        *row = (uint32_t)q;
        *pos = (uint32_t)r;
    }
}
// ... and `ahead` positions further on: forward by whole rows (self: each one shorter than the last)
SKL_WITHIN_HD inline void within_step(bool self_mode, uint64_t n, uint32_t row, uint32_t pos, uint32_t ahead, uint32_t *i, uint32_t *j)
{
    uint64_t p = (uint64_t)pos + ahead;
    if (self_mode) {
        uint64_t len = n - 1u - row;
        while (p >= len) {
            p -= len;
            ++row;
            --len;
        }
        *i = row;
        *j = row + 1u + (uint32_t)p;
    } else {
        uint32_t r, c;
        within_locate(false, p, n, &r, &c);   // (a row may be one pair long: no loop over rows)
        *i = row + r;
        *j = c;
    }
}

// The three kernels on the host, step for step.  dense: m x ncols values; first: position of dense[0] in the whole pair space
// of `n` columns.  Records [0, min(found, capacity)) go to out_i / out_j / out_d (sized by the caller); returns the number of
// positions that pass.  counts_out / offsets_out (nullable): what the count and the scan leave, offsets without a base.
inline uint64_t within_select_host(const float *dense, uint64_t m, uint32_t ncols, bool self_mode, uint64_t n, uint64_t first,
                                   const WithinPred &q, uint64_t capacity, uint32_t *out_i, uint32_t *out_j, float *out_d,
                                   std::vector<uint32_t> *counts_out = nullptr, std::vector<uint64_t> *offsets_out = nullptr)
{
    const uint64_t chunks = within_chunks(m);
    auto keep = [&](uint64_t p) { return within_keep(q, dense[p * ncols], ncols == 2u ? dense[p * ncols + 1u] : 0.0f); };
    // 1. count
    std::vector<uint32_t> counts(chunks, 0u);
    for (uint64_t c = 0; c < chunks; ++c) {
        for (uint64_t p = c * WITHIN_CHUNK; p < m && p < (c + 1u) * WITHIN_CHUNK; ++p) counts[c] += keep(p) ? 1u : 0u;
    }
    // 2. scan, a step at a time with the total carried
    std::vector<uint64_t> offsets(chunks, 0u);
    uint64_t carry = 0;
    for (uint64_t s = 0; s < within_scan_steps(chunks); ++s) {
        uint64_t in_step = 0;
        for (uint64_t c = s * WITHIN_SCAN_STEP; c < chunks && c < (s + 1u) * WITHIN_SCAN_STEP; ++c) {
            offsets[c] = carry + in_step;
            in_step += counts[c];
        }
        carry += in_step;
    }
    // 3. scatter: wave by wave, each from the (row, position) of its first pair
    for (uint64_t c = 0; c < chunks; ++c) {
        uint64_t slot = offsets[c];
        for (uint32_t w = 0; w < WITHIN_WAVES; ++w) {
            const uint64_t w0 = c * WITHIN_CHUNK + (uint64_t)w * WITHIN_WAVE_SPAN;
            if (w0 >= m) break;
            uint32_t row, pos;
            within_locate(self_mode, first + w0, n, &row, &pos);
            for (uint32_t a = 0; a < WITHIN_WAVE_SPAN && w0 + a < m; ++a) {
                if (!keep(w0 + a)) continue;
                if (slot < capacity) {
                    within_step(self_mode, n, row, pos, a, &out_i[slot], &out_j[slot]);
                    for (uint32_t x = 0; x < ncols; ++x) out_d[slot * ncols + x] = dense[(w0 + a) * ncols + x];
                }
                ++slot;
            }
        }
    }
    if (counts_out) *counts_out = counts;
    if (offsets_out) *offsets_out = offsets;
    return carry;
}

}  // namespace skl
