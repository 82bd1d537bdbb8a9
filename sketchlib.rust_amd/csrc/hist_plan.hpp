// hist_plan.hpp -- a histogram of the values a dense call stores (hist.hip, capi_hist.cpp): the grid and its
// validation, THE CELL RULE, the numbers of a launch (threads, chunk, workgroups, the size from which the counters leave LDS,
// scratch bytes), and hist_host(), the sequential restatement of the two kernels that tests/native/hist_check.cpp checks
// against a plain loop over the array.  The kernels take every one of these from here.  No HIP header.
//
// A band is `m` consecutive positions of a dense call's pair space, `ncols` f32 per position (within_plan.hpp).  A launch
// reads it ONCE: hist_groups() workgroups of HIST_THREADS threads stride over its chunks of HIST_CHUNK positions, a thread
// reading 16 bytes (2 or 4 positions) per trip, HIST_THREADS loads side by side.  Which pair a position is does not matter
// to a histogram, so nothing is located.
//   cells <= HIST_LDS_CELLS   hist_lds_kernel: each workgroup adds into a private u32 histogram in LDS and flushes its
//                             non-zero cells with 64-bit atomic adds at the end.  A band holds fewer than 2^32 pairs
//                             (within_band_ok), so a u32 counter cannot overflow within a launch.
//   larger grids              hist_global_kernel: the same loads, added straight into the u64 counts.
// Either way a wave first PEELS: the lanes whose cell equals the first pending lane's are found by a ballot and added as
// one popcount by one lane, HIST_PEEL_ROUNDS times, before the lanes still pending add 1 each; and the wave holds the counts of
// the first HIST_HELD_CELLS distinct cells it meets back in registers -- the spikes -- adding them when its walk ends, so a
// collection that is 97 % (1, 1) does not send every wave's every trip to one address.  Off-grid and NaN positions are
// ballots and popcounts kept in registers, added once per wave at the end.  Integer adds commute: the result is exact whatever
// the scheduling.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "within_plan.hpp"   // the band: within_band_bytes, within_band_ok, SKL_WITHIN_HD

// (timing only: profiles/dists_hist.md measures a library built with 0 rounds against the shipped one)
#ifndef SKL_HIST_PEEL_ROUNDS
#define SKL_HIST_PEEL_ROUNDS 3
#endif

namespace skl {

constexpr uint32_t HIST_THREADS = 256;              // 4 waves
constexpr uint32_t HIST_CHUNK = 2048;               // pair positions per chunk: 16 KiB of (core, acc), 8 KiB of single values
constexpr uint32_t HIST_LDS_CELLS = 16384;          // u32 counters of a workgroup's private histogram: 64 KiB, two workgroups in a CU's 160 KiB
constexpr uint32_t HIST_MAX_CELLS = 1u << 20;       // 8 MiB of u64 counts
constexpr uint32_t HIST_LDS_GROUPS = 512;           // workgroups of an LDS launch at most: two per CU of 256, each flushing once
constexpr uint32_t HIST_GLOBAL_GROUPS = 2048;       // ... and of a global one: eight per CU
constexpr uint32_t HIST_PEEL_ROUNDS = SKL_HIST_PEEL_ROUNDS;   // the spikes a real collection has -- (1, 1), 0 -- and one more
constexpr uint32_t HIST_HELD_CELLS = 4;             // cells whose counts a wave holds back in registers to the end of its walk (the first distinct ones it meets)
constexpr uint32_t HIST_OUTSIDE = 0xFFFFFFFFu;      // hist_cell: a value off the grid in some column, none of them NaN
constexpr uint32_t HIST_NAN = 0xFFFFFFFEu;          // hist_cell: a NaN in some column
static_assert(HIST_CHUNK % (HIST_THREADS * 4u) == 0u, "a chunk is whole trips of HIST_THREADS loads of 4 positions (and of 2)");
static_assert(HIST_MAX_CELLS < HIST_NAN, "a cell index never collides with the two codes");

inline uint64_t hist_chunks(uint64_t m) { return (m + HIST_CHUNK - 1u) / HIST_CHUNK; }
SKL_WITHIN_HD inline uint32_t hist_lane_positions(uint32_t ncols) { return ncols == 2u ? 2u : 4u; }
SKL_WITHIN_HD inline uint32_t hist_trips(uint32_t ncols) { return HIST_CHUNK / (HIST_THREADS * hist_lane_positions(ncols)); }
inline bool hist_in_lds(uint64_t cells) { return cells <= HIST_LDS_CELLS; }
inline uint32_t hist_groups(uint64_t chunks, bool in_lds)
{
    const uint64_t most = in_lds ? HIST_LDS_GROUPS : HIST_GLOBAL_GROUPS;
    return (uint32_t)(chunks < most ? chunks : most);
}
// scratch: the two outside words (u64, in a 16-byte slot), then the counts of a caller whose own are on the host
constexpr size_t HIST_SCRATCH_HEAD_BYTES = 16;
inline size_t hist_scratch_bytes(uint64_t cells_on_host) { return HIST_SCRATCH_HEAD_BYTES + (size_t)cells_on_host * sizeof(uint64_t); }

// THE GRID as the kernels see it: bounds rounded to float once, scale = (float)(n / (hi - lo)) with the quotient formed in double
struct HistGrid {
    float lo0 = 0.0f, hi0 = 1.0f, scale0 = 1.0f;
    float lo1 = 0.0f, hi1 = 1.0f, scale1 = 1.0f;
    uint32_t n0 = 1, n1 = 1;
    uint32_t ncols = 1;
};
inline uint64_t hist_cells(const HistGrid &g) { return (uint64_t)g.n0 * g.n1; }

// one column's part of the validation.  false: n == 0, a bound that is NaN or infinite (as given or once rounded to float),
// hi <= lo after rounding, or a range so narrow that the scale is not a finite float
inline bool hist_axis_make(double lo, double hi, uint32_t n, float *flo, float *fhi, float *scale)
{
    if (n == 0u || !std::isfinite(lo) || !std::isfinite(hi)) return false;
    const float l = (float)lo, h = (float)hi;
    if (!std::isfinite(l) || !std::isfinite(h) || !(h > l)) return false;
    const float s = (float)((double)n / ((double)h - (double)l));
    if (!std::isfinite(s) || !(s > 0.0f)) return false;
    *flo = l;
    *fhi = h;
    *scale = s;
    return true;
}
// false: the caller's SKL_ERR_INVALID_ARG.  ncols == 1: lo1, hi1 and n1 are not looked at, and n1 counts as 1
inline bool hist_grid_make(double lo0, double hi0, uint32_t n0, double lo1, double hi1, uint32_t n1, uint32_t ncols, HistGrid *g)
{
    HistGrid out;
    out.ncols = ncols == 2u ? 2u : 1u;
    if (!hist_axis_make(lo0, hi0, n0, &out.lo0, &out.hi0, &out.scale0)) return false;
    out.n0 = n0;
    if (out.ncols == 2u) {
        if (!hist_axis_make(lo1, hi1, n1, &out.lo1, &out.hi1, &out.scale1)) return false;
        out.n1 = n1;
    }
    if (hist_cells(out) > HIST_MAX_CELLS) return false;
    *g = out;
    return true;
}

// THE CELL RULE of one column, in f32 exactly as written: one subtract, one multiply, truncation, the last cell closed at hi.
// (v - lo) * scale is >= 0 here; at or beyond n (v == hi, or an infinite v - lo of a grid as wide as the floats) it is the last cell.
SKL_WITHIN_HD inline bool hist_axis_inside(float v, float lo, float hi) { return !(v < lo || v > hi); }   // (true for a NaN: tested first)
SKL_WITHIN_HD inline uint32_t hist_axis_cell(float v, float lo, float scale, uint32_t n)
{
    const float x = (v - lo) * scale;
    return x < (float)n ? (uint32_t)x : n - 1u;
}
// The cell of a position: c0 * n1 + c1, HIST_NAN (a NaN in some column: it wins over off-grid) or HIST_OUTSIDE
SKL_WITHIN_HD inline uint32_t hist_cell(const HistGrid &g, float v0, float v1)
{
    const bool two = g.ncols == 2u;
    if (v0 != v0 || (two && v1 != v1)) return HIST_NAN;
    if (!hist_axis_inside(v0, g.lo0, g.hi0) || (two && !hist_axis_inside(v1, g.lo1, g.hi1))) return HIST_OUTSIDE;
    const uint32_t c0 = hist_axis_cell(v0, g.lo0, g.scale0, g.n0);
    return two ? c0 * g.n1 + hist_axis_cell(v1, g.lo1, g.scale1, g.n1) : c0;
}

// One launch on the host, as the kernels walk the band: workgroup by workgroup, each striding over the chunks; the LDS form
// through a private u32 histogram flushed where it is not zero, the global form straight into counts.  dense: m x ncols
// values; counts ([cells]) and outside ([2]: off-grid, NaN) are ADDED to.
inline void hist_host(const float *dense, uint64_t m, const HistGrid &g, uint64_t *counts, uint64_t *outside)
{
    const uint64_t cells = hist_cells(g), chunks = hist_chunks(m);
    const bool in_lds = hist_in_lds(cells);
    const uint32_t groups = hist_groups(chunks, in_lds);
    std::vector<uint32_t> lds(in_lds ? cells : 0u);
    for (uint32_t wg = 0; wg < groups; ++wg) {
        std::fill(lds.begin(), lds.end(), 0u);
        for (uint64_t c = wg; c < chunks; c += groups) {
            for (uint64_t p = c * HIST_CHUNK; p < m && p < (c + 1u) * HIST_CHUNK; ++p) {
                const uint32_t cell = hist_cell(g, dense[p * g.ncols], g.ncols == 2u ? dense[p * g.ncols + 1u] : 0.0f);
                if (cell == HIST_NAN) ++outside[1];
                else if (cell == HIST_OUTSIDE) ++outside[0];
                else if (in_lds) ++lds[cell];
                else ++counts[cell];
            }
        }
        for (uint64_t x = 0; x < lds.size(); ++x) {
            if (lds[x]) counts[x] += lds[x];
        }
    }
}

}  // namespace skl
