// hist.hip -- the histogram of a dense band (gfx950, wave64) behind the dense kernels: skl_self_dists_hist / skl_cross_dists_hist
// (capi_hist.cpp).  The band is the f32 buffer a dense call leaves in device memory; it is read ONCE, in 16-byte loads, and
// every position is binned by hist_plan.hpp's cell rule.  The grid, the numbers of a launch and the sequential restatement
// (hist_host) are hist_plan.hpp's.
//   hist_lds_kernel<NCOLS>      cells <= HIST_LDS_CELLS: a workgroup zeroes a private u32 histogram in LDS, strides over the band's
//                               chunks adding with LDS atomics, and flushes its non-zero cells with 64-bit global atomic adds
//   hist_global_kernel<NCOLS>   larger grids: the same loads, added straight into the u64 counts
//
// 1. BOUNDS.  A thread's load is float4 number q = p / V of the band, taken only when its first position p < m, else number 0
//    (position 0 exists: a launch has m >= 1); the buffer holds within_band_bytes(m, NCOLS), whole 16-byte loads up to the last
//    position.  An element of a load beyond m is never binned.  A cell index comes from hist_cell(): below n0 * n1 = the length
//    of counts and, in the LDS kernel, at most HIST_LDS_CELLS = the length of the private histogram (launch_hist picks the
//    kernel by hist_in_lds).  The two codes (HIST_NAN, HIST_OUTSIDE) never index anything.
// 2. THE PEEL.  Real collections have spikes -- early-break pairs stored as exactly (1, 1), identical samples at 0 -- where all
//    64 lanes of a wave hit one counter and a per-lane atomic would serialise 64 deep.  hist_add() takes the cell of the first
//    pending lane, ballots the lanes that hold the same cell, lets that one lane add the popcount, and repeats HIST_PEEL_ROUNDS
//    times; whoever is still pending adds 1.  Every lane of the wave runs every ballot: the loop's condition is the pending
//    mask, which is wave-uniform, and lanes without a cell to add simply are not in it.  One popcount per wave and trip is still
//    one atomic per 64 positions on ONE address when 97 % of a collection is stored as (1, 1), and atomics on one address
//    are served one after the other (measured: the 256 x 256 call took 2.2 x the count-only within call that way).  So a wave
//    also HOLDS up to HIST_HELD_CELLS cells back (HistHeld), the first distinct ones it meets: the positions at a held cell are a
//    ballot and an addition in registers, and each sum is added by one atomic when the walk ends.  (Holding ONE cell still left
//    the 256 x 256 call at 1.6 x: the second and third spike, 1-3 % of the pairs each, were then what met on one address.)
//    On spread-out data the held cells are as rare as any other and the peel does what it did.
// 3. OUTSIDE and NAN are ballots and popcounts in (wave-uniform) registers; lane 0 of each wave adds the two sums once at the end.
// 4. A u32 LDS counter cannot overflow: a band holds fewer than 2^32 positions (within_band_ok).  Counts are integers and adds
//    commute, so the result does not depend on scheduling.  Nothing waits for another workgroup; the only barriers are the two
//    around the LDS histogram's life.  No scalar memory writes anywhere: plain C++ and vector atomics only.
#include "kernels.h"

namespace skl {

namespace {

// What a wave HOLDS BACK: the counts of up to HIST_HELD_CELLS cells, in (wave-uniform) registers, added by one atomic each
// when the walk ends.  The cells are the first distinct ones the wave meets -- on a collection with spikes, the spikes --
// and positions at them then cost a ballot and no atomic at all.
struct HistHeld {
    uint32_t cell[HIST_HELD_CELLS];    // HIST_NAN (no position's cell): the slot is free
    uint32_t count[HIST_HELD_CELLS];   // < 2^32: a wave sees fewer positions than the band holds
};

template <typename Counter>
__device__ __forceinline__ void hist_flush(Counter *hist, const HistHeld &held, uint32_t lane)
{
#pragma unroll
    for (uint32_t k = 0; k < HIST_HELD_CELLS; ++k) {
        if (held.count[k] && lane == 0u) atomicAdd(hist + held.cell[k], (Counter)held.count[k]);   // (count != 0: the slot holds a cell)
    }
}

// adds 1 to hist[cell] for every lane with `has` (cell < HIST_NAN there); Counter: uint32_t (LDS) or unsigned long long (the global counts)
template <typename Counter>
__device__ __forceinline__ void hist_add(Counter *hist, bool has, uint32_t cell, uint32_t lane, HistHeld &held)
{
    uint64_t pending = __ballot(has);
    if (HIST_PEEL_ROUNDS > 0u) {
#pragma unroll
        for (uint32_t k = 0; k < HIST_HELD_CELLS; ++k) {
            const uint64_t here = __ballot(has && cell == held.cell[k]);   // (held cells differ from each other: a lane is in one ballot at most)
            held.count[k] += (uint32_t)__popcll(here);
            pending &= ~here;
        }
#pragma unroll
        for (uint32_t r = 0; r < HIST_PEEL_ROUNDS; ++r) {
            if (pending == 0ull) return;   // (wave-uniform)
            const uint32_t first = (uint32_t)__ffsll((unsigned long long)pending) - 1u;
            const uint32_t lead = (uint32_t)__builtin_amdgcn_readlane((int)cell, (int)first);   // (no held cell: its lanes left `pending` above)
            const uint64_t same = __ballot((pending >> lane & 1ull) && cell == lead);
            bool taken = false;   // a free slot takes the cell and this trip's count
#pragma unroll
            for (uint32_t k = 0; k < HIST_HELD_CELLS; ++k) {
                if (!taken && held.cell[k] == HIST_NAN) {
                    held.cell[k] = lead;
                    held.count[k] = (uint32_t)__popcll(same);
                    taken = true;
                }
            }
            if (!taken && lane == first) atomicAdd(hist + lead, (Counter)__popcll(same));
            pending &= ~same;
        }
    }
    if (pending >> lane & 1ull) atomicAdd(hist + cell, (Counter)1);
}

// A workgroup's walk over its chunks of the band: every position binned into `hist`; the two outside sums of this wave come back
template <uint32_t NCOLS, typename Counter>
__device__ __forceinline__ void hist_walk(const HistArgs &a, Counter *hist, uint32_t *off_grid, uint32_t *nans)
{
    constexpr uint32_t V = NCOLS == 2u ? 2u : 4u;                      // positions per load: V * NCOLS = 4 floats
    constexpr uint32_t TRIPS = HIST_CHUNK / (HIST_THREADS * V);
    const float4 *__restrict__ src = reinterpret_cast<const float4 *>(a.band);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t n_off = 0, n_nan = 0;
    HistHeld held;
#pragma unroll
    for (uint32_t k = 0; k < HIST_HELD_CELLS; ++k) {
        held.cell[k] = HIST_NAN;
        held.count[k] = 0u;
    }
    for (uint64_t c = blockIdx.x; c < a.chunks; c += gridDim.x) {      // (workgroup-uniform)
        float4 v[TRIPS];
        uint64_t p[TRIPS];
#pragma unroll
        for (uint32_t t = 0; t < TRIPS; ++t) {
            p[t] = c * HIST_CHUNK + (uint64_t)(t * HIST_THREADS + threadIdx.x) * V;
            v[t] = src[p[t] < a.m ? p[t] / V : 0u];                    // (unconditional: it stays one 16-byte load)
        }
#pragma unroll
        for (uint32_t t = 0; t < TRIPS; ++t) {
            const float f[4] = {v[t].x, v[t].y, v[t].z, v[t].w};
#pragma unroll
            for (uint32_t e = 0; e < V; ++e) {
                const bool exists = p[t] + e < a.m;
                const uint32_t cell = hist_cell(a.grid, f[e * NCOLS], NCOLS == 2u ? f[e * NCOLS + 1u] : 0.0f);
                n_off += (uint32_t)__popcll(__ballot(exists && cell == HIST_OUTSIDE));
                n_nan += (uint32_t)__popcll(__ballot(exists && cell == HIST_NAN));
                hist_add(hist, exists && cell < HIST_NAN, cell, lane, held);
            }
        }
    }
    hist_flush(hist, held, lane);
    *off_grid = n_off;
    *nans = n_nan;
}

__device__ __forceinline__ void hist_outside_add(const HistArgs &a, uint32_t off_grid, uint32_t nans)
{
    if ((threadIdx.x & 63u) != 0u) return;
    if (off_grid) atomicAdd(a.outside, (unsigned long long)off_grid);
    if (nans) atomicAdd(a.outside + 1, (unsigned long long)nans);
}

}  // namespace

template <uint32_t NCOLS>
__global__ __launch_bounds__(HIST_THREADS) void hist_lds_kernel(const HistArgs a)
{
    __shared__ uint32_t lds[HIST_LDS_CELLS];
    const uint32_t cells = a.grid.n0 * a.grid.n1;   // <= HIST_LDS_CELLS (launch_hist)
    for (uint32_t x = threadIdx.x; x < cells; x += HIST_THREADS) lds[x] = 0u;
    __syncthreads();
    uint32_t off_grid, nans;
    hist_walk<NCOLS>(a, lds, &off_grid, &nans);
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < cells; x += HIST_THREADS) {
        const uint32_t k = lds[x];
        if (k) atomicAdd(a.counts + x, (unsigned long long)k);
    }
    hist_outside_add(a, off_grid, nans);
}

template <uint32_t NCOLS>
__global__ __launch_bounds__(HIST_THREADS) void hist_global_kernel(const HistArgs a)
{
    uint32_t off_grid, nans;
    hist_walk<NCOLS>(a, a.counts, &off_grid, &nans);
    hist_outside_add(a, off_grid, nans);
}

hipError_t launch_hist(const HistArgs &a, hipStream_t stream)
{
    if (a.chunks == 0) return hipSuccess;
    const bool in_lds = hist_in_lds(hist_cells(a.grid));
    const dim3 grid(hist_groups(a.chunks, in_lds)), block(HIST_THREADS);
    if (in_lds) {
        if (a.grid.ncols == 2u) hipLaunchKernelGGL(hist_lds_kernel<2>, grid, block, 0, stream, a);
        else hipLaunchKernelGGL(hist_lds_kernel<1>, grid, block, 0, stream, a);
    } else {
        if (a.grid.ncols == 2u) hipLaunchKernelGGL(hist_global_kernel<2>, grid, block, 0, stream, a);
        else hipLaunchKernelGGL(hist_global_kernel<1>, grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace skl
