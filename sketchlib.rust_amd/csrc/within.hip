// within.hip -- the pairs of a dense band that lie within a distance cap, compacted on the GPU (gfx950, wave64) behind the dense
// kernels: skl_self_dists_within / skl_cross_dists_within (capi_within.cpp).  The band is the f32 buffer a dense call leaves in
// device memory; three launches turn it into the list of (i, j, values) that pass, in the band's own order:
//   within_count_kernel    one workgroup per chunk of WITHIN_CHUNK pair positions, 16-byte loads, a ballot and a popcount per
//                          element of the load, the wave sums added through LDS: one u32 per chunk
//   within_scan_kernel     ONE workgroup, WITHIN_SCAN_STEP counts a step with the total carried: u64 offsets, starting from the
//                          total the earlier bands left in device memory, which it then advances
//   within_scatter_kernel  the count's chunking and loads again; slot = chunk offset + earlier waves + rank in the wave's ballots
// Exact and deterministic: no atomics, no workgroup waits for another, the order of the output is the order of the positions.
// Every number and the predicate come from within_plan.hpp, whose within_select_host() restates the three for the CPU test; a
// wave's loads and ballots are within_wave.hpp's, shared with cluster.hip.
#include "kernels.h"
#include "within_wave.hpp"

namespace skl {

template <uint32_t NCOLS>
__global__ __launch_bounds__(WITHIN_THREADS) void within_count_kernel(const WithinArgs a)
{
    __shared__ uint32_t wave_sum[WITHIN_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t w0 = (uint64_t)blockIdx.x * WITHIN_CHUNK + (uint64_t)wave * WITHIN_WAVE_SPAN;
    WithinWave<NCOLS> w;
    const uint32_t total = w0 < a.m ? w.load(a.band, a.m, a.pred, w0, lane) : 0u;   // (wave-uniform)
    if (lane == 0u) wave_sum[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < WITHIN_WAVES; ++k) sum += wave_sum[k];
        a.counts[blockIdx.x] = sum;
    }
}

__global__ __launch_bounds__(WITHIN_SCAN_THREADS) void within_scan_kernel(const WithinArgs a)
{
    __shared__ uint32_t ws[WITHIN_SCAN_THREADS / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t base = *a.total;
    __syncthreads();   // (every thread has read the total before thread 0 replaces it)
    uint64_t carry = 0;
    for (uint64_t s0 = 0; s0 < a.chunks; s0 += WITHIN_SCAN_STEP) {   // (workgroup-uniform trip count)
        const uint64_t c0 = s0 + 4ull * tid;
        uint32_t v[4], mine = 0;
#pragma unroll
        for (uint32_t x = 0; x < 4u; ++x) {
            v[x] = c0 + x < a.chunks ? a.counts[c0 + x] : 0u;
            mine += v[x];
        }
        uint32_t inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t below = __shfl_up(inc, o);
            if (lane >= (uint32_t)o) inc += below;
        }
        if (lane == 63u) ws[wave] = inc;
        __syncthreads();
        uint32_t off = 0, step_total = 0;
#pragma unroll
        for (uint32_t k = 0; k < WITHIN_SCAN_THREADS / 64u; ++k) {
            const uint32_t x = ws[k];
            if (k < wave) off += x;
            step_total += x;
        }
        uint64_t o = base + carry + off + (inc - mine);
#pragma unroll
        for (uint32_t x = 0; x < 4u; ++x) {
            if (c0 + x < a.chunks) a.offsets[c0 + x] = o;
            o += v[x];
        }
        carry += step_total;
        __syncthreads();   // (ws is written again in the next step)
    }
    if (tid == 0u) *a.total = base + carry;
}

template <uint32_t NCOLS>
__global__ __launch_bounds__(WITHIN_THREADS) void within_scatter_kernel(const WithinArgs a)
{
    __shared__ uint32_t wave_sum[WITHIN_WAVES];
    using W = WithinWave<NCOLS>;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t w0 = (uint64_t)blockIdx.x * WITHIN_CHUNK + (uint64_t)wave * WITHIN_WAVE_SPAN;
    if (a.counts[blockIdx.x] == 0u) return;   // (workgroup-uniform, before any barrier)
    W w;
    const uint32_t total = w0 < a.m ? w.load(a.band, a.m, a.pred, w0, lane) : 0u;
    if (lane == 0u) wave_sum[wave] = total;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t k = 0; k < wave; ++k) before += wave_sum[k];
    uint64_t slot0 = a.offsets[blockIdx.x] + before;   // the wave's first slot
    if (total == 0u || slot0 >= a.capacity) return;    // (no barrier follows)
    uint32_t row, pos;
    within_locate(a.self_mode != 0u, a.first + w0, a.n_cols, &row, &pos);
#pragma unroll
    for (uint32_t t = 0; t < W::TRIPS; ++t) {
        const float f[4] = {w.v[t].x, w.v[t].y, w.v[t].z, w.v[t].w};
        // positions run lane by lane, a lane's elements side by side: the rank counts every element of the lanes below
        uint32_t rank = 0, trip_total = 0;
#pragma unroll
        for (uint32_t e = 0; e < W::V; ++e) {
            rank += within_lanes_below(w.pass[t][e]);
            trip_total += (uint32_t)__popcll(w.pass[t][e]);
        }
#pragma unroll
        for (uint32_t e = 0; e < W::V; ++e) {
            if (w.pass[t][e] >> lane & 1ull) {
                const uint64_t slot = slot0 + rank;
                ++rank;
                if (slot < a.capacity) {
                    uint32_t i, j;
                    within_step(a.self_mode != 0u, a.n_cols, row, pos, (t * 64u + lane) * W::V + e, &i, &j);
                    const uint64_t at = slot - a.rebase;
                    a.out_i[at] = i;
                    a.out_j[at] = j;
                    a.out_d[at * NCOLS] = f[e * NCOLS];
                    if (NCOLS == 2u) a.out_d[at * NCOLS + 1u] = f[e * NCOLS + 1u];
                }
            }
        }
        slot0 += trip_total;
    }
}

hipError_t launch_within_count(const WithinArgs &a, hipStream_t stream)
{
    if (a.chunks == 0) return hipSuccess;
    if (a.ncols == 2u) hipLaunchKernelGGL(within_count_kernel<2>, dim3((uint32_t)a.chunks), dim3(WITHIN_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(within_count_kernel<1>, dim3((uint32_t)a.chunks), dim3(WITHIN_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_within_scan(const WithinArgs &a, hipStream_t stream)
{
    if (a.chunks == 0) return hipSuccess;
    hipLaunchKernelGGL(within_scan_kernel, dim3(1), dim3(WITHIN_SCAN_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_within_scatter(const WithinArgs &a, hipStream_t stream)
{
    if (a.chunks == 0 || a.capacity == 0) return hipSuccess;
    if (a.ncols == 2u) hipLaunchKernelGGL(within_scatter_kernel<2>, dim3((uint32_t)a.chunks), dim3(WITHIN_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(within_scatter_kernel<1>, dim3((uint32_t)a.chunks), dim3(WITHIN_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace skl
