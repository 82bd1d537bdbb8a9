// mst.hip -- the minimum spanning forest of the distance graph (gfx950, wave64) behind the dense kernels: skl_self_mst and
// skl_clusters_from_edges (capi_mst.cpp).  Boruvka: every round reads the whole triangle once more, band by band, and each
// component picks its smallest outgoing edge under the strict total order (w, i, j) of mst_plan.hpp, which makes the forest a
// property of the data alone.  The key, the words, the scratch layout and the sequential restatement are mst_plan.hpp's.
//   mst_min_edge_kernel<NCOLS>   within.hip's chunking, 16-byte loads and ballots (within_wave.hpp).  A position is LIVE where its
//                                weight is an edge and labels[i] != labels[j]; it offers key << 32 | j to best[i] and
//                                key << 32 | i to best[j], both by 64-bit atomic minimum
//   mst_offer_min_kernel         per sample: key << 32 | lo of its best edge to comp_min[its root]
//   mst_offer_hi_kernel          per sample whose offer is that minimum: hi to comp_hi[its root]
//   mst_append_kernel            per root that chose an edge: the record, its slot from an atomic counter -- unless the component at
//                                the other end chose the same edge and has the lower root.  Reads labels, writes none
//   mst_hook_kernel              per root that chose an edge: cluster_union(lo, hi) (cluster_union.hpp)
//   mst_edges_check_kernel / mst_edges_union_kernel   skl_clusters_from_edges: an index >= n sets the error word; union per edge
// cluster.hip's init, flatten and count kernels do the rest.
//
// 1. WHY best[x] IS ENOUGH.  At the smallest weight the smallest OTHER end is the smallest edge of x under (w, lo, hi): the edges
//    to o < x are (o, x), ascending in o; those to o > x are (x, o), ascending in o; and every o < x has lo = o < x, before all of
//    the second kind.  A component's smallest outgoing edge is the smallest of its samples' best edges.
// 2. LABELS are flat and constant during the min-edge launch (the flatten kernel ran, nothing writes them): plain loads.  After
//    the first round most pairs lie inside one component and end at the label compare, with no atomic.
// 3. ROW SIDE.  A wave's 512 consecutive positions lie in one row i, sometimes two, and in many rows only near the tip of the
//    triangle (rows shorter than 256 pairs).  Each lane keeps the minimum of its offers to the wave's FIRST row and to the one
//    after it in two registers; after the last trip two cross-lane minima leave ONE atomic per row.  Offers to rows beyond those
//    two are reduced row by row on the spot (a ballot picks a row, its lanes' minimum goes out through one lane), so the result is
//    right however many rows a span covers -- at n <= 65 every span covers several.  Without this a row's best would take an
//    atomic from every one of its n - 1 - i pairs, all to one address.
// 4. COLUMN SIDE.  Within a row j is consecutive across a wave's lanes, so best[j ..] is one coalesced read; it is read first, and
//    the atomic is issued only where the offer is smaller.  best[] only ever DECREASES during a launch (every writer is an atomic
//    minimum), so a stale read returns an older, LARGER value: it lets a useless atomic through and never suppresses a needed one.
//    The read is a relaxed agent-scope atomic load, so that it is served past the L1 and the per-XCD L2, where a line would stay
//    stale for the whole launch.  A column's offers arrive row after row in an order unrelated to their weights, and a running
//    minimum over a random order improves about ln n times: after the first rows nearly every offer loses at the read.  The same
//    read stands before the row side's atomics and before those of the two per-sample kernels.
// 5. TERMINATION.  Nothing spins or waits for another lane: the only device loops are the row-by-row reduction (one row leaves
//    the ballot per turn), within_step's walk over rows, and the descending walks of cluster_union.hpp, whose argument
//    (cluster.hip, 1) carries over: labels only decrease.  The hook reads its choice from comp_min / comp_hi, which no kernel of
//    that launch writes.  The append kernel runs BEFORE the hook kernel because it needs the flat labels to name the component at
//    the other end.  Choices under a strict total order never close a cycle, so every hook joins two trees and the slots never
//    exceed n - 1 (a slot beyond that is dropped, not written).
// 6. No scalar memory writes and no scalar atomics anywhere: plain C++ and vector atomics only.
#include "kernels.h"
#include "cluster_union.hpp"
#include "within_wave.hpp"

// 0: every live position sends its own atomic to best[i] (timing only: what the reduction of 3. buys, profiles/mst.md)
#ifndef MST_ROW_REDUCE
#define MST_ROW_REDUCE 1
#endif

namespace skl {

namespace {

__device__ __forceinline__ uint64_t word_load(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// *p = min(*p, offer), the atomic only where the word as read is above the offer (4.)
__device__ __forceinline__ void word_min(uint64_t *p, uint64_t offer)
{
    if (offer < word_load(p)) (void)__hip_atomic_fetch_min(p, offer, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t wave_min(uint64_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)(v >> 32), off);
        const uint64_t o = (uint64_t)hi << 32 | lo;
        v = o < v ? o : v;
    }
    return v;
}

}  // namespace

template <uint32_t NCOLS>
__global__ __launch_bounds__(WITHIN_THREADS) void mst_min_edge_kernel(const MstArgs a)
{
    using W = WithinWave<NCOLS>;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t w0 = (uint64_t)blockIdx.x * WITHIN_CHUNK + (uint64_t)wave * WITHIN_WAVE_SPAN;
    if (w0 >= a.m) return;   // (wave-uniform; the kernel has no barrier)
    W w;
    const MstPred pred = a.pred;
    if (w.load_if(a.band, a.m, w0, lane, [&pred](float v0, float v1) { return mst_keep(pred, v0, v1); }) == 0u) return;
    uint32_t row, pos;
    within_locate(true, a.first + w0, a.n, &row, &pos);
    uint64_t first_row = MST_EMPTY, second_row = MST_EMPTY;   // this lane's offers to best[row] and best[row + 1]
#pragma unroll
    for (uint32_t t = 0; t < W::TRIPS; ++t) {
        const float f[4] = {w.v[t].x, w.v[t].y, w.v[t].z, w.v[t].w};
#pragma unroll
        for (uint32_t e = 0; e < W::V; ++e) {
            uint32_t i = 0, j = 0;
            bool live = false;
            if (w.pass[t][e] >> lane & 1ull) {
                within_step(true, a.n, row, pos, (t * 64u + lane) * W::V + e, &i, &j);
                live = a.labels[i] != a.labels[j];
            }
            if (__ballot(live) == 0ull) continue;   // (wave-uniform)
            uint64_t to_row = MST_EMPTY;
            if (live) {
                const uint32_t key = mst_key(NCOLS == 2u && pred.column ? f[e * NCOLS + 1u] : f[e * NCOLS]);
                word_min(a.best + j, mst_offer(key, i));
                to_row = mst_offer(key, j);
            }
#if MST_ROW_REDUCE
            if (live && i == row) first_row = to_row < first_row ? to_row : first_row;
            if (live && i == row + 1u) second_row = to_row < second_row ? to_row : second_row;
            const bool far = live && i > row + 1u;
            uint64_t rest = __ballot(far);
            while (rest) {   // (wave-uniform: one row leaves `rest` per turn)
                const int leader = __ffsll((unsigned long long)rest) - 1;
                const uint32_t r = __shfl(i, leader);
                const bool mine = far && i == r;
                const uint64_t least = wave_min(mine ? to_row : MST_EMPTY);
                if ((int)lane == leader) word_min(a.best + r, least);
                rest &= ~__ballot(mine);
            }
#else
            if (live) word_min(a.best + i, to_row);
#endif
        }
    }
#if MST_ROW_REDUCE
    first_row = wave_min(first_row);
    second_row = wave_min(second_row);
    if (lane == 0u) {
        if (first_row != MST_EMPTY) word_min(a.best + row, first_row);
        if (second_row != MST_EMPTY) word_min(a.best + row + 1u, second_row);   // (an offer came from a pair of that row: it exists)
    }
#endif
}

__global__ __launch_bounds__(CLUSTER_THREADS) void mst_offer_min_kernel(const MstArgs a)
{
    const uint64_t x = (uint64_t)blockIdx.x * CLUSTER_THREADS + threadIdx.x;
    if (x >= a.n) return;
    const uint64_t b = a.best[x];
    if (b == MST_EMPTY) return;
    const uint32_t o = mst_offer_sample(b), lo = o < x ? o : (uint32_t)x;
    word_min(a.comp_min + a.labels[x], mst_offer(mst_offer_key(b), lo));
}

__global__ __launch_bounds__(CLUSTER_THREADS) void mst_offer_hi_kernel(const MstArgs a)
{
    const uint64_t x = (uint64_t)blockIdx.x * CLUSTER_THREADS + threadIdx.x;
    if (x >= a.n) return;
    const uint64_t b = a.best[x];
    if (b == MST_EMPTY) return;
    const uint32_t o = mst_offer_sample(b), lo = o < x ? o : (uint32_t)x, hi = o < x ? (uint32_t)x : o;
    const uint32_t root = a.labels[x];
    if (mst_offer(mst_offer_key(b), lo) != a.comp_min[root]) return;   // (the offer kernel has finished: plain load)
    uint32_t *p = a.comp_hi + root;
    if (hi < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) (void)__hip_atomic_fetch_min(p, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CLUSTER_THREADS) void mst_append_kernel(const MstArgs a)
{
    const uint64_t r = (uint64_t)blockIdx.x * CLUSTER_THREADS + threadIdx.x;
    if (r >= a.n) return;
    const uint64_t chosen = a.comp_min[r];
    if (chosen == MST_EMPTY) return;   // (only a root ever received an offer)
    if (!mst_root_appends(a.labels, a.comp_min, a.comp_hi, (uint32_t)r)) return;
    const uint32_t slot = atomicAdd(a.n_edges, 1u);
    if ((uint64_t)slot + 1u >= a.n) return;   // (never: 5.)
    a.rec_i[slot] = mst_offer_sample(chosen);
    a.rec_j[slot] = a.comp_hi[r];
    a.rec_w[slot] = mst_key_weight(mst_offer_key(chosen));
}

__global__ __launch_bounds__(CLUSTER_THREADS) void mst_hook_kernel(const MstArgs a)
{
    const uint64_t r = (uint64_t)blockIdx.x * CLUSTER_THREADS + threadIdx.x;
    if (r >= a.n) return;
    const uint64_t chosen = a.comp_min[r];
    if (chosen != MST_EMPTY) cluster_union(a.labels, mst_offer_sample(chosen), a.comp_hi[r]);
}

// reads the edges as they came and nothing through them
__global__ __launch_bounds__(CLUSTER_THREADS) void mst_edges_check_kernel(const MstArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * CLUSTER_THREADS + threadIdx.x;
    if (k < a.n_edges_in && ((uint64_t)a.edge_i[k] >= a.n || (uint64_t)a.edge_j[k] >= a.n)) *a.error = 1u;   // (every writer stores the same value)
}

__global__ __launch_bounds__(CLUSTER_THREADS) void mst_edges_union_kernel(const MstArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * CLUSTER_THREADS + threadIdx.x;
    if (k < a.n_edges_in) cluster_union(a.labels, a.edge_i[k], a.edge_j[k]);   // (checked: both below n)
}

hipError_t launch_mst_min_edge(const MstArgs &a, hipStream_t stream)
{
    if (a.chunks == 0) return hipSuccess;
    if (a.ncols == 2u) hipLaunchKernelGGL(mst_min_edge_kernel<2>, dim3((uint32_t)a.chunks), dim3(WITHIN_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(mst_min_edge_kernel<1>, dim3((uint32_t)a.chunks), dim3(WITHIN_THREADS), 0, stream, a);
    return hipGetLastError();
}

// offer (min), offer (hi), append, hook: one sample a thread each, in this order on the one stream
hipError_t launch_mst_choose_and_hook(const MstArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    const dim3 grid((uint32_t)cluster_blocks(a.n)), block(CLUSTER_THREADS);
    hipLaunchKernelGGL(mst_offer_min_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(mst_offer_hi_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(mst_append_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(mst_hook_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_mst_edges_check(const MstArgs &a, hipStream_t stream)
{
    if (a.n_edges_in == 0) return hipSuccess;
    hipLaunchKernelGGL(mst_edges_check_kernel, dim3((uint32_t)cluster_blocks(a.n_edges_in)), dim3(CLUSTER_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_mst_edges_union(const MstArgs &a, hipStream_t stream)
{
    if (a.n_edges_in == 0) return hipSuccess;
    hipLaunchKernelGGL(mst_edges_union_kernel, dim3((uint32_t)cluster_blocks(a.n_edges_in)), dim3(CLUSTER_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace skl
