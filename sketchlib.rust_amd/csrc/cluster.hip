// cluster.hip -- single-linkage clusters under a distance cap (gfx950, wave64) behind the dense kernels: skl_self_clusters_within
// and skl_clusters_merge (capi_clusters.cpp).  The band is the f32 buffer a dense call leaves in device memory; instead of listing
// the pairs that pass the cap (within.hip), the union kernel joins the two samples of each in a lock-free union-find over `labels`,
// one u32 per sample of the slab:
//   cluster_init_kernel / cluster_check_kernel   write the identity / verify labels[i] <= i (one error word), before anything follows a label
//   cluster_union_kernel<NCOLS>                  within.hip's chunking, 16-byte loads and ballots (within_wave.hpp); a lane that holds a passing
//                                                pair finds both roots and hooks the higher under the lower.  A chunk (a wave's span of one)
//                                                without a passing position does nothing.
//   cluster_merge_kernel                         union(i, other[i]) with the same device function
//   cluster_flatten_kernel                       labels[i] becomes its root
//   cluster_count_kernel                         the roots, exactly: a ballot and a popcount per wave, one integer atomic add per workgroup
// The label form, the grids and the sequential restatement (cluster_labels_host) are cluster_plan.hpp's; the device functions
// cluster_find(), cluster_shorten() and cluster_union() live in cluster_union.hpp, which mst.hip includes too.
//
// 1. INVARIANT.  Every value ever stored to labels[x] is an index <= x of x's own cluster: the identity, a checked input, a hook
//    of the root x under a LOWER root of a cluster it is being joined with, or a lower ancestor of x.  So a label only ever
//    decreases, a walk along labels strictly descends and ends within n steps whatever other lanes do meanwhile, and a root is
//    the lowest index of its tree.  cluster_union() retries only after a failed compare-and-swap, and continues from the value
//    that came back, which is strictly below the index it tried to hook: the sum of the two indices it holds falls with every
//    retry, so it ends.  No lane, wave or workgroup ever waits for a store of another: no spin, no flag, no grid barrier.  The
//    hook is atomicCAS(&labels[hi], hi, lo), never an atomic minimum: a minimum would replace a link another lane has just made
//    from hi to a third root and cut that root's tree off; the CAS fails instead and the lane goes on from that link.
// 2. PATH SHORTENING during the union launch: a relaxed agent-scope atomic minimum of labels[x] with the root just found, for the
//    two END POINTS of the pair only, and only when the end point did not already point straight at it.  The minimum keeps the
//    invariant (the root is an ancestor of x, hence <= x and of x's cluster; ancestors lie below x, so their own walks never pass
//    through x and nothing is cut off).  End points are what recurs -- a sample of a cluster of c members is an end point of c - 1
//    passing pairs -- so they end up pointing at the root after their first pair, and from then on a pair inside one cluster costs
//    two loads and NO atomic.  Inner nodes of a path are left to the flatten kernel after the last band: shortening them too
//    would issue an atomic per step for links that are mostly walked once.
// 3. LABEL ACCESSES inside the union, merge and flatten kernels are relaxed agent-scope atomic loads (__hip_atomic_load): the
//    per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores, so a plain load may
//    keep returning a value another lane replaced long ago.  Even an atomic load may be STALE by the time it is used, and that is
//    harmless: labels only decrease, so a stale value is an older, higher ancestor of the same cluster (the walk takes more
//    steps) or says "still a root" of an index that has been hooked since.  The second case reaches the CAS, which acts on memory
//    itself: it fails, returns the link, and the lane continues from it.  A stale "roots are equal" cannot happen: equal roots were
//    read from both walks, and two samples that were ever in one tree stay in one.  Launch boundaries on the one stream order
//    everything else: the init or the check before the first union, each band's union before the next, the last before the flatten,
//    the flatten before the count.
// 4. No scalar memory writes and no scalar atomics anywhere: plain C++ and vector atomics only.
#include "kernels.h"
#include "cluster_union.hpp"
#include "within_wave.hpp"

namespace skl {

__global__ __launch_bounds__(CLUSTER_THREADS) void cluster_init_kernel(const ClusterArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * CLUSTER_THREADS + threadIdx.x;
    if (i < a.n) a.labels[i] = (uint32_t)i;
}

// reads `labels` ([n], the caller's array as it came) and nothing through it
__global__ __launch_bounds__(CLUSTER_THREADS) void cluster_check_kernel(const uint32_t *__restrict__ labels, uint64_t n, uint32_t *error)
{
    const uint64_t i = (uint64_t)blockIdx.x * CLUSTER_THREADS + threadIdx.x;
    if (i < n && (uint64_t)labels[i] > i) *error = 1u;   // (every writer stores the same value)
}

template <uint32_t NCOLS>
__global__ __launch_bounds__(WITHIN_THREADS) void cluster_union_kernel(const ClusterArgs a)
{
    using W = WithinWave<NCOLS>;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t w0 = (uint64_t)blockIdx.x * WITHIN_CHUNK + (uint64_t)wave * WITHIN_WAVE_SPAN;
    if (w0 >= a.m) return;   // (wave-uniform; the kernel has no barrier)
    W w;
    if (w.load(a.band, a.m, a.pred, w0, lane) == 0u) return;
    uint32_t row, pos;
    within_locate(true, a.first + w0, a.n, &row, &pos);
#pragma unroll
    for (uint32_t t = 0; t < W::TRIPS; ++t) {
#pragma unroll
        for (uint32_t e = 0; e < W::V; ++e) {
            if (w.pass[t][e] >> lane & 1ull) {
                uint32_t i, j;
                within_step(true, a.n, row, pos, (t * 64u + lane) * W::V + e, &i, &j);
                cluster_union(a.labels, i, j);
            }
        }
    }
}

__global__ __launch_bounds__(CLUSTER_THREADS) void cluster_merge_kernel(const ClusterArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * CLUSTER_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t o = a.other[i];   // (checked: o <= i)
    if (o != (uint32_t)i) cluster_union(a.labels, (uint32_t)i, o);
}

__global__ __launch_bounds__(CLUSTER_THREADS) void cluster_flatten_kernel(const ClusterArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * CLUSTER_THREADS + threadIdx.x;
    if (i >= a.n) return;
    uint32_t direct;
    const uint32_t r = cluster_find(a.labels, (uint32_t)i, &direct);
    // (only this thread writes labels[i] in this launch; a root keeps itself, so no walk of another thread is cut short of its root)
    if (direct != r) __hip_atomic_store(a.labels + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CLUSTER_THREADS) void cluster_count_kernel(const ClusterArgs a)
{
    __shared__ uint32_t wave_sum[CLUSTER_THREADS / 64u];
    const uint64_t i = (uint64_t)blockIdx.x * CLUSTER_THREADS + threadIdx.x;
    const uint64_t roots = __ballot(i < a.n && a.labels[i] == (uint32_t)i);
    if ((threadIdx.x & 63u) == 0u) wave_sum[threadIdx.x >> 6] = (uint32_t)__popcll(roots);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < CLUSTER_THREADS / 64u; ++k) sum += wave_sum[k];
        if (sum) atomicAdd(a.count, (unsigned long long)sum);
    }
}

namespace {

inline dim3 sample_grid(uint64_t n) { return dim3((uint32_t)cluster_blocks(n)); }

}  // namespace

hipError_t launch_cluster_init(const ClusterArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(cluster_init_kernel, sample_grid(a.n), dim3(CLUSTER_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cluster_check(const ClusterArgs &a, const uint32_t *labels, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(cluster_check_kernel, sample_grid(a.n), dim3(CLUSTER_THREADS), 0, stream, labels, a.n, a.error);
    return hipGetLastError();
}

hipError_t launch_cluster_union(const ClusterArgs &a, hipStream_t stream)
{
    if (a.chunks == 0) return hipSuccess;
    if (a.ncols == 2u) hipLaunchKernelGGL(cluster_union_kernel<2>, dim3((uint32_t)a.chunks), dim3(WITHIN_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(cluster_union_kernel<1>, dim3((uint32_t)a.chunks), dim3(WITHIN_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cluster_merge(const ClusterArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(cluster_merge_kernel, sample_grid(a.n), dim3(CLUSTER_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cluster_flatten(const ClusterArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(cluster_flatten_kernel, sample_grid(a.n), dim3(CLUSTER_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_cluster_count(const ClusterArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(cluster_count_kernel, sample_grid(a.n), dim3(CLUSTER_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace skl
