// cluster_plan.hpp -- single-linkage clusters under a distance cap (cluster.hip, capi_clusters.cpp): the
// numbers of the launches, the scratch layout, and the SEQUENTIAL restatement of the kernels that
// tests/native/cluster_check.cpp checks against a brute-force component search.  No HIP header.
//
// A partition of n samples is an array of n u32 LABELS with labels[i] <= i: a forest whose edges point to lower indices, so
// every walk along labels descends and ends at a root (labels[r] == r), the lowest index of its tree.  The finished form is
// flat: labels[i] is the root itself.
//   UNION      the positions of a dense band that pass the cap (within_plan.hpp: the predicate, the chunking, the (i, j) of a
//              position) each join the trees of their two samples: the higher root is hooked under the lower
//   FLATTEN    labels[i] becomes its root
//   COUNT      the number of roots
//   CHECK      labels[i] <= i for every i: what makes a caller's array safe to follow (a value beyond i could leave the array)
//   MERGE      union(i, other[i]) over all i: the clusters connected through either of two partitions
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "within_plan.hpp"

namespace skl {

constexpr uint32_t CLUSTER_THREADS = 256;   // workgroup of the per-sample kernels (init, check, flatten, count, merge): one sample a thread
inline uint64_t cluster_blocks(uint64_t n) { return (n + CLUSTER_THREADS - 1u) / CLUSTER_THREADS; }
constexpr uint64_t CLUSTER_MAX_SAMPLES = 0xFFFFFFFFull;   // labels are u32, and the per-sample grids stay below 2^24 workgroups

// scratch: two words in a 16-byte slot -- [0] the check's error word (u32), [1] the root count (u64) -- then the label
// array(s) when the caller's live on the host
constexpr size_t CLUSTER_SCRATCH_HEAD_BYTES = 16;
inline size_t cluster_scratch_bytes(uint64_t n_labels_on_host) { return CLUSTER_SCRATCH_HEAD_BYTES + (size_t)n_labels_on_host * sizeof(uint32_t); }

inline void cluster_init_host(uint32_t *labels, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) labels[i] = (uint32_t)i;
}
// CHECK: reads, never writes
inline bool cluster_labels_ok_host(const uint32_t *labels, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) {
        if (labels[i] > i) return false;
    }
    return true;
}
inline uint32_t cluster_find_host(const uint32_t *labels, uint32_t x)
{
    while (labels[x] != x) x = labels[x];
    return x;
}
inline void cluster_union_host(uint32_t *labels, uint32_t a, uint32_t b)
{
    const uint32_t ra = cluster_find_host(labels, a), rb = cluster_find_host(labels, b);
    if (ra == rb) return;
    if (ra < rb) labels[rb] = ra;
    else labels[ra] = rb;
}
// FLATTEN + COUNT (ascending: labels[i]'s own label is flat by the time i is reached)
inline uint64_t cluster_finish_host(uint32_t *labels, uint64_t n)
{
    uint64_t roots = 0;
    for (uint64_t i = 0; i < n; ++i) {
        labels[i] = labels[labels[i]];
        roots += labels[i] == i ? 1u : 0u;
    }
    return roots;
}

// One band of a self call on the host, as the union kernel walks it: chunk by chunk and wave by wave, each wave from the
// (row, position) of its first pair, every passing position's (i, j) joined; then flatten and count.  dense: m x ncols values,
// the first one at condensed position `first` of n samples; labels: a checked partition of the n samples (the identity, or
// what an earlier band left).  Returns the number of clusters.
inline uint64_t cluster_labels_host(const float *dense, uint64_t m, uint32_t ncols, uint64_t n, uint64_t first, const WithinPred &q,
                                    uint32_t *labels)
{
    for (uint64_t c = 0; c < within_chunks(m); ++c) {
        for (uint32_t w = 0; w < WITHIN_WAVES; ++w) {
            const uint64_t w0 = c * WITHIN_CHUNK + (uint64_t)w * WITHIN_WAVE_SPAN;
            if (w0 >= m) break;
            uint32_t row, pos;
            within_locate(true, first + w0, n, &row, &pos);
            for (uint32_t a = 0; a < WITHIN_WAVE_SPAN && w0 + a < m; ++a) {
                const uint64_t p = w0 + a;
                if (!within_keep(q, dense[p * ncols], ncols == 2u ? dense[p * ncols + 1u] : 0.0f)) continue;
                uint32_t i, j;
                within_step(true, n, row, pos, a, &i, &j);
                cluster_union_host(labels, i, j);
            }
        }
    }
    return cluster_finish_host(labels, n);
}

// MERGE on the host.  false: one of the two arrays fails the check, and nothing was written.
inline bool cluster_merge_host(uint32_t *labels, const uint32_t *other, uint64_t n, uint64_t *n_clusters)
{
    if (!cluster_labels_ok_host(labels, n) || !cluster_labels_ok_host(other, n)) return false;
    for (uint64_t i = 0; i < n; ++i) cluster_union_host(labels, (uint32_t)i, other[i]);
    *n_clusters = cluster_finish_host(labels, n);
    return true;
}

}  // namespace skl
