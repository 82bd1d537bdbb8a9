// cluster_union.hpp -- the lock-free union-find on a label array (device code): the walk to a root, the shortening of an end point
// and the hook, shared by cluster.hip (its union, merge and flatten kernels; the invariants are argued in its head comment, 1-3)
// and mst.hip (the hook of a Boruvka round, the edges of skl_clusters_from_edges).  The label form is cluster_plan.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace skl {

__device__ __forceinline__ uint32_t label_load(const uint32_t *labels, uint32_t x)
{
    return __hip_atomic_load(labels + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x: strictly descending (invariant 1).  *direct: labels[x] as first read
__device__ __forceinline__ uint32_t cluster_find(const uint32_t *labels, uint32_t x, uint32_t *direct)
{
    uint32_t p = label_load(labels, x);
    *direct = p;
    while (p != x) {
        x = p;
        p = label_load(labels, x);
    }
    return x;
}

// end point x, whose label read `direct`, has root r: point it there unless it did (or is the root)
__device__ __forceinline__ void cluster_shorten(uint32_t *labels, uint32_t x, uint32_t direct, uint32_t r)
{
    if (direct != r) (void)__hip_atomic_fetch_min(labels + x, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void cluster_union(uint32_t *labels, uint32_t a, uint32_t b)
{
    uint32_t da, db;
    uint32_t ra = cluster_find(labels, a, &da), rb = cluster_find(labels, b, &db);
    const bool same = ra == rb;   // the read-only test, before any atomic: inside a clonal cluster nearly every pair ends here
    cluster_shorten(labels, a, da, ra);
    cluster_shorten(labels, b, db, rb);
    if (same) return;
    for (;;) {
        const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const uint32_t seen = atomicCAS(labels + hi, hi, lo);
        if (seen == hi) return;                 // hooked
        // hi had been hooked by another lane, under seen < hi: go on from there (hi + lo falls with every turn)
        uint32_t unused;
        ra = cluster_find(labels, seen, &unused);
        rb = cluster_find(labels, lo, &unused);
        if (ra == rb) return;
    }
}

}  // namespace skl
