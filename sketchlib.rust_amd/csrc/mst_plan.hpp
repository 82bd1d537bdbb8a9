// mst_plan.hpp -- the minimum spanning forest of the distance graph (mst.hip, capi_mst.cpp): the edge order and its
// device key, the predicate, the scratch layout, and the SEQUENTIAL restatement of a whole call (mst_forest_host) that
// tests/native/mst_check.cpp checks against a plain Kruskal.  No HIP header.
//
// GRAPH     the n samples of a slab; the weight of {i, j} is the f32 value the dense call stores for the pair in one chosen column;
//           a pair is an edge where its weight is not a NaN and <= the cap (a float)
// ORDER     edges compare by (w, i, j) with i < j, w as a float with -0.0f == +0.0f.  On the device w becomes mst_key(w): a u32 that
//           is monotone in w + 0.0f.  The order is strict and total, so the minimum spanning forest under it is UNIQUE: it is what
//           Kruskal over the edges sorted by (mst_key(w), i, j) leaves, whatever the schedule that found it
// ROUND     Boruvka.  best[x] = min over the live pairs {x, o} (an edge whose ends carry different labels) of key << 32 | o: at the
//           smallest weight the smallest OTHER end is the smallest edge, for o < x (the edges (o, x), ascending in o) as for o > x
//           (the edges (x, o), ascending in o), and every o < x comes before every o > x.  A component's choice takes two steps with
//           64-bit words: comp_min[root] = min of key << 32 | lo over its samples, then comp_hi[root] = min of hi over the samples
//           whose offer equals that minimum.  Every root that chose an edge appends it (when both ends chose the same edge, the lower
//           root alone) and joins the two ends in the union-find of cluster_plan.hpp; then flatten and count.
// The call stops after a round that added no edge, or as soon as n - 1 edges are there; a round that adds one at least doubles
// the smallest component that still has an outgoing edge, so rounds <= log2 n, and the host loop gives up beyond MST_MAX_ROUNDS.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "cluster_plan.hpp"

namespace skl {

constexpr uint32_t MST_MAX_ROUNDS = 32;             // labels are u32: more rounds than that cannot add an edge each
constexpr uint64_t MST_EMPTY = ~0ull;               // best[] / comp_min[] without an offer: above every key << 32 | sample
constexpr uint32_t MST_NO_SAMPLE = 0xFFFFFFFFu;     // comp_hi[] without an offer (a sample index is < CLUSTER_MAX_SAMPLES)

// THE KEY: a u32 whose unsigned order is the float order of w + 0.0f (which turns -0.0f into +0.0f and leaves every other value):
// negative floats have their bits turned over, the others get the top bit.  Never called on a NaN (not an edge).
SKL_WITHIN_HD inline uint32_t mst_key(float w)
{
    const float z = w + 0.0f;
    uint32_t u;
    __builtin_memcpy(&u, &z, sizeof u);
    return u & 0x80000000u ? ~u : u | 0x80000000u;
}
// ... and back: the weight an edge is reported with (the stored value; a stored -0.0f comes back as +0.0f)
SKL_WITHIN_HD inline float mst_key_weight(uint32_t key)
{
    const uint32_t u = key & 0x80000000u ? key & 0x7FFFFFFFu : ~key;
    float w;
    __builtin_memcpy(&w, &u, sizeof w);
    return w;
}
SKL_WITHIN_HD inline uint64_t mst_offer(uint32_t key, uint32_t sample) { return (uint64_t)key << 32 | sample; }
SKL_WITHIN_HD inline uint32_t mst_offer_key(uint64_t offer) { return (uint32_t)(offer >> 32); }
SKL_WITHIN_HD inline uint32_t mst_offer_sample(uint64_t offer) { return (uint32_t)offer; }

// THE PREDICATE on the two stored values of a position (v1: anything with one column).  False for a NaN weight.
struct MstPred {
    float cap = 0.0f;
    uint32_t column = 0;
};
// false: the cap is NaN or negative (the caller's SKL_ERR_INVALID_ARG)
inline bool mst_pred_make(double max_dist, uint32_t column, MstPred *q)
{
    if (max_dist != max_dist || max_dist < 0.0) return false;
    q->cap = (float)max_dist;
    q->column = column;
    return true;
}
SKL_WITHIN_HD inline float mst_weight(const MstPred &q, float v0, float v1) { return q.column ? v1 : v0; }
SKL_WITHIN_HD inline bool mst_keep(const MstPred &q, float v0, float v1) { return mst_weight(q, v0, v1) <= q.cap; }

// the edge order on (w, i, j) records
struct MstEdge {
    uint32_t i, j;
    float w;
};
inline bool mst_edge_less(const MstEdge &a, const MstEdge &b)
{
    const uint32_t ka = mst_key(a.w), kb = mst_key(b.w);
    if (ka != kb) return ka < kb;
    if (a.i != b.i) return a.i < b.i;
    return a.j < b.j;
}

// SCRATCH (one slot): a 16-byte head -- [0] u32 the edges appended so far, [4] u32 an error word (an edge index >= n),
// [8] u64 the root count -- then labels[n] u32, best[n] u64, comp_min[n] u64, comp_hi[n] u32 and the records rec_i[n], rec_j[n]
// (u32), rec_w[n] (f32); every array starts on a 16-byte boundary.  best, comp_min and comp_hi are one run of bytes, so that one
// fill with 0xFF empties the three of them.
constexpr size_t MST_SCRATCH_HEAD_BYTES = 16;
inline size_t mst_align16(size_t b) { return (b + 15u) / 16u * 16u; }
struct MstLayout {
    size_t labels, best, comp_min, comp_hi, rec_i, rec_j, rec_w, bytes;
    size_t fill_at, fill_bytes;   // best .. the end of comp_hi
};
inline MstLayout mst_layout(uint64_t n)
{
    MstLayout l;
    size_t at = MST_SCRATCH_HEAD_BYTES;
    l.labels = at, at = mst_align16(at + (size_t)n * sizeof(uint32_t));
    l.best = at, at = mst_align16(at + (size_t)n * sizeof(uint64_t));
    l.comp_min = at, at = mst_align16(at + (size_t)n * sizeof(uint64_t));
    l.comp_hi = at, at = mst_align16(at + (size_t)n * sizeof(uint32_t));
    l.fill_at = l.best, l.fill_bytes = at - l.best;
    l.rec_i = at, at = mst_align16(at + (size_t)n * sizeof(uint32_t));
    l.rec_j = at, at = mst_align16(at + (size_t)n * sizeof(uint32_t));
    l.rec_w = at, at = mst_align16(at + (size_t)n * sizeof(float));
    l.bytes = at;
    return l;
}
// skl_clusters_from_edges: the head, labels[n], then the staged edge_i[e], edge_j[e]
struct MstEdgesLayout {
    size_t labels, edge_i, edge_j, bytes;
};
inline MstEdgesLayout mst_edges_layout(uint64_t n, uint64_t n_edges)
{
    MstEdgesLayout l;
    size_t at = MST_SCRATCH_HEAD_BYTES;
    l.labels = at, at = mst_align16(at + (size_t)n * sizeof(uint32_t));
    l.edge_i = at, at = mst_align16(at + (size_t)n_edges * sizeof(uint32_t));
    l.edge_j = at, at = mst_align16(at + (size_t)n_edges * sizeof(uint32_t));
    l.bytes = at;
    return l;
}

// ---- the per-sample steps of a round on the host, one loop per kernel ----
// OFFER 1: comp_min[root] = min (key << 32 | lo) over the samples of the component that hold an offer
inline void mst_offer_min_host(const uint32_t *labels, const uint64_t *best, uint64_t *comp_min, uint64_t n)
{
    for (uint64_t x = 0; x < n; ++x) {
        if (best[x] == MST_EMPTY) continue;
        const uint32_t o = mst_offer_sample(best[x]), lo = o < x ? o : (uint32_t)x;
        comp_min[labels[x]] = std::min(comp_min[labels[x]], mst_offer(mst_offer_key(best[x]), lo));
    }
}
// OFFER 2: comp_hi[root] = min hi over the samples whose offer is that minimum
inline void mst_offer_hi_host(const uint32_t *labels, const uint64_t *best, const uint64_t *comp_min, uint32_t *comp_hi, uint64_t n)
{
    for (uint64_t x = 0; x < n; ++x) {
        if (best[x] == MST_EMPTY) continue;
        const uint32_t o = mst_offer_sample(best[x]), lo = o < x ? o : (uint32_t)x, hi = o < x ? (uint32_t)x : o;
        if (mst_offer(mst_offer_key(best[x]), lo) == comp_min[labels[x]]) comp_hi[labels[x]] = std::min(comp_hi[labels[x]], hi);
    }
}
// does root r append its choice?  Not when the component at the other end chose the same edge and has the lower root.  Reads
// flat labels (before any hook of the round).
SKL_WITHIN_HD inline bool mst_root_appends(const uint32_t *labels, const uint64_t *comp_min, const uint32_t *comp_hi, uint32_t r)
{
    const uint32_t lo = mst_offer_sample(comp_min[r]), hi = comp_hi[r];
    const uint32_t other = labels[lo] == r ? labels[hi] : labels[lo];
    return !(other < r && comp_min[other] == comp_min[r] && comp_hi[other] == comp_hi[r]);
}

// A WHOLE CALL on the host over the dense array of all n (n - 1) / 2 pairs (ncols values each), as the kernels walk it: the
// min-edge kernel chunk by chunk and wave by wave, each wave from the (row, position) of its first pair; then the two offers, the
// append, the hook, flatten and count; round after round.  out: room for n - 1 edges, sorted by the edge order on return;
// labels: n u32 (flat, lowest index of the component).  false: more than MST_MAX_ROUNDS rounds (never, by the halving argument).
inline bool mst_forest_host(const float *dense, uint64_t n, uint32_t ncols, const MstPred &q, MstEdge *out, uint32_t *labels, uint64_t *n_edges,
                            uint32_t *rounds)
{
    *n_edges = 0;
    *rounds = 0;
    cluster_init_host(labels, n);
    if (n < 2) return true;
    const uint64_t m = n * (n - 1u) / 2u;
    std::vector<uint64_t> best(n), comp_min(n);
    std::vector<uint32_t> comp_hi(n);
    uint64_t edges = 0;
    for (uint32_t round = 0; round < MST_MAX_ROUNDS; ++round) {
        std::fill(best.begin(), best.end(), MST_EMPTY);
        std::fill(comp_min.begin(), comp_min.end(), MST_EMPTY);
        std::fill(comp_hi.begin(), comp_hi.end(), MST_NO_SAMPLE);
        // MIN EDGE
        for (uint64_t c = 0; c < within_chunks(m); ++c) {
            for (uint32_t w = 0; w < WITHIN_WAVES; ++w) {
                const uint64_t w0 = c * WITHIN_CHUNK + (uint64_t)w * WITHIN_WAVE_SPAN;
                if (w0 >= m) break;
                uint32_t row, pos;
                within_locate(true, w0, n, &row, &pos);
                for (uint32_t a = 0; a < WITHIN_WAVE_SPAN && w0 + a < m; ++a) {
                    const uint64_t p = w0 + a;
                    const float v0 = dense[p * ncols], v1 = ncols == 2u ? dense[p * ncols + 1u] : 0.0f;
                    if (!mst_keep(q, v0, v1)) continue;
                    uint32_t i, j;
                    within_step(true, n, row, pos, a, &i, &j);
                    if (labels[i] == labels[j]) continue;
                    const uint32_t key = mst_key(mst_weight(q, v0, v1));
                    best[i] = std::min(best[i], mst_offer(key, j));
                    best[j] = std::min(best[j], mst_offer(key, i));
                }
            }
        }
        mst_offer_min_host(labels, best.data(), comp_min.data(), n);
        mst_offer_hi_host(labels, best.data(), comp_min.data(), comp_hi.data(), n);
        // APPEND (labels still flat), then HOOK
        const uint64_t before = edges;
        for (uint64_t r = 0; r < n; ++r) {
            if (labels[r] != r || comp_min[r] == MST_EMPTY) continue;
            if (!mst_root_appends(labels, comp_min.data(), comp_hi.data(), (uint32_t)r)) continue;
            if (edges >= n - 1u) return false;   // (a cycle: never, under a strict total order)
            out[edges++] = MstEdge{mst_offer_sample(comp_min[r]), comp_hi[r], mst_key_weight(mst_offer_key(comp_min[r]))};
        }
        for (uint64_t r = 0; r < n; ++r) {
            // (labels[r] may have been hooked by a lower root meanwhile: the choice is the one made as a root, comp_min[r] says so)
            if (comp_min[r] != MST_EMPTY) cluster_union_host(labels, mst_offer_sample(comp_min[r]), comp_hi[r]);
        }
        const uint64_t roots = cluster_finish_host(labels, n);
        if (edges == before) break;
        ++*rounds;
        if (edges + roots != n) return false;
        if (edges == n - 1u) break;
        if (round + 1u == MST_MAX_ROUNDS) return false;
    }
    std::sort(out, out + edges, mst_edge_less);
    *n_edges = edges;
    return true;
}

// skl_clusters_from_edges on the host.  false: an index >= n, and nothing was written.
inline bool mst_clusters_from_edges_host(const uint32_t *edge_i, const uint32_t *edge_j, uint64_t n_edges, uint64_t n, uint32_t *labels,
                                         uint64_t *n_clusters)
{
    for (uint64_t k = 0; k < n_edges; ++k) {
        if (edge_i[k] >= n || edge_j[k] >= n) return false;
    }
    cluster_init_host(labels, n);
    for (uint64_t k = 0; k < n_edges; ++k) cluster_union_host(labels, edge_i[k], edge_j[k]);
    *n_clusters = cluster_finish_host(labels, n);
    return true;
}

}  // namespace skl
