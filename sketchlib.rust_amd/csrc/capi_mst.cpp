// capi_mst.cpp -- skl_self_mst / skl_clusters_from_edges: the minimum spanning forest of the distance graph, and the clusters a list
// of edges connects (mst.hip; the edge order, the key and the scratch layout: mst_plan.hpp).  The driver is Boruvka over
// capi_clusters.cpp's bands: every round cuts the whole triangle into the bands of a host-destined dense call (dense_plan.hpp
// plan_host_bands, under the same budget or SKL_PAIRS_BAND), each band is evaluated by dense_band() into scratch and the min-edge
// launch follows it on the context's stream; then the components choose, append and hook, the labels are flattened and the roots
// counted.  The 16-byte head is the only thing a round sends to the host.  The records travel once, after the last round, and
// are sorted there by the edge order.
#include "capi_internal.hpp"

#include <algorithm>
#include <string>
#include <vector>

using namespace skl;

namespace {

struct MstHead {
    uint32_t edges, error;
    unsigned long long roots;
};
static_assert(sizeof(MstHead) == MST_SCRATCH_HEAD_BYTES, "the head is read back in one copy");

}  // namespace

extern "C" int skl_self_mst(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, int column, double max_dist, uint32_t *out_i,
                            uint32_t *out_j, float *out_w, uint32_t *labels, uint64_t *n_edges, uint32_t *rounds)
{
    const RoctxRange range_("skl:mst");
    if (!n_edges || !rounds) return fail(SKL_ERR_INVALID_ARG, "n_edges or rounds is null");
    *n_edges = 0;
    *rounds = 0;
    if (!out_i || !out_j || !out_w) return fail(SKL_ERR_INVALID_ARG, "an edge output is null");
    SKL_TRY(check_params(s, s, p));
    const bool coreacc = p->dist_type == SKL_DIST_COREACC;
    const uint32_t ncols = coreacc ? 2u : 1u;
    if (!coreacc && p->ani) return fail(SKL_ERR_INVALID_ARG, "the tree is defined on distances, not on identities (p->ani)");
    if (column != 0 && !(column == 1 && coreacc)) {
        return fail(SKL_ERR_INVALID_ARG, "column %d of %u stored column%s", column, ncols, ncols == 2u ? "s" : "");
    }
    MstPred pred;
    if (!mst_pred_make(max_dist, (uint32_t)column, &pred)) return fail(SKL_ERR_INVALID_ARG, "max_dist = %g: a cap is a distance (not NaN, not negative)", max_dist);
    const int mode = coreacc ? MODE_COREACC : MODE_JACCARD;
    const int jout = coreacc ? 0 : JOUT_DIST;
    SKL_TRY(ctx_bind(ctx));
    const uint64_t n = s->n;
    if (n == 0) return SKL_OK;
    if (n > CLUSTER_MAX_SAMPLES) return fail(SKL_ERR_INVALID_ARG, "%llu samples: labels are u32", (unsigned long long)n);
    if (n == 1) {
        if (labels) labels[0] = 0;
        ctx->last_kernel.clear();
        return SKL_OK;
    }

    const MstLayout lay = mst_layout(n);
    void *ws = nullptr;
    SKL_TRY(ctx_scratch(ctx, lay.bytes, &ws, SCRATCH_MST));
    char *base = (char *)ws;
    MstHead *d_head = (MstHead *)ws;
    MstArgs a = {};
    a.labels = (uint32_t *)(base + lay.labels);
    a.n = n;
    a.ncols = ncols;
    a.pred = pred;
    a.best = (uint64_t *)(base + lay.best);
    a.comp_min = (uint64_t *)(base + lay.comp_min);
    a.comp_hi = (uint32_t *)(base + lay.comp_hi);
    a.rec_i = (uint32_t *)(base + lay.rec_i);
    a.rec_j = (uint32_t *)(base + lay.rec_j);
    a.rec_w = (float *)(base + lay.rec_w);
    a.n_edges = &d_head->edges;
    a.error = &d_head->error;
    ClusterArgs c = {};
    c.labels = a.labels;
    c.n = n;
    c.count = &d_head->roots;
    HIP_TRY(hipMemsetAsync(ws, 0, MST_SCRATCH_HEAD_BYTES, ctx->stream));
    HIP_TRY(launch_cluster_init(c, ctx->stream));

    const size_t rec = ncols * sizeof(float);
    const size_t budget = ctx->knobs.pairs_band > 0 ? (size_t)ctx->knobs.pairs_band * rec : BAND_BYTES;
    const HostBands plan = plan_host_bands(true, n, 0, n - 1, rec, budget);
    uint64_t widest = 0;
    for (const HostBand &b : plan.bands) widest = std::max(widest, b.pairs);
    if (!within_band_ok(widest)) return fail(SKL_ERR_INVALID_ARG, "a band of %llu pairs (2^32 or more)", (unsigned long long)widest);
    void *band = nullptr;
    SKL_TRY(ctx_scratch(ctx, within_band_bytes(widest, ncols), &band, SCRATCH_KEY_BAND));
    a.band = (const float *)band;

    std::string dense_name;
    MstHead head = {};
    uint32_t adding = 0;
    bool done = false;
    for (uint32_t round = 0; round < MST_MAX_ROUNDS && !done; ++round) {
        HIP_TRY(hipMemsetAsync(base + lay.fill_at, 0xFF, lay.fill_bytes, ctx->stream));   // best, comp_min, comp_hi: no offer
        for (const HostBand &b : plan.bands) {
            SKL_TRY(dense_band(ctx, s, s, p, mode, jout, 1, b.r0, b.r1, band));
            if (dense_name.empty()) dense_name = ctx->last_kernel;
            a.m = b.pairs;
            a.chunks = within_chunks(b.pairs);
            a.first = cond_index(b.r0, b.r0 + 1, n);
            HIP_TRY(launch_mst_min_edge(a, ctx->stream));
        }
        HIP_TRY(launch_mst_choose_and_hook(a, ctx->stream));
        HIP_TRY(launch_cluster_flatten(c, ctx->stream));
        HIP_TRY(hipMemsetAsync(&d_head->roots, 0, sizeof d_head->roots, ctx->stream));
        HIP_TRY(launch_cluster_count(c, ctx->stream));
        const uint32_t before = head.edges;
        HIP_TRY(hipMemcpyAsync(&head, d_head, sizeof head, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (head.edges == before) {
            done = true;   // a round that added no edge: every component is without an outgoing edge
            break;
        }
        ++adding;
        if ((uint64_t)head.edges + head.roots != n) {
            return fail(SKL_ERR_HIP, "internal: %u edges and %llu components of %llu samples", head.edges, head.roots, (unsigned long long)n);
        }
        done = (uint64_t)head.edges == n - 1;   // a tree: nothing is left to join
    }
    if (!done) return fail(SKL_ERR_HIP, "internal: the forest was not finished in %u rounds", MST_MAX_ROUNDS);

    const uint64_t found = head.edges;
    std::vector<uint32_t> ri(found), rj(found);
    std::vector<float> rw(found);
    if (found) {
        HIP_TRY(hipMemcpyAsync(ri.data(), a.rec_i, found * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(rj.data(), a.rec_j, found * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(rw.data(), a.rec_w, found * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (labels) HIP_TRY(hipMemcpyAsync(labels, a.labels, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<MstEdge> edges(found);
    for (uint64_t r = 0; r < found; ++r) edges[r] = MstEdge{ri[r], rj[r], rw[r]};
    std::sort(edges.begin(), edges.end(), mst_edge_less);
    for (uint64_t r = 0; r < found; ++r) {
        out_i[r] = edges[r].i;
        out_j[r] = edges[r].j;
        out_w[r] = edges[r].w;
    }
    *n_edges = found;
    *rounds = adding;
    ctx->last_kernel = dense_name + " + skl::mst_min_edge_kernel, skl::mst_offer_min_kernel, skl::mst_offer_hi_kernel, skl::mst_append_kernel, " +
                       "skl::mst_hook_kernel, skl::cluster_flatten_kernel, skl::cluster_count_kernel (minimum spanning forest, " + std::to_string(adding) +
                       " rounds added an edge, " + std::to_string(plan.bands.size()) + " bands a round)";
    return SKL_OK;
}

extern "C" int skl_clusters_from_edges(skl_ctx *ctx, const uint32_t *edge_i, const uint32_t *edge_j, uint64_t n_edges_in, uint64_t n,
                                       uint32_t *labels, uint64_t *n_clusters)
{
    const RoctxRange range_("skl:clusters from edges");
    if (!n_clusters) return fail(SKL_ERR_INVALID_ARG, "n_clusters is null");
    *n_clusters = 0;
    if (n_edges_in && (!edge_i || !edge_j)) return fail(SKL_ERR_INVALID_ARG, "an edge array is null");
    if (n == 0) {
        if (n_edges_in) return fail(SKL_ERR_INVALID_ARG, "an edge among 0 samples");
        return ctx ? SKL_OK : fail(SKL_ERR_INVALID_ARG, "null context");
    }
    if (!labels) return fail(SKL_ERR_INVALID_ARG, "labels is null");
    if (n > CLUSTER_MAX_SAMPLES) return fail(SKL_ERR_INVALID_ARG, "%llu samples: labels are u32", (unsigned long long)n);
    if (n_edges_in > CLUSTER_MAX_SAMPLES) return fail(SKL_ERR_INVALID_ARG, "%llu edges (2^32 or more)", (unsigned long long)n_edges_in);
    SKL_TRY(ctx_bind(ctx));
    const MstEdgesLayout lay = mst_edges_layout(n, n_edges_in);
    void *ws = nullptr;
    SKL_TRY(ctx_scratch(ctx, lay.bytes, &ws, SCRATCH_MST));
    char *base = (char *)ws;
    MstHead *d_head = (MstHead *)ws;
    MstArgs a = {};
    a.labels = (uint32_t *)(base + lay.labels);
    a.n = n;
    a.edge_i = (const uint32_t *)(base + lay.edge_i);
    a.edge_j = (const uint32_t *)(base + lay.edge_j);
    a.n_edges_in = n_edges_in;
    a.error = &d_head->error;
    ClusterArgs c = {};
    c.labels = a.labels;
    c.n = n;
    c.count = &d_head->roots;
    HIP_TRY(hipMemsetAsync(ws, 0, MST_SCRATCH_HEAD_BYTES, ctx->stream));
    if (n_edges_in) {
        HIP_TRY(hipMemcpyAsync(base + lay.edge_i, edge_i, n_edges_in * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(base + lay.edge_j, edge_j, n_edges_in * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    // CHECK before anything follows an index
    HIP_TRY(launch_mst_edges_check(a, ctx->stream));
    uint32_t error = 0;
    HIP_TRY(hipMemcpyAsync(&error, a.error, sizeof error, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (error) return fail(SKL_ERR_INVALID_ARG, "an edge names a sample >= n = %llu", (unsigned long long)n);
    HIP_TRY(launch_cluster_init(c, ctx->stream));
    HIP_TRY(launch_mst_edges_union(a, ctx->stream));
    HIP_TRY(launch_cluster_flatten(c, ctx->stream));
    HIP_TRY(launch_cluster_count(c, ctx->stream));
    unsigned long long count = 0;
    HIP_TRY(hipMemcpyAsync(&count, c.count, sizeof count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(labels, a.labels, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_clusters = count;
    ctx->last_kernel = (n_edges_in ? std::string("skl::mst_edges_check_kernel, skl::mst_edges_union_kernel, ") : std::string()) +
                       "skl::cluster_flatten_kernel, skl::cluster_count_kernel";
    return SKL_OK;
}
