// capi_clusters.cpp -- skl_self_clusters_within / skl_clusters_merge: single-linkage clusters under a distance cap, as one label
// per sample (cluster.hip; the label form, the grids and the scratch layout: cluster_plan.hpp).  The driver is capi_within.cpp's:
// the row range is cut into the bands of a host-destined dense call (dense_plan.hpp plan_host_bands, under the same budget or
// SKL_PAIRS_BAND), each band is evaluated by dense_band() into scratch, and the union launch follows it on the context's stream.
// The labels stay in device memory from the init (or the check) to the count: nothing goes to the host between bands, and the
// flatten and the count run once after the last band.  A caller's host array travels through SCRATCH_CLUSTER_LABELS.
#include "capi_internal.hpp"

#include <algorithm>
#include <string>

using namespace skl;

namespace {

// The labels on the device and the two words beside them.  Host arrays are staged in scratch behind the 16-byte head.
struct ClusterBuffers {
    uint32_t *d_labels = nullptr, *d_other = nullptr;
    uint32_t *error = nullptr;
    unsigned long long *count = nullptr;
};

int cluster_buffers(skl_ctx *ctx, uint32_t *labels, const uint32_t *other, uint64_t n, bool on_device, ClusterBuffers *b)
{
    const uint64_t staged = on_device ? 0 : (other ? 2 * n : n);
    void *ws = nullptr;
    SKL_TRY(ctx_scratch(ctx, cluster_scratch_bytes(staged), &ws, SCRATCH_CLUSTER_LABELS));
    b->error = (uint32_t *)ws;
    b->count = (unsigned long long *)((char *)ws + 8);
    uint32_t *stage = (uint32_t *)((char *)ws + CLUSTER_SCRATCH_HEAD_BYTES);
    b->d_labels = on_device ? labels : stage;
    b->d_other = on_device ? const_cast<uint32_t *>(other) : stage + n;
    HIP_TRY(hipMemsetAsync(ws, 0, CLUSTER_SCRATCH_HEAD_BYTES, ctx->stream));
    return SKL_OK;
}

// CHECK of one array as the caller handed it over (staged first when it lives on the host): SKL_ERR_INVALID_ARG before anything
// follows one of its values.  Nothing has been written to the caller's memory by then.
int cluster_checked(skl_ctx *ctx, const ClusterArgs &a, const uint32_t *src, uint32_t *d_array, bool on_device, const char *what)
{
    if (!on_device) HIP_TRY(hipMemcpyAsync(d_array, src, a.n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_cluster_check(a, d_array, ctx->stream));
    uint32_t error = 0;
    HIP_TRY(hipMemcpyAsync(&error, a.error, sizeof error, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (error) return fail(SKL_ERR_INVALID_ARG, "%s: a label exceeds its own index (labels[i] <= i is required of an input partition)", what);
    return SKL_OK;
}

// FLATTEN, COUNT, and the one read every call ends on: the stream is idle and the labels are in place on return
int cluster_finish(skl_ctx *ctx, const ClusterArgs &a, uint32_t *labels, bool on_device, uint64_t *n_clusters)
{
    HIP_TRY(launch_cluster_flatten(a, ctx->stream));
    HIP_TRY(launch_cluster_count(a, ctx->stream));
    unsigned long long count = 0;
    HIP_TRY(hipMemcpyAsync(&count, a.count, sizeof count, hipMemcpyDeviceToHost, ctx->stream));
    if (!on_device) HIP_TRY(hipMemcpyAsync(labels, a.labels, a.n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_clusters = count;
    return SKL_OK;
}

}  // namespace

extern "C" int skl_self_clusters_within(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t row_begin, size_t row_end,
                                        double max_first, double max_second, uint32_t *labels, int labels_on_device, int flags,
                                        uint64_t *n_clusters)
{
    const RoctxRange range_("skl:clusters within");
    if (!n_clusters) return fail(SKL_ERR_INVALID_ARG, "n_clusters is null");
    *n_clusters = 0;
    if (!labels) return fail(SKL_ERR_INVALID_ARG, "labels is null");
    if (flags & ~SKL_CLUSTERS_CONTINUE) return fail(SKL_ERR_INVALID_ARG, "unknown flags %d", flags);
    SKL_TRY(check_params(s, s, p));
    const bool coreacc = p->dist_type == SKL_DIST_COREACC;
    const uint32_t ncols = coreacc ? 2u : 1u;
    const int mode = coreacc ? MODE_COREACC : MODE_JACCARD;
    const int jout = coreacc ? 0 : (p->ani ? JOUT_ANI : JOUT_DIST);
    WithinPred pred;
    if (!within_pred_make(max_first, max_second, !coreacc && p->ani, ncols, &pred)) {
        return fail(SKL_ERR_INVALID_ARG, "max_first = %g, max_second = %g: a cap is a distance (not NaN; max_first >= 0)", max_first, max_second);
    }
    SKL_TRY(ctx_bind(ctx));
    // (the row range as the within calls read it)
    const uint64_t n = s->n;
    uint64_t r0 = row_begin, r1 = row_end;
    if (r0 > r1 || r1 > n) return fail(SKL_ERR_INVALID_ARG, "row range [%llu, %llu) out of bounds", (unsigned long long)r0, (unsigned long long)r1);
    r1 = std::min<uint64_t>(r1, n ? n - 1 : 0);
    if (n == 0) return SKL_OK;
    if (n > CLUSTER_MAX_SAMPLES) return fail(SKL_ERR_INVALID_ARG, "%llu samples: labels are u32", (unsigned long long)n);

    const bool on_device = labels_on_device != 0;
    ClusterBuffers buf;
    SKL_TRY(cluster_buffers(ctx, labels, nullptr, n, on_device, &buf));
    ClusterArgs a = {};
    a.labels = buf.d_labels;
    a.n = n;
    a.ncols = ncols;
    a.pred = pred;
    a.error = buf.error;
    a.count = buf.count;
    if (flags & SKL_CLUSTERS_CONTINUE) SKL_TRY(cluster_checked(ctx, a, labels, buf.d_labels, on_device, "labels"));
    else HIP_TRY(launch_cluster_init(a, ctx->stream));

    // (an empty row range or a single sample: no band, and the labels are still finished and counted)
    HostBands plan;
    if (r1 > r0) {
        const size_t rec = ncols * sizeof(float);
        const size_t budget = ctx->knobs.pairs_band > 0 ? (size_t)ctx->knobs.pairs_band * rec : BAND_BYTES;
        plan = plan_host_bands(true, n, r0, r1, rec, budget);
    }
    uint64_t widest = 0;
    for (const HostBand &b : plan.bands) widest = std::max(widest, b.pairs);
    if (!within_band_ok(widest)) return fail(SKL_ERR_INVALID_ARG, "a band of %llu pairs (2^32 or more)", (unsigned long long)widest);
    void *band = nullptr;
    if (widest) SKL_TRY(ctx_scratch(ctx, within_band_bytes(widest, ncols), &band, SCRATCH_KEY_BAND));
    a.band = (const float *)band;

    std::string dense_name;
    for (const HostBand &b : plan.bands) {
        SKL_TRY(dense_band(ctx, s, s, p, mode, jout, 1, b.r0, b.r1, band));
        if (dense_name.empty()) dense_name = ctx->last_kernel;
        a.m = b.pairs;
        a.chunks = within_chunks(b.pairs);
        a.first = cond_index(b.r0, b.r0 + 1, n);
        HIP_TRY(launch_cluster_union(a, ctx->stream));
    }
    SKL_TRY(cluster_finish(ctx, a, labels, on_device, n_clusters));
    ctx->last_kernel = (plan.bands.empty() ? std::string() : dense_name + " + skl::cluster_union_kernel, ") +
                       "skl::cluster_flatten_kernel, skl::cluster_count_kernel (clusters within the cap, chunks of " + std::to_string(WITHIN_CHUNK) +
                       " positions" + (plan.bands.size() > 1 ? "; " + std::to_string(plan.bands.size()) + " bands" : "") + ")";
    return SKL_OK;
}

extern "C" int skl_clusters_merge(skl_ctx *ctx, uint32_t *labels, const uint32_t *other, uint64_t n, int on_device, uint64_t *n_clusters)
{
    const RoctxRange range_("skl:clusters merge");
    if (!n_clusters) return fail(SKL_ERR_INVALID_ARG, "n_clusters is null");
    *n_clusters = 0;
    if (n == 0) return ctx ? SKL_OK : fail(SKL_ERR_INVALID_ARG, "null context");
    if (!labels || !other) return fail(SKL_ERR_INVALID_ARG, "a label array is null");
    if (n > CLUSTER_MAX_SAMPLES) return fail(SKL_ERR_INVALID_ARG, "%llu samples: labels are u32", (unsigned long long)n);
    SKL_TRY(ctx_bind(ctx));
    ClusterBuffers buf;
    SKL_TRY(cluster_buffers(ctx, labels, other, n, on_device != 0, &buf));
    ClusterArgs a = {};
    a.labels = buf.d_labels;
    a.other = buf.d_other;
    a.n = n;
    a.error = buf.error;
    a.count = buf.count;
    SKL_TRY(cluster_checked(ctx, a, labels, buf.d_labels, on_device != 0, "labels"));
    SKL_TRY(cluster_checked(ctx, a, other, buf.d_other, on_device != 0, "other"));
    HIP_TRY(launch_cluster_merge(a, ctx->stream));
    SKL_TRY(cluster_finish(ctx, a, labels, on_device != 0, n_clusters));
    ctx->last_kernel = "skl::cluster_merge_kernel, skl::cluster_flatten_kernel, skl::cluster_count_kernel";
    return SKL_OK;
}
