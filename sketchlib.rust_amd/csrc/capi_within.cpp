// capi_within.cpp -- skl_self_dists_within / skl_cross_dists_within: the pairs of a dense call that lie within a distance cap,
// compacted on the device (within.hip; the numbers, the predicate and the locator: within_plan.hpp).  The row range is cut into
// the bands of a host-destined dense call (dense_plan.hpp plan_host_bands, under the same budget); each band is evaluated by
// dense_band() into scratch exactly as that call would, then counted, scanned and scattered behind it on the context's stream.
// The running total lives in device memory, so the bands of a device-destined call chain without a trip to the host; a
// host-destined call reads it after every band, because it has the band's records to copy anyway.
#include "capi_internal.hpp"

#include <algorithm>
#include <string>

using namespace skl;

namespace {

int within_call(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, const skl_dist_params *p, int self_mode, uint64_t r0,
                uint64_t r1, double max_first, double max_second, uint32_t *out_i, uint32_t *out_j, float *out_d, uint64_t capacity,
                int out_on_device, uint64_t *n_found)
{
    const RoctxRange range_("skl:dists within");
    if (!n_found) return fail(SKL_ERR_INVALID_ARG, "n_found is null");
    *n_found = 0;
    SKL_TRY(check_params(rows, cols, p));
    const bool coreacc = p->dist_type == SKL_DIST_COREACC;
    const uint32_t ncols = coreacc ? 2u : 1u;
    const int mode = coreacc ? MODE_COREACC : MODE_JACCARD;
    const int jout = coreacc ? 0 : (p->ani ? JOUT_ANI : JOUT_DIST);
    WithinPred pred;
    if (!within_pred_make(max_first, max_second, !coreacc && p->ani, ncols, &pred)) {
        return fail(SKL_ERR_INVALID_ARG, "max_first = %g, max_second = %g: a cap is a distance (not NaN; max_first >= 0)", max_first, max_second);
    }
    if (capacity && (!out_i || !out_j || !out_d)) return fail(SKL_ERR_INVALID_ARG, "capacity %llu with a null output", (unsigned long long)capacity);
    SKL_TRY(ctx_bind(ctx));
    // (the row range as dense_rows() reads it)
    const uint64_t n_cols = cols->n;
    const uint64_t row_limit = self_mode ? (n_cols ? n_cols - 1 : 0) : rows->n;
    if (r0 > r1 || r1 > (self_mode ? n_cols : rows->n)) {
        return fail(SKL_ERR_INVALID_ARG, "row range [%llu, %llu) out of bounds", (unsigned long long)r0, (unsigned long long)r1);
    }
    r1 = std::min<uint64_t>(r1, row_limit);
    if (r1 <= r0 || n_cols == 0) return SKL_OK;

    const size_t rec = ncols * sizeof(float);
    // (SKL_PAIRS_BAND, the pair-list calls' pairs per band, cuts these bands too: tests force several on small inputs)
    const size_t budget = ctx->knobs.pairs_band > 0 ? (size_t)ctx->knobs.pairs_band * rec : BAND_BYTES;
    const HostBands plan = plan_host_bands(self_mode != 0, n_cols, r0, r1, rec, budget);
    uint64_t widest = 0;
    for (const HostBand &b : plan.bands) widest = std::max(widest, b.pairs);
    if (!within_band_ok(widest)) return fail(SKL_ERR_INVALID_ARG, "a band of %llu pairs (2^32 or more)", (unsigned long long)widest);
    void *band = nullptr, *ws = nullptr;
    SKL_TRY(ctx_scratch(ctx, within_band_bytes(widest, ncols), &band, SCRATCH_KEY_BAND));
    SKL_TRY(ctx_scratch(ctx, within_scratch_bytes(within_chunks(widest)), &ws, SCRATCH_WITHIN));

    WithinArgs a = {};
    a.band = (const float *)band;
    a.ncols = ncols;
    a.self_mode = self_mode ? 1u : 0u;
    a.n_cols = n_cols;
    a.pred = pred;
    a.total = (uint64_t *)ws;
    a.offsets = (uint64_t *)((char *)ws + within_scratch_offsets_at());
    a.capacity = capacity;
    HIP_TRY(hipMemsetAsync(a.total, 0, WITHIN_SCRATCH_TOTAL_BYTES, ctx->stream));

    std::string dense_name;
    uint64_t total = 0;   // (host-destined calls: as of the last band read back)
    for (const HostBand &b : plan.bands) {
        SKL_TRY(dense_band(ctx, rows, cols, p, mode, jout, self_mode, b.r0, b.r1, band));
        if (dense_name.empty()) dense_name = ctx->last_kernel;
        a.m = b.pairs;
        a.chunks = within_chunks(b.pairs);
        a.counts = (uint32_t *)((char *)ws + within_scratch_counts_at(a.chunks));
        a.first = self_mode ? cond_index(b.r0, b.r0 + 1, n_cols) : b.r0 * n_cols;
        HIP_TRY(launch_within_count(a, ctx->stream));
        HIP_TRY(launch_within_scan(a, ctx->stream));
        if (capacity == 0) continue;   // count only: no scatter pass
        if (out_on_device) {
            a.out_i = out_i;
            a.out_j = out_j;
            a.out_d = out_d;
            a.rebase = 0;
            HIP_TRY(launch_within_scatter(a, ctx->stream));
            continue;
        }
        // host outputs: this band's records through a staging buffer of exactly their number
        const uint64_t before = total;
        HIP_TRY(hipMemcpyAsync(&total, a.total, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        const uint64_t take = std::min<uint64_t>(total - before, capacity > before ? capacity - before : 0);
        if (take == 0) continue;
        void *stage = nullptr;
        SKL_TRY(ctx_scratch(ctx, take * (rec + 2 * sizeof(uint32_t)), &stage, SCRATCH_KNN_STAGING));
        a.out_d = (float *)stage;
        a.out_i = (uint32_t *)((char *)stage + take * rec);
        a.out_j = a.out_i + take;
        a.rebase = before;
        HIP_TRY(launch_within_scatter(a, ctx->stream));
        HIP_TRY(hipMemcpyAsync(out_d + before * ncols, a.out_d, take * rec, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(out_i + before, a.out_i, take * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(out_j + before, a.out_j, take * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));   // (the next band scatters into the same buffer)
    }
    // the one read every call ends on: the stream is idle, and a device-destined call's records are in place, on return
    HIP_TRY(hipMemcpyAsync(&total, a.total, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_found = total;
    ctx->last_kernel = dense_name + " + skl::within_count_kernel, skl::within_scan_kernel" +
                       (capacity ? ", skl::within_scatter_kernel" : " (count only)") + " (pairs within the cap, chunks of " +
                       std::to_string(WITHIN_CHUNK) + " positions" + (plan.bands.size() > 1 ? "; " + std::to_string(plan.bands.size()) + " bands" : "") + ")";
    return SKL_OK;
}

}  // namespace

extern "C" int skl_self_dists_within(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t row_begin, size_t row_end,
                                     double max_first, double max_second, uint32_t *out_i, uint32_t *out_j, float *out_d, uint64_t capacity,
                                     int out_on_device, uint64_t *n_found)
{
    return within_call(ctx, s, s, p, 1, row_begin, row_end, max_first, max_second, out_i, out_j, out_d, capacity, out_on_device, n_found);
}

extern "C" int skl_cross_dists_within(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query, const skl_dist_params *p,
                                      size_t ref_begin, size_t ref_end, double max_first, double max_second, uint32_t *out_i,
                                      uint32_t *out_j, float *out_d, uint64_t capacity, int out_on_device, uint64_t *n_found)
{
    return within_call(ctx, ref, query, p, 0, ref_begin, ref_end, max_first, max_second, out_i, out_j, out_d, capacity, out_on_device, n_found);
}
