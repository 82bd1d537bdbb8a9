// capi_hist.cpp -- skl_self_dists_hist / skl_cross_dists_hist: the histogram of the values a dense call stores, on a grid the
// caller gives (hist.hip; the grid, the cell rule and the launch numbers: hist_plan.hpp).  The driver is capi_within.cpp's: the row
// range is cut into the bands of a host-destined dense call (dense_plan.hpp plan_host_bands, under the same budget or
// SKL_PAIRS_BAND), each band is evaluated by dense_band() into scratch exactly as that call would, and the histogram launch
// follows it on the context's stream.  The counts and the two outside words stay in device memory from the first band to the
// last: nothing goes to the host between bands.  A caller's host array is served from SCRATCH_HIST and copied back once.
#include "capi_internal.hpp"

#include <algorithm>
#include <string>
#include <vector>

using namespace skl;

namespace {

int hist_call(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, const skl_dist_params *p, int self_mode, uint64_t r0,
              uint64_t r1, const skl_hist_grid *grid, uint64_t *counts, int counts_on_device, int flags, uint64_t *outside)
{
    const RoctxRange range_("skl:dists hist");
    // (every refusal comes before the first write to counts or outside)
    if (!grid || !counts || !outside) return fail(SKL_ERR_INVALID_ARG, "grid, counts or outside is null");
    if (flags & ~SKL_HIST_ACCUMULATE) return fail(SKL_ERR_INVALID_ARG, "unknown flags %d", flags);
    SKL_TRY(check_params(rows, cols, p));
    const bool coreacc = p->dist_type == SKL_DIST_COREACC;
    const uint32_t ncols = coreacc ? 2u : 1u;
    const int mode = coreacc ? MODE_COREACC : MODE_JACCARD;
    const int jout = coreacc ? 0 : (p->ani ? JOUT_ANI : JOUT_DIST);
    HistGrid g;
    if (!hist_grid_make(grid->lo0, grid->hi0, grid->n0, grid->lo1, grid->hi1, grid->n1, ncols, &g)) {
        return fail(SKL_ERR_INVALID_ARG,
                    "grid [%g, %g] / %u x [%g, %g] / %u: bounds are finite with hi > lo as floats, cell counts are not 0, and at most %u cells",
                    grid->lo0, grid->hi0, grid->n0, grid->lo1, grid->hi1, grid->n1, HIST_MAX_CELLS);
    }
    SKL_TRY(ctx_bind(ctx));
    // (the row range as dense_rows() reads it)
    const uint64_t n_cols = cols->n;
    const uint64_t row_limit = self_mode ? (n_cols ? n_cols - 1 : 0) : rows->n;
    if (r0 > r1 || r1 > (self_mode ? n_cols : rows->n)) {
        return fail(SKL_ERR_INVALID_ARG, "row range [%llu, %llu) out of bounds", (unsigned long long)r0, (unsigned long long)r1);
    }
    r1 = std::min<uint64_t>(r1, row_limit);
    // (an empty row range, or no column: no band, and the outputs are still zeroed or kept)
    HostBands plan;
    const size_t rec = ncols * sizeof(float);
    if (r1 > r0 && n_cols) {
        const size_t budget = ctx->knobs.pairs_band > 0 ? (size_t)ctx->knobs.pairs_band * rec : BAND_BYTES;
        plan = plan_host_bands(self_mode != 0, n_cols, r0, r1, rec, budget);
    }
    uint64_t widest = 0;
    for (const HostBand &b : plan.bands) widest = std::max(widest, b.pairs);
    if (!within_band_ok(widest)) return fail(SKL_ERR_INVALID_ARG, "a band of %llu pairs (2^32 or more)", (unsigned long long)widest);

    const uint64_t cells = hist_cells(g);
    const bool on_device = counts_on_device != 0, accumulate = (flags & SKL_HIST_ACCUMULATE) != 0;
    void *band = nullptr, *ws = nullptr;
    if (widest) SKL_TRY(ctx_scratch(ctx, within_band_bytes(widest, ncols), &band, SCRATCH_KEY_BAND));
    SKL_TRY(ctx_scratch(ctx, hist_scratch_bytes(on_device ? 0 : cells), &ws, SCRATCH_HIST));
    HistArgs a = {};
    a.band = (const float *)band;
    a.grid = g;
    a.outside = (unsigned long long *)ws;
    a.counts = on_device ? (unsigned long long *)counts : (unsigned long long *)((char *)ws + HIST_SCRATCH_HEAD_BYTES);
    // the scratch words and staged counts start at 0 and are added to the caller's at the end; a device array is the accumulator itself
    HIP_TRY(hipMemsetAsync(ws, 0, hist_scratch_bytes(on_device ? 0 : cells), ctx->stream));
    if (on_device && !accumulate) HIP_TRY(hipMemsetAsync(counts, 0, cells * sizeof(uint64_t), ctx->stream));

    std::string dense_name;
    for (const HostBand &b : plan.bands) {
        SKL_TRY(dense_band(ctx, rows, cols, p, mode, jout, self_mode, b.r0, b.r1, band));
        if (dense_name.empty()) dense_name = ctx->last_kernel;
        a.m = b.pairs;
        a.chunks = hist_chunks(b.pairs);
        HIP_TRY(launch_hist(a, ctx->stream));
    }
    // the one read every call ends on: the stream is idle and the counts are in place on return
    unsigned long long out2[2] = {0, 0};
    std::vector<uint64_t> staged;
    HIP_TRY(hipMemcpyAsync(out2, a.outside, sizeof out2, hipMemcpyDeviceToHost, ctx->stream));
    if (!on_device) {
        uint64_t *dst = counts;
        if (accumulate) {
            staged.resize(cells);
            dst = staged.data();
        }
        HIP_TRY(hipMemcpyAsync(dst, a.counts, cells * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (uint64_t x = 0; x < staged.size(); ++x) counts[x] += staged[x];
    outside[0] = (accumulate ? outside[0] : 0u) + out2[0];
    outside[1] = (accumulate ? outside[1] : 0u) + out2[1];
    ctx->last_kernel = plan.bands.empty()
                           ? std::string()
                           : dense_name + " + " + (hist_in_lds(cells) ? "skl::hist_lds_kernel" : "skl::hist_global_kernel") + " (histogram of the stored values, " +
                                 std::to_string(g.n0) + " x " + std::to_string(g.n1) + " cells, chunks of " + std::to_string(HIST_CHUNK) + " positions" +
                                 (plan.bands.size() > 1 ? "; " + std::to_string(plan.bands.size()) + " bands" : "") + ")";
    return SKL_OK;
}

}  // namespace

extern "C" int skl_self_dists_hist(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t row_begin, size_t row_end,
                                   const skl_hist_grid *grid, uint64_t *counts, int counts_on_device, int flags, uint64_t *outside)
{
    return hist_call(ctx, s, s, p, 1, row_begin, row_end, grid, counts, counts_on_device, flags, outside);
}

extern "C" int skl_cross_dists_hist(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query, const skl_dist_params *p,
                                    size_t ref_begin, size_t ref_end, const skl_hist_grid *grid, uint64_t *counts, int counts_on_device,
                                    int flags, uint64_t *outside)
{
    return hist_call(ctx, ref, query, p, 0, ref_begin, ref_end, grid, counts, counts_on_device, flags, outside);
}
