// capi_pairs.cpp -- skl_self_dists_pairs / skl_cross_dists_pairs: the distances of an explicit list of sample pairs
// (pair_list.hip).  The list is validated whole before anything is launched, then uploaded and processed in bands; the work
// items (runs of consecutive entries with the same first sample, cut at 64 and at the band's end) are made on the host.
#include "capi_internal.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace skl;

namespace {
constexpr uint64_t PAIRS_BAND_DEFAULT = 64ull << 20;   // listed pairs per band (SKL_PAIRS_BAND)
constexpr uint64_t PAIRS_BAND_MAX = 1ull << 31;        // entry positions of a band are u32
constexpr uint64_t COUNTS_BYTES_MAX = 1ull << 30;      // counts parked in memory (more than MAX_FUSED_K lengths) per band

int pairs_call(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, const skl_dist_params *p, const char *a_side,
               const char *b_side, const uint32_t *pair_a, const uint32_t *pair_b, size_t n_pairs, float *out, int out_on_device)
{
    const RoctxRange range_("skl:pair list");
    SKL_TRY(check_params(rows, cols, p));
    SKL_TRY(ctx_bind(ctx));
    if (n_pairs == 0) return SKL_OK;
    if (!pair_a || !pair_b || !out) return fail(SKL_ERR_INVALID_ARG, "null argument");
    for (size_t x = 0; x < n_pairs; ++x) {
        if (pair_a[x] >= rows->n) {
            return fail(SKL_ERR_INVALID_ARG, "pair %zu: %s index %u out of range (%zu samples)", x, a_side, pair_a[x], rows->n);
        }
        if (pair_b[x] >= cols->n) {
            return fail(SKL_ERR_INVALID_ARG, "pair %zu: %s index %u out of range (%zu samples)", x, b_side, pair_b[x], cols->n);
        }
    }
    const bool coreacc = p->dist_type == SKL_DIST_COREACC;
    PairArgs g;
    SKL_TRY(fill_args_ref_layout(rows, cols, p, coreacc ? MODE_COREACC : MODE_JACCARD, coreacc ? 0 : (p->ani ? JOUT_ANI : JOUT_DIST), &g));
    g.xcd_shift = ctx_xcd_shift(ctx);
    const bool counts_out = g.k_count > (uint32_t)MAX_FUSED_K;
    uint64_t band = ctx->knobs.pairs_band > 0 ? (uint64_t)ctx->knobs.pairs_band : PAIRS_BAND_DEFAULT;
    band = std::min(band, PAIRS_BAND_MAX);
    if (counts_out) band = std::min(band, std::max<uint64_t>(1, COUNTS_BYTES_MAX / (g.k_count * sizeof(uint32_t))));
    band = std::min<uint64_t>(band, n_pairs);
    const size_t rec = coreacc ? 2 * sizeof(float) : sizeof(float);

    DevBuf d_a, d_b, d_ws, d_out, d_counts;
    HIP_TRY(hipMalloc(&d_a.p, band * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&d_b.p, band * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&d_ws.p, (band + 1) * sizeof(uint32_t)));
    if (!out_on_device) HIP_TRY(hipMalloc(&d_out.p, band * rec));
    if (counts_out) HIP_TRY(hipMalloc(&d_counts.p, band * g.k_count * sizeof(uint32_t)));

    PairListArgs c;
    memset(&c, 0, sizeof c);
    c.pair_a = (const uint32_t *)d_a.p;
    c.pair_b = (const uint32_t *)d_b.p;
    c.work_start = (const uint32_t *)d_ws.p;
    c.b_rows = cols->d_rows;
    c.coreacc = coreacc ? 1u : 0u;
    c.counts = (uint32_t *)d_counts.p;
    c.kf = rows->d_kf;
    ctx->last_kernel = pair_list_kernel_name(g);

    std::vector<uint32_t> ws;
    for (uint64_t b0 = 0; b0 < n_pairs; b0 += band) {
        const uint64_t m = std::min<uint64_t>(band, n_pairs - b0);
        const uint32_t *a = pair_a + b0;
        ws.clear();
        for (uint64_t x = 0; x < m;) {   // a run of equal `a`, cut at 64 entries (and by the band's end)
            ws.push_back((uint32_t)x);
            uint64_t e = x + 1;
            while (e < m && e - x < (uint64_t)LANES && a[e] == a[x]) ++e;
            x = e;
        }
        c.n_work = ws.size();
        ws.push_back((uint32_t)m);
        c.n_entries = m;
        c.out = out_on_device ? (void *)((char *)out + b0 * rec) : d_out.p;
        HIP_TRY(hipMemcpyAsync(d_a.p, a, m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_b.p, pair_b + b0, m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d_ws.p, ws.data(), ws.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        std::pair<hipEvent_t, hipEvent_t> *ev = timing_slot(ctx);   // (bracketed like the pair kernels: skl_ctx_kernel_ms)
        if (ev) HIP_TRY(hipEventRecord(ev->first, ctx->stream));
        HIP_TRY(launch_pair_list(c, g, ctx->stream));
        if (ev) HIP_TRY(hipEventRecord(ev->second, ctx->stream));
        if (!out_on_device) HIP_TRY(hipMemcpyAsync((char *)out + b0 * rec, d_out.p, m * rec, hipMemcpyDeviceToHost, ctx->stream));
        // the band's buffers (and the host's work-item array) are reused by the next band and freed on return
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return SKL_OK;
}
}  // namespace

extern "C" int skl_self_dists_pairs(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, const uint32_t *pair_a,
                                    const uint32_t *pair_b, size_t n_pairs, float *out, int out_on_device)
{
    return pairs_call(ctx, s, s, p, "first sample", "second sample", pair_a, pair_b, n_pairs, out, out_on_device);
}

extern "C" int skl_cross_dists_pairs(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query, const skl_dist_params *p,
                                     const uint32_t *pair_ref, const uint32_t *pair_query, size_t n_pairs, float *out,
                                     int out_on_device)
{
    return pairs_call(ctx, ref, query, p, "reference", "query", pair_ref, pair_query, n_pairs, out, out_on_device);
}
