// capi_inv.cpp -- the entry points of include/sketchlib_dist.h for `inverted query`: a device-resident
// index of u16 index sketches (skl_inverted), the query against it (src/inverted.rs:229-269) and its best hits
// (src/lib.rs:1019-1109).  Kernels: inv_query.hip, inv_top.hip.
#include "capi_internal.hpp"

#include <algorithm>
#include <cstring>

using namespace skl;

struct skl_inverted {
    int device = 0;
    size_t n = 0, sketch_size = 0, words = 0;
    uint32_t *d_planes = nullptr;   // [words * 16][n] (inv_query.hip)
};

namespace {

constexpr size_t UPLOAD_BYTES = 256ull << 20;   // raw u16 bins staged per relayout pass
constexpr size_t DEFAULT_BAND_BYTES = 1ull << 30;   // device memory per query band (outputs + query planes)

uint32_t tail_mask(size_t sketch_size)
{
    const uint32_t rem = (uint32_t)(sketch_size % 32);
    return rem ? (1u << rem) - 1u : 0xFFFFFFFFu;
}

// rows x sketch_size u16 bins from the host -> planes, `chunk` rows per staged upload
int upload_planes(skl_ctx *ctx, const uint16_t *bins, size_t rows, size_t sketch_size, size_t words,
                  uint64_t stride_row, uint64_t stride_word, uint64_t stride_plane, uint32_t *planes)
{
    const size_t chunk = std::max<size_t>(1, std::min(rows, UPLOAD_BYTES / (sketch_size * sizeof(uint16_t))));
    DevBuf d_raw;
    HIP_TRY(hipMalloc(&d_raw.p, chunk * sketch_size * sizeof(uint16_t)));
    for (size_t r0 = 0; r0 < rows; r0 += chunk) {
        const size_t nr = std::min(chunk, rows - r0);
        HIP_TRY(hipMemcpyAsync(d_raw.p, bins + r0 * sketch_size, nr * sketch_size * sizeof(uint16_t),
                               hipMemcpyHostToDevice, ctx->stream));
        InvPlanesArgs a;
        a.bins = (const uint16_t *)d_raw.p;
        a.rows = (uint32_t)nr;
        a.sketch_size = (uint32_t)sketch_size;
        a.words = (uint32_t)words;
        a.row0 = r0;
        a.stride_row = stride_row;
        a.stride_word = stride_word;
        a.stride_plane = stride_plane;
        a.planes = planes;
        HIP_TRY(launch_inv_planes(a, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));   // the staging buffer is reused (and freed) next
    }
    return SKL_OK;
}

}  // namespace

extern "C" int skl_inverted_create(skl_ctx *ctx, const uint16_t *bins, size_t n_samples, size_t sketch_size,
                                   skl_inverted **out)
{
    const RoctxRange range_("skl:inverted create");
    if (!out) return fail(SKL_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    SKL_TRY(ctx_bind(ctx));
    if (!bins && n_samples) return fail(SKL_ERR_INVALID_ARG, "null argument");
    if (sketch_size == 0 || sketch_size > 0xFFFFFFFFull) return fail(SKL_ERR_INVALID_ARG, "sketch_size %zu out of range", sketch_size);
    if (n_samples > 0xFFFFFFFFull - 256) return fail(SKL_ERR_INVALID_ARG, "%zu samples: at most 2^32 - 257 per index", n_samples);
    skl_inverted *ix = new skl_inverted;
    ix->device = ctx->device;
    ix->n = n_samples;
    ix->sketch_size = sketch_size;
    ix->words = (sketch_size + 31) / 32;
    if (n_samples) {
        const hipError_t e = hipMalloc(&ix->d_planes, ix->words * 16 * n_samples * sizeof(uint32_t));
        if (e != hipSuccess) {
            delete ix;
            return fail(e == hipErrorOutOfMemory ? SKL_ERR_OOM : SKL_ERR_HIP, "hipMalloc of %zu index planes: %s",
                        ix->words * 16 * n_samples, hipGetErrorString(e));
        }
        const int rc = upload_planes(ctx, bins, n_samples, sketch_size, ix->words, 1, 16ull * n_samples, n_samples,
                                     ix->d_planes);
        if (rc != SKL_OK) {
            (void)hipFree(ix->d_planes);
            delete ix;
            return rc;
        }
    }
    *out = ix;
    return SKL_OK;
}

extern "C" int skl_inverted_destroy(skl_inverted *ix)
{
    if (!ix) return SKL_OK;
    if (ix->d_planes) {
        (void)hipSetDevice(ix->device);
        (void)hipFree(ix->d_planes);
    }
    delete ix;
    return SKL_OK;
}

extern "C" size_t skl_inverted_band_queries(skl_ctx *ctx, const skl_inverted *ix, int mode)
{
    if (!ctx || !ix) return 0;
    const size_t budget = ctx->knobs.invq_band_bytes > 0 ? (size_t)ctx->knobs.invq_band_bytes : DEFAULT_BAND_BYTES;
    const size_t out_row = mode == SKL_INVQ_MATCH_COUNT ? ix->n * sizeof(uint32_t) : (ix->n + 63) / 64 * sizeof(uint64_t);
    const size_t per_query = out_row + ix->sketch_size * sizeof(uint16_t) + ix->words * 64;
    size_t band = std::max<size_t>(1, budget / per_query);
    if (band >= (size_t)IQ_QTILE) band -= band % IQ_QTILE;                 // whole tiles where the budget allows
    const size_t s_blocks = std::max<size_t>(1, (ix->n + 255) / 256);
    const size_t max_tiles = std::max<size_t>(1, IQ_MAX_BLOCKS / s_blocks);   // one launch's grid
    return std::min(band, max_tiles * IQ_QTAIL);
}

extern "C" int skl_inverted_query(skl_ctx *ctx, const skl_inverted *ix, const uint16_t *query_bins, size_t n_queries,
                                  int mode, void *out)
{
    const RoctxRange range_("skl:inverted query");
    SKL_TRY(ctx_bind(ctx));
    if (!ix) return fail(SKL_ERR_INVALID_ARG, "null index");
    if (mode != SKL_INVQ_MATCH_COUNT && mode != SKL_INVQ_ANY_BINS && mode != SKL_INVQ_ALL_BINS) {
        return fail(SKL_ERR_INVALID_ARG, "unknown query mode %d", mode);
    }
    if (ix->device != ctx->device) return fail(SKL_ERR_INVALID_ARG, "index and context are on different devices");
    if (n_queries == 0 || ix->n == 0) return SKL_OK;
    if (!query_bins || !out) return fail(SKL_ERR_INVALID_ARG, "null argument");
    const size_t n = ix->n, S = ix->sketch_size, W = ix->words;
    const size_t n_words64 = (n + 63) / 64;
    const size_t out_row = mode == SKL_INVQ_MATCH_COUNT ? n * sizeof(uint32_t) : n_words64 * sizeof(uint64_t);
    const size_t band = std::min(n_queries, skl_inverted_band_queries(ctx, ix, mode));
    const size_t band_pad = (band + IQ_QTILE - 1) / IQ_QTILE * IQ_QTILE;
    DevBuf d_qplanes, d_out;
    HIP_TRY(hipMalloc(&d_qplanes.p, W * band_pad * 16 * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&d_out.p, band * out_row));
    for (size_t q0 = 0; q0 < n_queries; q0 += band) {
        const size_t nq = std::min(band, n_queries - q0);
        const size_t nq_pad = (nq + IQ_QTILE - 1) / IQ_QTILE * IQ_QTILE;
        HIP_TRY(hipMemsetAsync(d_qplanes.p, 0, W * nq_pad * 16 * sizeof(uint32_t), ctx->stream));
        SKL_TRY(upload_planes(ctx, query_bins + q0 * S, nq, S, W, 16, 16ull * nq_pad, 1, (uint32_t *)d_qplanes.p));
        InvQueryArgs a;
        memset(&a, 0, sizeof a);
        a.ref_planes = ix->d_planes;
        a.q_planes = (const uint32_t *)d_qplanes.p;
        a.n = (uint32_t)n;
        a.nq = (uint32_t)nq;
        a.nq_pad = (uint32_t)nq_pad;
        a.words = (uint32_t)W;
        a.sketch_size = (uint32_t)S;
        a.tail_mask = tail_mask(S);
        a.mode = mode == SKL_INVQ_MATCH_COUNT ? INVQ_COUNTS : mode == SKL_INVQ_ANY_BINS ? INVQ_ANY : INVQ_ALL;
        a.counts = (uint32_t *)d_out.p;
        a.bits = (uint64_t *)d_out.p;
        a.n_words64 = n_words64;
        HIP_TRY(launch_inv_query(a, ctx->stream));
        HIP_TRY(hipMemcpyAsync((char *)out + q0 * out_row, d_out.p, nq * out_row, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return SKL_OK;
}

// The best hits of every query: the counts band of match-count mode stays on the device, inv_top.hip selects behind it on
// the same stream, and top ids + top counts per query come back.
extern "C" int skl_inverted_query_top(skl_ctx *ctx, const skl_inverted *ix, const uint16_t *query_bins, size_t n_queries,
                                      size_t top, uint32_t *out_ids, uint32_t *out_counts)
{
    const RoctxRange range_("skl:inverted query top");
    SKL_TRY(ctx_bind(ctx));
    if (!ix) return fail(SKL_ERR_INVALID_ARG, "null index");
    if (top == 0 || top > SKL_INVQ_TOP_MAX) {
        return fail(SKL_ERR_INVALID_ARG, "top = %zu: 1 to %d hits per query (SKL_INVQ_TOP_MAX)", top, SKL_INVQ_TOP_MAX);
    }
    static_assert(SKL_INVQ_TOP_MAX == INV_TOP_MAX, "the public limit is the plan's");
    if (ix->device != ctx->device) return fail(SKL_ERR_INVALID_ARG, "index and context are on different devices");
    if (n_queries == 0) return SKL_OK;
    if (!query_bins || !out_ids || !out_counts) return fail(SKL_ERR_INVALID_ARG, "null argument");
    const size_t n = ix->n, S = ix->sketch_size, W = ix->words;
    if (n == 0) {
        std::fill(out_ids, out_ids + n_queries * top, INV_TOP_PAD_ID);
        std::fill(out_counts, out_counts + n_queries * top, 0u);
        return SKL_OK;
    }
    const size_t band = std::min(n_queries, skl_inverted_band_queries(ctx, ix, SKL_INVQ_MATCH_COUNT));
    const size_t band_pad = (band + IQ_QTILE - 1) / IQ_QTILE * IQ_QTILE;
    DevBuf d_qplanes, d_counts, d_hits;
    HIP_TRY(hipMalloc(&d_qplanes.p, W * band_pad * 16 * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&d_counts.p, band * n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&d_hits.p, 2 * band * top * sizeof(uint32_t)));   // the band's ids, then its counts
    InvTopArgs t;
    memset(&t, 0, sizeof t);
    t.counts = (const uint32_t *)d_counts.p;
    t.n = (uint32_t)n;
    t.top = (uint32_t)top;
    t.n_eff = inv_top_n_eff(t.top, t.n);
    t.digit_bits = inv_top_digit_bits(ctx->knobs.invq_top_digit_bits);
    t.digits = inv_top_digits((uint32_t)S, t.digit_bits);
    t.list_len = inv_top_list_len(t.n_eff);
    for (size_t q0 = 0; q0 < n_queries; q0 += band) {
        const size_t nq = std::min(band, n_queries - q0);
        const size_t nq_pad = (nq + IQ_QTILE - 1) / IQ_QTILE * IQ_QTILE;
        HIP_TRY(hipMemsetAsync(d_qplanes.p, 0, W * nq_pad * 16 * sizeof(uint32_t), ctx->stream));
        SKL_TRY(upload_planes(ctx, query_bins + q0 * S, nq, S, W, 16, 16ull * nq_pad, 1, (uint32_t *)d_qplanes.p));
        InvQueryArgs a;
        memset(&a, 0, sizeof a);
        a.ref_planes = ix->d_planes;
        a.q_planes = (const uint32_t *)d_qplanes.p;
        a.n = (uint32_t)n;
        a.nq = (uint32_t)nq;
        a.nq_pad = (uint32_t)nq_pad;
        a.words = (uint32_t)W;
        a.sketch_size = (uint32_t)S;
        a.tail_mask = tail_mask(S);
        a.mode = INVQ_COUNTS;
        a.counts = (uint32_t *)d_counts.p;
        HIP_TRY(launch_inv_query(a, ctx->stream));
        t.nq = (uint32_t)nq;
        t.ids = (uint32_t *)d_hits.p;
        t.hit_counts = t.ids + nq * top;
        std::pair<hipEvent_t, hipEvent_t> *ev = timing_slot(ctx);   // (the selection alone, bracketed like the pair kernels: skl_ctx_kernel_ms)
        if (ev) HIP_TRY(hipEventRecord(ev->first, ctx->stream));
        HIP_TRY(launch_inv_top(t, ctx->stream));
        if (ev) HIP_TRY(hipEventRecord(ev->second, ctx->stream));
        HIP_TRY(hipMemcpyAsync(out_ids + q0 * top, t.ids, nq * top * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(out_counts + q0 * top, t.hit_counts, nq * top * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return SKL_OK;
}
