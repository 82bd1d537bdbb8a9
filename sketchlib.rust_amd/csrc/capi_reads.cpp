// capi_reads.cpp -- the entry points of include/sketchlib_dist.h for read sketching with a count filter: a
// device-resident batch of read sets (skl_reads) and the survivors of a range of window starts under a threshold
// table.  Kernel: read_survivors.hip; its span table: sketch_plan.hpp.  The filter itself is replayed by the caller
// (csrc/host/read_filter.hpp).
#include "capi_internal.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

#include "nthash.hpp"

using namespace skl;

struct skl_reads {
    skl_ctx *ctx = nullptr;
    size_t n_samples = 0, nk = 0;
    uint64_t num_bins = 0;
    int rc = 1;
    std::vector<uint64_t> code_begin;   // host copy: window ranges are clamped against it
    void *d_base = nullptr;    // packed codes | code_begin | offset_begin | word_begin | offsets | top_f | top_r | kmers
    void *d_call = nullptr;    // win_begin | win_end | span_begin | counts | thresholds | survivors (grow-only)
    size_t call_bytes = 0;
    const uint32_t *packed = nullptr;
    const uint64_t *code_begin_d = nullptr, *offset_begin_d = nullptr, *word_begin_d = nullptr, *offsets_d = nullptr;
    const uint64_t *top_f = nullptr, *top_r = nullptr;
    const uint32_t *kmers = nullptr;
};

extern "C" int skl_reads_create(skl_ctx *ctx, const uint32_t *packed, const uint64_t *code_begin, const uint64_t *offsets,
                                const uint64_t *offset_begin, size_t n_samples, const size_t *kmers, size_t nk,
                                uint64_t num_bins, int rc, skl_reads **out)
{
    const RoctxRange range_("skl:reads create");
    if (!out) return fail(SKL_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!ctx) {   // a null context is what a caller without a device has: say so
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
            return fail(SKL_ERR_NO_DEVICE, "no HIP device is visible; this library has no CPU path");
        }
    }
    SKL_TRY(ctx_bind(ctx));
    if (!code_begin || !offset_begin || !kmers) return fail(SKL_ERR_INVALID_ARG, "null argument");
    if (n_samples == 0 || nk == 0) return fail(SKL_ERR_INVALID_ARG, "no samples or no k-mer lengths");
    if (n_samples > 0xFFFFFFFFull || nk > 0xFFFFull) return fail(SKL_ERR_INVALID_ARG, "too many samples or k-mer lengths");
    if (num_bins == 0 || num_bins > 0xFFFFFFFFull) return fail(SKL_ERR_INVALID_ARG, "num_bins out of range");
    const uint64_t n_offs = offset_begin[n_samples];
    if ((code_begin[n_samples] && !packed) || (n_offs && !offsets)) return fail(SKL_ERR_INVALID_ARG, "null argument");
    std::vector<uint64_t> word_begin(n_samples, 0);
    uint64_t words = 0;
    for (size_t s = 0; s < n_samples; ++s) {
        if (code_begin[s + 1] < code_begin[s] || offset_begin[s + 1] < offset_begin[s]) {
            return fail(SKL_ERR_INVALID_ARG, "sample ranges must not decrease");
        }
        word_begin[s] = words;
        words += (code_begin[s + 1] - code_begin[s] + 15) / 16;
    }
    std::vector<uint64_t> top(8 * nk);
    std::vector<uint32_t> k32(nk);
    for (size_t ki = 0; ki < nk; ++ki) {
        if (kmers[ki] == 0 || kmers[ki] > 0xFFFFu) return fail(SKL_ERR_INVALID_ARG, "k-mer length out of range");
        k32[ki] = (uint32_t)kmers[ki];
        nthash_top_tables(kmers[ki], top.data() + ki * 4, top.data() + 4 * nk + ki * 4);
    }
    // layout in u64 words
    const size_t w_packed = (std::max<uint64_t>(words, 1) + 1) / 2;
    const size_t at_cb = w_packed, at_ob = at_cb + n_samples + 1, at_wb = at_ob + n_samples + 1, at_offs = at_wb + n_samples;
    const size_t at_top = at_offs + n_offs, at_k = at_top + 8 * nk, total = at_k + (nk + 1) / 2;
    skl_reads *r = new skl_reads;
    r->ctx = ctx;
    r->n_samples = n_samples;
    r->nk = nk;
    r->num_bins = num_bins;
    r->rc = rc ? 1 : 0;
    r->code_begin.assign(code_begin, code_begin + n_samples + 1);
    const hipError_t e = hipMalloc(&r->d_base, total * sizeof(uint64_t));
    if (e != hipSuccess) {
        delete r;
        return fail(e == hipErrorOutOfMemory ? SKL_ERR_OOM : SKL_ERR_HIP, "hipMalloc of %zu words: %s", total, hipGetErrorString(e));
    }
    uint64_t *d = (uint64_t *)r->d_base;
    r->packed = (const uint32_t *)d;
    r->code_begin_d = d + at_cb;
    r->offset_begin_d = d + at_ob;
    r->word_begin_d = d + at_wb;
    r->offsets_d = d + at_offs;
    r->top_f = d + at_top;
    r->top_r = d + at_top + 4 * nk;
    r->kmers = (const uint32_t *)(d + at_k);
    std::vector<uint64_t> small;
    small.insert(small.end(), code_begin, code_begin + n_samples + 1);
    small.insert(small.end(), offset_begin, offset_begin + n_samples + 1);
    small.insert(small.end(), word_begin.begin(), word_begin.end());
    if (n_offs) small.insert(small.end(), offsets, offsets + n_offs);
    small.insert(small.end(), top.begin(), top.end());
    small.resize(total - at_cb, 0);
    memcpy(small.data() + (at_k - at_cb), k32.data(), nk * sizeof(uint32_t));
    auto copy_up = [&]() -> int {
        if (words) HIP_TRY(hipMemcpyAsync(d, packed, words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d + at_cb, small.data(), small.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return SKL_OK;
    };
    const int rc_ = copy_up();
    if (rc_ != SKL_OK) {
        (void)hipFree(r->d_base);
        delete r;
        return rc_;
    }
    *out = r;
    return SKL_OK;
}

extern "C" int skl_reads_destroy(skl_reads *r)
{
    if (!r) return SKL_OK;
    (void)hipSetDevice(r->ctx->device);
    if (r->d_base) (void)hipFree(r->d_base);
    if (r->d_call) (void)hipFree(r->d_call);
    delete r;
    return SKL_OK;
}

extern "C" int skl_reads_survivors(skl_reads *r, const uint64_t *win_begin, const uint64_t *win_end,
                                   const uint64_t *thresholds, uint64_t capacity, uint64_t *out_survivors,
                                   uint64_t *out_counts)
{
    const RoctxRange range_("skl:reads survivors");
    if (!r) return fail(SKL_ERR_INVALID_ARG, "null handle");
    skl_ctx *ctx = r->ctx;
    SKL_TRY(ctx_bind(ctx));
    if (!win_begin || !win_end || !thresholds || !out_counts || (capacity && !out_survivors)) {
        return fail(SKL_ERR_INVALID_ARG, "null argument");
    }
    const size_t n = r->n_samples, nk = r->nk, streams = n * nk;
    const std::vector<uint64_t> head = read_survivor_spans(r->code_begin.data(), win_begin, win_end, n);   // win_begin | win_end | span_begin
    const uint64_t n_spans = head[3 * n];
    if (capacity > (1ull << 40) / std::max<size_t>(streams, 1)) return fail(SKL_ERR_INVALID_ARG, "capacity too large");
    const size_t at_counts = 3 * n + 1, at_thr = at_counts + streams, at_surv = at_thr + streams * r->num_bins;
    const size_t need = (at_surv + streams * capacity * 2) * sizeof(uint64_t);
    if (need > r->call_bytes) {
        if (r->d_call) HIP_TRY(hipFree(r->d_call));
        r->d_call = nullptr;
        r->call_bytes = 0;
        HIP_TRY(hipMalloc(&r->d_call, need));
        r->call_bytes = need;
    }
    uint64_t *d = (uint64_t *)r->d_call;
    HIP_TRY(hipMemcpyAsync(d, head.data(), head.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(d + at_counts, 0, streams * sizeof(uint64_t), ctx->stream));
    HIP_TRY(hipMemcpyAsync(d + at_thr, thresholds, streams * r->num_bins * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    ReadSurvivorArgs a;
    memset(&a, 0, sizeof a);
    a.packed = r->packed;
    a.word_begin = r->word_begin_d;
    a.code_begin = r->code_begin_d;
    a.offsets = r->offsets_d;
    a.offset_begin = r->offset_begin_d;
    a.win_begin = d;
    a.win_end = d + n;
    a.span_begin = d + 2 * n;
    a.n_spans = n_spans;
    a.n_samples = (uint32_t)n;
    a.nk = (uint32_t)nk;
    a.kmers = r->kmers;
    a.top_f = r->top_f;
    a.top_r = r->top_r;
    a.num_bins = r->num_bins;
    a.bin_size = bin_size_of(r->num_bins);
    a.inv_bin_size = 1.0 / (double)a.bin_size;
    a.rc = r->rc;
    a.thresholds = d + at_thr;
    a.capacity = capacity;
    a.survivors = d + at_surv;
    a.counts = (unsigned long long *)(d + at_counts);
    std::pair<hipEvent_t, hipEvent_t> *tev = timing_slot(ctx);
    if (tev) HIP_TRY(hipEventRecord(tev->first, ctx->stream));
    HIP_TRY(launch_read_survivors(a, ctx->stream));
    if (tev) HIP_TRY(hipEventRecord(tev->second, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out_counts, d + at_counts, streams * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t st = 0; st < streams; ++st) {   // only the records written
        const uint64_t m = std::min(out_counts[st], capacity);
        if (m) {
            HIP_TRY(hipMemcpyAsync(out_survivors + st * capacity * 2, d + at_surv + st * capacity * 2, m * 2 * sizeof(uint64_t),
                                   hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->last_kernel = "skl::read_survivors_kernel (64 window starts per thread, rolling canonical ntHash, signs below the "
                       "threshold of their bin appended per wave)";
    return SKL_OK;
}
