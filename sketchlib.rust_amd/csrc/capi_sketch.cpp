// capi_sketch.cpp -- the DNA sketching entry points of include/sketchlib_dist.h: skl_sketch_signs,
// skl_sketch_signs_packed and their finished forms skl_sketch_usigs_packed, skl_sketch_bins_u16_packed.  Kernel: sketch_kernel.hip;
// which form hashes what and how the samples fall into upload batches: sketch_plan.hpp (pure); the arithmetic: nthash.hpp.
#include "capi_internal.hpp"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>

#include "nthash.hpp"

using namespace skl;

// The bases of samples [s0, s1) packed into dst (the words of sample s start at dst + (word_begin[s] - word_begin[s0])).
static void pack_samples(const uint8_t *codes, const uint64_t *code_begin, const std::vector<uint64_t> &word_begin, size_t s0, size_t s1,
                         uint32_t *dst, unsigned threads)
{
    // work items: (sample, word range) pieces of at most 1 Mi words
    struct Piece { size_t s; uint64_t w0, w1; };
    std::vector<Piece> pieces;
    for (size_t s = s0; s < s1; ++s) {
        const uint64_t words = word_begin[s + 1] - word_begin[s];
        for (uint64_t w = 0; w < words; w += (1ull << 20)) pieces.push_back({s, w, std::min<uint64_t>(words, w + (1ull << 20))});
    }
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t x = next.fetch_add(1);
            if (x >= pieces.size()) break;
            const Piece &pc = pieces[x];
            pack_code_words(codes + code_begin[pc.s], code_begin[pc.s + 1] - code_begin[pc.s], pc.w0, pc.w1,
                            dst + (word_begin[pc.s] - word_begin[s0]));
        }
    };
    const unsigned t = (unsigned)std::max<size_t>(1, std::min<size_t>(threads, pieces.size()));
    std::vector<std::thread> pool;
    for (unsigned i = 1; i < t; ++i) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
}

int sketch_scratch_release(skl_ctx *ctx, bool pinned_ring)
{
    if (ctx->scratch_bytes[SCRATCH_SKETCH_BASES] + ctx->scratch_bytes[SCRATCH_SKETCH_SIGNS] <= (1ull << 30)) return SKL_OK;
    for (int slot : {SCRATCH_SKETCH_BASES, SCRATCH_SKETCH_SIGNS}) {
        if (ctx->scratch[slot]) HIP_TRY(hipFree(ctx->scratch[slot]));
        ctx->scratch[slot] = nullptr;
        ctx->scratch_bytes[slot] = 0;
    }
    if (pinned_ring && ctx->pinned) {
        HIP_TRY(hipHostFree(ctx->pinned));
        ctx->pinned = nullptr;
        ctx->pinned_words = 0;
    }
    return SKL_OK;
}

// skl_sketch_signs / skl_sketch_signs_packed: validate, plan (sketch_plan.hpp), then batch i + 1's upload (the auxiliary stream)
// under batch i's kernel, batch i's signs on their way back under batch i + 1's kernel.  The bases cross PCIe at 2 bits each;
// the device buffers belong to the context (grow-only).  One-byte codes are packed on host threads straight into a pinned
// two-batch ring, so their upload is a true DMA.
static int sketch_signs_impl(skl_ctx *ctx, const uint8_t *codes, const uint32_t *packed, const uint64_t *code_begin,
                             const uint64_t *offsets, const uint64_t *offset_begin, size_t n_samples,
                             const size_t *kmers, size_t nk, uint64_t num_bins, int rc, uint64_t *out_signs,
                             const FinishDest *fin = nullptr)   // fin: the streams are finished on the device and go there; out_signs unused
{
    SKL_TRY(ctx_bind(ctx));
    if (!code_begin || !offset_begin || !kmers || (!out_signs && !fin)) return fail(SKL_ERR_INVALID_ARG, "null argument");
    if (n_samples == 0 || nk == 0) return SKL_OK;
    if (num_bins == 0) return fail(SKL_ERR_INVALID_ARG, "num_bins is zero");
    const uint64_t n_codes = code_begin[n_samples], n_offs = offset_begin[n_samples];
    if ((n_codes && !codes && !packed) || (n_offs && !offsets)) return fail(SKL_ERR_INVALID_ARG, "null argument");
    std::vector<uint32_t> k32(nk);
    std::vector<uint64_t> top_f(nk * 4), top_r(nk * 4);
    size_t kmax = 0;
    for (size_t ki = 0; ki < nk; ++ki) {
        if (kmers[ki] == 0 || kmers[ki] > 0xFFFFu) return fail(SKL_ERR_INVALID_ARG, "k-mer length out of range");
        k32[ki] = (uint32_t)kmers[ki];
        kmax = std::max(kmax, kmers[ki]);
        nthash_top_tables(kmers[ki], top_f.data() + ki * 4, top_r.data() + ki * 4);
    }
    for (size_t s = 0; s < n_samples; ++s) {
        if (code_begin[s + 1] < code_begin[s] || offset_begin[s + 1] < offset_begin[s]) {
            return fail(SKL_ERR_INVALID_ARG, "sample ranges must not decrease");
        }
    }
    const SketchPlan plan = sketch_plan(code_begin, n_samples, kmax, ctx->knobs.sketch_global);   // (SKL_SKETCH_KERNEL=global: A/B)
    const std::vector<uint64_t> &span_begin = plan.span_begin, &word_begin = plan.word_begin;
    // batches of whole samples (SKL_SKETCH_BATCH_WORDS: tests cut small inputs into several)
    const std::vector<size_t> cuts = sketch_upload_batches(
        word_begin.data(), n_samples, ctx->knobs.sketch_batch_words > 0 ? (uint64_t)ctx->knobs.sketch_batch_words : SKETCH_BATCH_WORDS);
    const size_t n_batches = cuts.size() - 1;
    const uint64_t total_words = word_begin[n_samples];
    const size_t sign_words = n_samples * nk * num_bins;
    // device buffers of the context: packed codes | signs | the small arrays
    void *d_packed = nullptr, *d_signs = nullptr, *d_small = nullptr;
    SKL_TRY(ctx_scratch(ctx, std::max<uint64_t>(total_words, 4) * sizeof(uint32_t), &d_packed, SCRATCH_SKETCH_BASES));
    SKL_TRY(ctx_scratch(ctx, sign_words * sizeof(uint64_t), &d_signs, SCRATCH_SKETCH_SIGNS));
    const size_t small_words = 4 * (n_samples + 1) + n_offs + 9 * nk + 8;   // u64 each (the k-mer lengths: two per word)
    SKL_TRY(ctx_scratch(ctx, small_words * sizeof(uint64_t), &d_small, SCRATCH_SKETCH_SMALL));
    FinishDev fin_dev;
    if (fin) SKL_TRY(finish_reserve(ctx, n_samples * nk, num_bins, &fin_dev, fin->bins_u16 != nullptr));
    std::vector<uint64_t> small;
    small.reserve(small_words);
    auto put = [&](const uint64_t *v, size_t count) {
        const size_t at = small.size();
        small.insert(small.end(), v, v + count);
        return at;
    };
    const size_t at_cb = put(code_begin, n_samples + 1), at_ob = put(offset_begin, n_samples + 1), at_sb = put(span_begin.data(), n_samples + 1);
    const size_t at_wb = put(word_begin.data(), n_samples), at_offs = put(offsets, n_offs);
    const size_t at_tf = put(top_f.data(), top_f.size()), at_tr = put(top_r.data(), top_r.size());
    const size_t at_k = small.size();
    small.resize(at_k + (nk + 1) / 2, 0);
    memcpy(small.data() + at_k, k32.data(), nk * sizeof(uint32_t));
    if (small.size() > small_words) return fail(SKL_ERR_INVALID_ARG, "internal: small-array layout");
    HIP_TRY(hipMemcpyAsync(d_small, small.data(), small.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_signs, 0xFF, sign_words * sizeof(uint64_t), ctx->stream));   // u64::MAX
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // (`small` is pageable: uploaded before it dies; the aux stream starts behind this)

    SketchArgs a;
    memset(&a, 0, sizeof a);
    const uint64_t *ds = (const uint64_t *)d_small;
    a.packed = (const uint32_t *)d_packed;
    a.word_begin = ds + at_wb;
    a.code_begin = ds + at_cb;
    a.offsets = ds + at_offs;
    a.offset_begin = ds + at_ob;
    a.span_begin = ds + at_sb;
    a.n_samples = (uint32_t)n_samples;
    a.nk = (uint32_t)nk;
    a.kmers = (const uint32_t *)(ds + at_k);
    a.top_f = ds + at_tf;
    a.top_r = ds + at_tr;
    a.num_bins = num_bins;
    a.bin_size = bin_size_of(num_bins);
    a.inv_bin_size = 1.0 / (double)a.bin_size;
    a.rc = rc ? 1 : 0;
    a.signs = (uint64_t *)d_signs;
    a.lds_form = plan.lds_form ? 1u : 0u;

    // one-byte codes: packed on host threads into a pinned ring of two batches (grow-only, kept by the context)
    uint64_t ring_words = 0;
    if (!packed) {
        for (size_t b = 0; b < n_batches; ++b) ring_words = std::max(ring_words, word_begin[cuts[b + 1]] - word_begin[cuts[b]]);
        if (ctx->pinned_words < 2 * ring_words) {
            if (ctx->pinned) HIP_TRY(hipHostFree(ctx->pinned));
            ctx->pinned = nullptr;
            ctx->pinned_words = 0;
            HIP_TRY(hipHostMalloc((void **)&ctx->pinned, std::max<uint64_t>(2 * ring_words, 4) * sizeof(uint32_t), hipHostMallocDefault));
            ctx->pinned_words = 2 * ring_words;
        }
    }
    std::vector<hipEvent_t> ev(3 * n_batches, nullptr);   // per batch: uploaded, hashed, (ring slot) free again
    struct EventGuard {
        std::vector<hipEvent_t> &e;
        ~EventGuard() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } guard{ev};
    for (auto &e : ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const unsigned pack_threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    auto upload = [&](size_t b) -> int {
        const RoctxRange range_("skl:sketch_batch pack + upload");
        const size_t s0 = cuts[b], s1 = cuts[b + 1];
        const uint64_t w0 = word_begin[s0], words = word_begin[s1] - w0;
        if (words == 0) {
            HIP_TRY(hipEventRecord(ev[3 * b], ctx->aux_stream));
            return SKL_OK;
        }
        const uint32_t *src;
        if (packed) {
            src = packed + w0;
        } else {
            uint32_t *slot = ctx->pinned + (b & 1) * ring_words;
            if (b >= 2) HIP_TRY(hipEventSynchronize(ev[3 * (b - 2) + 2]));   // that slot's previous upload has left it
            pack_samples(codes, code_begin, word_begin, s0, s1, slot, pack_threads);
            src = slot;
        }
        HIP_TRY(hipMemcpyAsync((uint32_t *)d_packed + w0, src, words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->aux_stream));
        HIP_TRY(hipEventRecord(ev[3 * b], ctx->aux_stream));
        HIP_TRY(hipEventRecord(ev[3 * b + 2], ctx->aux_stream));
        return SKL_OK;
    };
    auto launch = [&](size_t b) -> int {
        const RoctxRange range_("skl:sketch_batch hash + bin minima");
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ev[3 * b], 0));
        a.first_span = span_begin[cuts[b]];
        a.n_spans = span_begin[cuts[b + 1]] - a.first_span;
        std::pair<hipEvent_t, hipEvent_t> *tev = timing_slot(ctx);   // (bracketed like the pair kernels, batch by batch)
        if (tev) HIP_TRY(hipEventRecord(tev->first, ctx->stream));
        HIP_TRY(launch_sketch_signs(a, ctx->stream));
        if (tev) HIP_TRY(hipEventRecord(tev->second, ctx->stream));
        if (fin) {   // densify + transpose behind the batch's bin minima, ahead of its download
            const size_t s0 = cuts[b], s1 = cuts[b + 1];
            SKL_TRY(finish_launch(ctx, (const uint64_t *)d_signs + s0 * nk * num_bins, (s1 - s0) * nk, num_bins, fin_dev, s0 * nk));
        }
        HIP_TRY(hipEventRecord(ev[3 * b + 1], ctx->stream));
        return SKL_OK;
    };
    auto download = [&](size_t b) -> int {   // (a copy into pageable memory blocks its caller: issued after the next batch's launch)
        const size_t s0 = cuts[b], s1 = cuts[b + 1];
        HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ev[3 * b + 1], 0));
        if (fin) return finish_download(fin_dev, s0 * nk, (s1 - s0) * nk, num_bins, *fin, s0 * nk, ctx->aux_stream);
        HIP_TRY(hipMemcpyAsync(out_signs + s0 * nk * num_bins, (const uint64_t *)d_signs + s0 * nk * num_bins,
                               (s1 - s0) * nk * num_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->aux_stream));
        return SKL_OK;
    };
    SKL_TRY(upload(0));
    SKL_TRY(launch(0));
    for (size_t b = 0; b < n_batches; ++b) {
        if (b + 1 < n_batches) {
            SKL_TRY(upload(b + 1));
            SKL_TRY(launch(b + 1));
        }
        SKL_TRY(download(b));
    }
    ctx->last_kernel = !plan.lds_form ? "skl::nthash_binmin_kernel (256 window starts per thread, rolling canonical ntHash, atomicMin per bin)"
                       : num_bins <= (uint64_t)SKETCH_LDS_BINS_MAX
                           ? "skl::nthash_binmin_lds_kernel (bases staged in LDS as 2-bit codes, 128 window starts per thread, rolling "
                             "canonical ntHash through a fused 16-entry step table, bin minima in LDS)"
                           : "skl::nthash_binmin_lds_kernel (bases staged in LDS as 2-bit codes, 128 window starts per thread, rolling "
                             "canonical ntHash through a fused 16-entry step table, bin minima in global memory)";
    HIP_TRY(hipStreamSynchronize(ctx->aux_stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (fin) {   // (the call's signs are all still on the device)
        ctx->last_kernel += std::string(" + ") + finish_kernel_name(ctx, num_bins, fin->bins_u16 != nullptr);
        SKL_TRY(finish_fallback((const uint64_t *)d_signs, n_samples * nk, num_bins, *fin, 0));
    }
    return sketch_scratch_release(ctx, true);   // (both streams are idle here)
}

extern "C" int skl_sketch_signs(skl_ctx *ctx, const uint8_t *codes, const uint64_t *code_begin,
                                const uint64_t *offsets, const uint64_t *offset_begin, size_t n_samples,
                                const size_t *kmers, size_t nk, uint64_t num_bins, int rc, uint64_t *out_signs)
{
    return sketch_signs_impl(ctx, codes, nullptr, code_begin, offsets, offset_begin, n_samples, kmers, nk, num_bins, rc, out_signs);
}

extern "C" int skl_sketch_signs_packed(skl_ctx *ctx, const uint32_t *packed, const uint64_t *code_begin,
                                       const uint64_t *offsets, const uint64_t *offset_begin, size_t n_samples,
                                       const size_t *kmers, size_t nk, uint64_t num_bins, int rc, uint64_t *out_signs)
{
    if (!packed && code_begin && n_samples && code_begin[n_samples]) return fail(SKL_ERR_INVALID_ARG, "null argument");
    return sketch_signs_impl(ctx, nullptr, packed, code_begin, offsets, offset_begin, n_samples, kmers, nk, num_bins, rc, out_signs);
}

// The same call with every (sample, k) stream finished: densify_bin and the 14-plane transpose on the device, behind each
// batch's bin minima (SKL_SKETCH_FINISH=host: the signs come back and host threads finish them, as callers did before).
extern "C" int skl_sketch_usigs_packed(skl_ctx *ctx, const uint32_t *packed, const uint64_t *code_begin,
                                       const uint64_t *offsets, const uint64_t *offset_begin, size_t n_samples,
                                       const size_t *kmers, size_t nk, uint64_t num_bins, int rc, uint64_t *out_usigs,
                                       uint64_t *out_first_sign, uint8_t *out_flags)
{
    SKL_TRY(ctx_bind(ctx));
    if (!out_usigs || !out_flags) return fail(SKL_ERR_INVALID_ARG, "null argument");
    if (!packed && code_begin && n_samples && code_begin[n_samples]) return fail(SKL_ERR_INVALID_ARG, "null argument");
    SKL_TRY(finish_check_bins(num_bins));
    return sketch_finished_call(ctx, n_samples * nk, num_bins, FinishDest{out_usigs, out_first_sign, out_flags},
                                [&](uint64_t *signs, const FinishDest *fin) {
                                    return sketch_signs_impl(ctx, nullptr, packed, code_begin, offsets, offset_begin, n_samples, kmers, nk,
                                                             num_bins, rc, signs, fin);
                                });
}

// An inverted index's rows: one k-mer length, exactly num_bins bins (any count), the u16 finish behind each batch's bin
// minima on the same stream -- 2 num_bins bytes and a flag byte come home per sample.
extern "C" int skl_sketch_bins_u16_packed(skl_ctx *ctx, const uint32_t *packed, const uint64_t *code_begin,
                                          const uint64_t *offsets, const uint64_t *offset_begin, size_t n_samples,
                                          size_t kmer, uint64_t num_bins, int rc, uint16_t *out_bins, uint8_t *out_flags)
{
    SKL_TRY(ctx_bind(ctx));
    if (!out_bins || !out_flags) return fail(SKL_ERR_INVALID_ARG, "null argument");
    if (!packed && code_begin && n_samples && code_begin[n_samples]) return fail(SKL_ERR_INVALID_ARG, "null argument");
    SKL_TRY(finish_check_bins_u16(num_bins));
    return sketch_finished_call(ctx, n_samples, num_bins, FinishDest{nullptr, nullptr, out_flags, out_bins},
                                [&](uint64_t *signs, const FinishDest *fin) {
                                    return sketch_signs_impl(ctx, nullptr, packed, code_begin, offsets, offset_begin, n_samples, &kmer, 1,
                                                             num_bins, rc, signs, fin);
                                });
}
