// capi_finish.cpp -- finishing streams of bin minima: skl_sketch_finish / skl_sketch_finish_u16 of
// include/sketchlib_dist.h and the pieces skl_sketch_usigs_packed, skl_sketch_bins_u16_packed (capi_sketch.cpp) and
// skl_sketch_usigs_aa (capi_aa.cpp) put behind each batch's bin-minimum launches.  A destination with bins_u16 set asks for
// the u16 form (an inverted index's rows, any num_bins); otherwise the 14 planes (multiples of 64).  Kernel: sketch_finish.hip; launch rules, flag bits and the host form of the two steps: finish_plan.hpp (pure).
#include "capi_internal.hpp"

#include <algorithm>
#include <atomic>
#include <thread>

using namespace skl;

int finish_check_bins(uint64_t num_bins)
{
    if (num_bins == 0 || num_bins > 0xFFFFFFFFull) return fail(SKL_ERR_INVALID_ARG, "num_bins out of range");
    if (num_bins % 64 != 0) return fail(SKL_ERR_INVALID_ARG, "num_bins must be a multiple of 64 to be finished (bit-sliced words hold 64 bins)");
    return SKL_OK;
}

int finish_check_bins_u16(uint64_t num_bins)
{
    if (num_bins == 0 || num_bins > 0xFFFFFFFFull) return fail(SKL_ERR_INVALID_ARG, "num_bins out of range");
    return SKL_OK;
}

int finish_reserve(skl_ctx *ctx, uint64_t streams, uint64_t num_bins, FinishDev *dev, bool u16)
{
    const uint64_t words = finish_words(num_bins);
    void *p = nullptr;
    if (u16) {   // rows [streams][num_bins] u16, then the flags
        SKL_TRY(ctx_scratch(ctx, (size_t)(streams * num_bins * sizeof(uint16_t) + streams), &p, SCRATCH_SKETCH_FINISHED));
        dev->usigs = dev->first_sign = nullptr;
        dev->bins_u16 = (uint16_t *)p;
        dev->flags = (uint8_t *)(dev->bins_u16 + streams * num_bins);
    } else {
        SKL_TRY(ctx_scratch(ctx, (size_t)(streams * (words + 1) * sizeof(uint64_t) + streams), &p, SCRATCH_SKETCH_FINISHED));
        dev->usigs = (uint64_t *)p;
        dev->first_sign = dev->usigs + streams * words;
        dev->flags = (uint8_t *)(dev->first_sign + streams);
        dev->bins_u16 = nullptr;
    }
    dev->targets = nullptr;
    if (!finish_lds_form(num_bins)) {
        void *t = nullptr;
        SKL_TRY(ctx_scratch(ctx, (size_t)(finish_workgroups(streams, num_bins) * num_bins * sizeof(uint32_t)), &t, SCRATCH_SKETCH_TARGETS));
        dev->targets = (uint32_t *)t;
    }
    return SKL_OK;
}

int finish_launch(skl_ctx *ctx, const uint64_t *d_signs, uint64_t n_streams, uint64_t num_bins, const FinishDev &dev, uint64_t at)
{
    if (n_streams == 0) return SKL_OK;
    FinishArgs a;
    a.signs = d_signs;
    a.n_streams = n_streams;
    a.num_bins = (uint32_t)num_bins;
    a.max_attempts = finish_max_attempts(ctx->knobs.finish_max_attempts);
    const bool u16 = dev.bins_u16 != nullptr;
    a.usigs = u16 ? nullptr : dev.usigs + at * finish_words(num_bins);
    a.first_sign = u16 ? nullptr : dev.first_sign + at;
    a.flags = dev.flags + at;
    a.targets = dev.targets;
    a.bins_u16 = u16 ? dev.bins_u16 + at * num_bins : nullptr;
    std::pair<hipEvent_t, hipEvent_t> *tev = timing_slot(ctx);   // (bracketed like the bin-minimum launches)
    if (tev) HIP_TRY(hipEventRecord(tev->first, ctx->stream));
    HIP_TRY(u16 ? launch_sketch_finish_u16(a, ctx->stream) : launch_sketch_finish(a, ctx->stream));
    if (tev) HIP_TRY(hipEventRecord(tev->second, ctx->stream));
    return SKL_OK;
}

int finish_download(const FinishDev &dev, uint64_t at, uint64_t n_streams, uint64_t num_bins, const FinishDest &dst, uint64_t dst_at,
                    hipStream_t stream)
{
    if (n_streams == 0) return SKL_OK;
    const uint64_t words = finish_words(num_bins);
    if (dst.bins_u16) {
        HIP_TRY(hipMemcpyAsync(dst.bins_u16 + dst_at * num_bins, dev.bins_u16 + at * num_bins, n_streams * num_bins * sizeof(uint16_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(dst.flags + dst_at, dev.flags + at, n_streams, hipMemcpyDeviceToHost, stream));
        return SKL_OK;
    }
    HIP_TRY(hipMemcpyAsync(dst.usigs + dst_at * words, dev.usigs + at * words, n_streams * words * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    if (dst.first_sign) HIP_TRY(hipMemcpyAsync(dst.first_sign + dst_at, dev.first_sign + at, n_streams * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(dst.flags + dst_at, dev.flags + at, n_streams, hipMemcpyDeviceToHost, stream));
    return SKL_OK;
}

// stream `at` of dst from its signs, in the form dst asks for; returns the flag
static uint8_t finish_one_on_host(const uint64_t *signs, uint64_t num_bins, const FinishDest &dst, uint64_t at)
{
    if (dst.bins_u16) return finish_stream_host_u16(signs, num_bins, dst.bins_u16 + at * num_bins);
    return finish_stream_host(signs, num_bins, dst.usigs + at * finish_words(num_bins), dst.first_sign ? dst.first_sign + at : nullptr);
}

int finish_fallback(const uint64_t *d_signs, uint64_t n_streams, uint64_t num_bins, const FinishDest &dst, uint64_t dst_at)
{
    std::vector<uint64_t> raw;
    for (uint64_t s = 0; s < n_streams; ++s) {
        if (!(dst.flags[dst_at + s] & FINISH_UNFINISHED)) continue;
        raw.resize(num_bins);
        HIP_TRY(hipMemcpy(raw.data(), d_signs + s * num_bins, num_bins * sizeof(uint64_t), hipMemcpyDeviceToHost));
        dst.flags[dst_at + s] = (uint8_t)(FINISH_UNFINISHED | finish_one_on_host(raw.data(), num_bins, dst, dst_at + s));
    }
    return SKL_OK;
}

void finish_on_host(const uint64_t *signs, uint64_t n_streams, uint64_t num_bins, const FinishDest &dst, bool only_unfinished)
{
    std::atomic<uint64_t> next{0};
    auto work = [&] {
        for (;;) {
            const uint64_t s = next.fetch_add(1);
            if (s >= n_streams) break;
            if (only_unfinished && !(dst.flags[s] & FINISH_UNFINISHED)) continue;
            const uint8_t flag = finish_one_on_host(signs + s * num_bins, num_bins, dst, s);
            dst.flags[s] = (uint8_t)(flag | (only_unfinished ? FINISH_UNFINISHED : 0));
        }
    };
    const uint64_t t = std::max<uint64_t>(1, std::min<uint64_t>({16, std::thread::hardware_concurrency(), n_streams}));
    std::vector<std::thread> pool;
    for (uint64_t i = 1; i < t; ++i) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
}

const char *finish_kernel_name(const skl_ctx *ctx, uint64_t num_bins, bool u16)
{
    if (u16) {
        if (ctx->knobs.sketch_finish_host) return "densify + u16 bins on host threads (SKL_SKETCH_FINISH=host)";
        return finish_lds_form(num_bins) ? "skl::sketch_finish_kernel (densify + u16 bins, a workgroup per stream, targets in LDS)"
                                         : "skl::sketch_finish_kernel (densify + u16 bins, workgroups walk the streams, targets in global memory)";
    }
    if (ctx->knobs.sketch_finish_host) return "densify + transpose on host threads (SKL_SKETCH_FINISH=host)";
    return finish_lds_form(num_bins) ? "skl::sketch_finish_kernel (densify + 14-plane transpose, a workgroup per stream, targets in LDS)"
                                     : "skl::sketch_finish_kernel (densify + 14-plane transpose, workgroups walk the streams, targets in global memory)";
}

// Signs the caller already holds: up in batches of at most 256 MiB, finished, the words (or u16 rows) back.
static int finish_host_signs(skl_ctx *ctx, const uint64_t *signs, size_t n_streams, uint64_t num_bins, const FinishDest &dst)
{
    const bool u16 = dst.bins_u16 != nullptr;
    ctx->last_kernel = finish_kernel_name(ctx, num_bins, u16);
    if (ctx->knobs.sketch_finish_host) {
        finish_on_host(signs, n_streams, num_bins, dst, false);
        return SKL_OK;
    }
    const uint64_t per_batch = std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)n_streams, 0x7FFFFFFFull, (256ull << 20) / (num_bins * sizeof(uint64_t))}));
    void *d_signs = nullptr;
    SKL_TRY(ctx_scratch(ctx, (size_t)(per_batch * num_bins * sizeof(uint64_t)), &d_signs, SCRATCH_SKETCH_SIGNS));
    FinishDev dev;
    SKL_TRY(finish_reserve(ctx, per_batch, num_bins, &dev, u16));
    for (uint64_t s0 = 0; s0 < n_streams; s0 += per_batch) {
        const uint64_t ns = std::min<uint64_t>(per_batch, n_streams - s0);
        HIP_TRY(hipMemcpyAsync(d_signs, signs + s0 * num_bins, ns * num_bins * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        SKL_TRY(finish_launch(ctx, (const uint64_t *)d_signs, ns, num_bins, dev, 0));
        SKL_TRY(finish_download(dev, 0, ns, num_bins, dst, s0, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    finish_on_host(signs, n_streams, num_bins, dst, true);   // what ran into the probe cap (the caller's copy of the signs is at hand)
    return SKL_OK;
}

extern "C" int skl_sketch_finish(skl_ctx *ctx, const uint64_t *signs, size_t n_streams, uint64_t num_bins, uint64_t *out_usigs,
                                 uint64_t *out_first_sign, uint8_t *out_flags)
{
    SKL_TRY(ctx_bind(ctx));
    if (!signs || !out_usigs || !out_flags) return fail(SKL_ERR_INVALID_ARG, "null argument");
    SKL_TRY(finish_check_bins(num_bins));
    if (n_streams == 0) return SKL_OK;
    return finish_host_signs(ctx, signs, n_streams, num_bins, FinishDest{out_usigs, out_first_sign, out_flags});
}

// The u16 form: any num_bins, `sign as u16` of every densified bin (an inverted index's rows).
extern "C" int skl_sketch_finish_u16(skl_ctx *ctx, const uint64_t *signs, size_t n_streams, uint64_t num_bins, uint16_t *out_bins,
                                     uint8_t *out_flags)
{
    SKL_TRY(ctx_bind(ctx));
    if (!signs || !out_bins || !out_flags) return fail(SKL_ERR_INVALID_ARG, "null argument");
    SKL_TRY(finish_check_bins_u16(num_bins));
    if (n_streams == 0) return SKL_OK;
    return finish_host_signs(ctx, signs, n_streams, num_bins, FinishDest{nullptr, nullptr, out_flags, out_bins});
}
