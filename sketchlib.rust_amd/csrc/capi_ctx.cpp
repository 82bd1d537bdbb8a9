// capi_ctx.cpp -- the context of include/sketchlib_dist.h: error plumbing, the handle registry, a context's life cycle, streams
// and grow-only scratch, the timing of pair-kernel launches, the clock sampler and the small diagnostics a context answers.
//
// There is deliberately no CPU compute path in this library: if HIP cannot run, calls fail.
#include "capi_internal.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <vector>

using namespace skl;

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------

static thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}



extern "C" const char *skl_last_error(void) { return g_last_error.c_str(); }
extern "C" int skl_abi_version(void) { return SKL_ABI_VERSION; }

static bool is_gfx950(int dev)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

extern "C" int skl_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int d = 0; d < n; ++d) ok += is_gfx950(d) ? 1 : 0;
    return ok;
}

// ---------------------------------------------------------------------------
// handle registry: destroy calls in any order (and twice) must be harmless -- a binding's
// finalisers run in arbitrary order at interpreter shutdown.
// ---------------------------------------------------------------------------

std::mutex g_registry_mutex;
std::set<const void *> g_live_sketches;
static std::set<const void *> g_live_ctx;

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------

int ctx_bind(skl_ctx *ctx)
{
    if (!ctx) return fail(SKL_ERR_INVALID_ARG, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
#ifdef SKL_AB
    // A/B build only: one process interleaves variants (scripts/ab_sweep.py), so the switches are read at
    // every API entry -- before any dispatch decision of the call, not in the middle of it
    ctx->knobs = read_knobs();
#endif
    return SKL_OK;
}

int ctx_scratch(skl_ctx *ctx, size_t bytes, void **out, ScratchSlot which)
{
    void *&buf = ctx->scratch[which];
    size_t &cap = ctx->scratch_bytes[which];
    if (bytes > cap) {
        if (buf) {
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            HIP_TRY(hipFree(buf));
            buf = nullptr;
            cap = 0;
        }
        HIP_TRY(hipMalloc(&buf, bytes));
        cap = bytes;
        if (which == SCRATCH_COUNTS) ctx->clean_plane1 = nullptr;   // a new counts scratch: nothing is known to be zero in it
    }
    *out = buf;
    return SKL_OK;
}

extern "C" int skl_ctx_create(int device, skl_ctx **out)
{
    if (!out) return fail(SKL_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        return fail(SKL_ERR_NO_DEVICE, "no HIP device is visible; this library has no CPU path");
    }
    if (device < 0 || device >= n) {
        return fail(SKL_ERR_INVALID_ARG, "device %d out of range (0..%d)", device, n - 1);
    }
    if (!is_gfx950(device)) {
        return fail(SKL_ERR_NO_DEVICE, "device %d is not gfx950 (MI355X); kernels are built for gfx950 only",
                    device);
    }
    HIP_TRY(hipSetDevice(device));
    skl_ctx *ctx = new skl_ctx();
    ctx->device = device;
    ctx->knobs = read_knobs();
    ctx->timing_every = ctx->knobs.timing_every;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ctx->n_cu = prop.multiProcessorCount;
    }
    hipError_t e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete ctx;
        return fail(SKL_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    ctx->stream = ctx->own_stream;
    e = hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking);
    for (int x = 0; x < 2 && e == hipSuccess; ++x) {
        e = hipEventCreateWithFlags(&ctx->knn_pair_done[x], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->knn_topk_done[x], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        delete ctx;
        return fail(SKL_ERR_HIP, "stream/event creation: %s", hipGetErrorString(e));
    }
    {
        std::lock_guard<std::mutex> lock(g_registry_mutex);
        g_live_ctx.insert(ctx);
    }
    *out = ctx;
    return SKL_OK;
}

extern "C" int skl_ctx_destroy(skl_ctx *ctx)
{
    if (!ctx) return SKL_OK;
    std::lock_guard<std::mutex> lock(g_registry_mutex);
    if (!g_live_ctx.erase(ctx)) return SKL_OK;  // already destroyed
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->aux_stream) (void)hipStreamSynchronize(ctx->aux_stream);
    if (ctx->epi_stream) (void)hipStreamSynchronize(ctx->epi_stream);
    // slabs die with their context; their handles become inert
    const std::set<skl_sketches *> owned = ctx->sketches;
    for (skl_sketches *s : owned) free_sketches_locked(s);
    for (auto &ev : ctx->events) {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    for (void *buf : ctx->scratch) {
        if (buf) (void)hipFree(buf);
    }
    if (ctx->sampler_stop) {
        *(volatile uint32_t *)ctx->sampler_stop = 1u;   // a sampler still running ends at its next poll
        if (ctx->sampler_stream) (void)hipStreamSynchronize(ctx->sampler_stream);
        (void)hipHostFree(ctx->sampler_stop);
    }
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    free_plans(ctx);
    for (hipEvent_t ev : ctx->eb_events) {
        if (ev) (void)hipEventDestroy(ev);
    }
    if (ctx->eb_counter) (void)hipFree(ctx->eb_counter);
    if (ctx->sampler_buf) (void)hipFree(ctx->sampler_buf);
    if (ctx->sampler_count) (void)hipFree(ctx->sampler_count);
    if (ctx->sampler_stream) (void)hipStreamDestroy(ctx->sampler_stream);
    if (ctx->tile_scratch.d_prefix) (void)hipFree(ctx->tile_scratch.d_prefix);
    if (ctx->tile_scratch.h_staging) (void)hipHostFree(ctx->tile_scratch.h_staging);
    if (ctx->tile_scratch.staged) (void)hipEventDestroy(ctx->tile_scratch.staged);
    for (uint4 *d : ctx->tile_scratch.d_units) {
        if (d) (void)hipFree(d);
    }
    if (ctx->tile_scratch.h_units) (void)hipHostFree(ctx->tile_scratch.h_units);
    if (ctx->tile_scratch.units_staged) (void)hipEventDestroy(ctx->tile_scratch.units_staged);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    if (ctx->aux_stream) (void)hipStreamDestroy(ctx->aux_stream);
    if (ctx->epi_stream) (void)hipStreamDestroy(ctx->epi_stream);
    for (int x = 0; x < 2; ++x) {
        if (ctx->knn_pair_done[x]) (void)hipEventDestroy(ctx->knn_pair_done[x]);
        if (ctx->knn_topk_done[x]) (void)hipEventDestroy(ctx->knn_topk_done[x]);
    }
    delete ctx;
    return SKL_OK;
}

extern "C" int skl_ctx_set_stream(skl_ctx *ctx, void *hip_stream)
{
    SKL_TRY(ctx_bind(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return SKL_OK;
}

extern "C" int skl_ctx_use_default_stream(skl_ctx *ctx)
{
    SKL_TRY(ctx_bind(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->stream = nullptr;   // the legacy default stream: ordered with every blocking stream
    return SKL_OK;
}

extern "C" int skl_ctx_synchronize(skl_ctx *ctx)
{
    SKL_TRY(ctx_bind(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SKL_OK;
}

extern "C" int skl_ctx_reload_env(skl_ctx *ctx)
{
    SKL_TRY(ctx_bind(ctx));
    ctx->knobs = read_knobs();
    ctx->timing_every = ctx->knobs.timing_every;
    return SKL_OK;
}

// Pair-kernel timing is a diagnostic and OFF unless asked for: an event record is a barrier packet on the queue, and two
// per launch cost a sub-millisecond launch ~5 us.  every = 0: off (the default); N >= 1: every N-th launch is bracketed.
extern "C" int skl_ctx_early_break_stats(skl_ctx *ctx, uint64_t *pairs, uint64_t *completed_one_by_one)
{
    SKL_TRY(ctx_bind(ctx));
    uint64_t done = 0;
    if (ctx->eb_counter) {
        std::vector<uint32_t> slots(1024, 0u);
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->aux_stream));
        HIP_TRY(hipMemcpy(slots.data(), ctx->eb_counter, slots.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (const uint32_t v : slots) done += v;
    }
    if (pairs) *pairs = ctx->eb_pairs;
    if (completed_one_by_one) *completed_one_by_one = done;
    return SKL_OK;
}

extern "C" int skl_ctx_set_unit_table(skl_ctx *ctx, int mode)
{
    if (!ctx) return fail(SKL_ERR_INVALID_ARG, "skl_ctx_set_unit_table: null context");
    if (mode < -1 || mode > 1) return fail(SKL_ERR_INVALID_ARG, "skl_ctx_set_unit_table: mode = %d must be -1, 0 or 1", mode);
    ctx->unit_table_mode = mode;
    return SKL_OK;
}

extern "C" int skl_ctx_unit_table(skl_ctx *ctx, int *last_launch_read_one, uint64_t *hits, uint64_t *builds)
{
    if (!ctx) return fail(SKL_ERR_INVALID_ARG, "skl_ctx_unit_table: null context");
    if (last_launch_read_one) *last_launch_read_one = ctx->last_unit_table ? 1 : 0;
    if (hits) *hits = ctx->tile_scratch.units.hits;
    if (builds) *builds = ctx->tile_scratch.units.builds;
    return SKL_OK;
}

extern "C" int skl_ctx_timing_enable(skl_ctx *ctx, int every)
{
    SKL_TRY(ctx_bind(ctx));
    if (every < 0) return fail(SKL_ERR_INVALID_ARG, "skl_ctx_timing_enable: every = %d must be >= 0", every);
    ctx->timing_every = every;
    ctx->launches_seen = 0;
    return SKL_OK;
}

// Shader clock under load.  start(): launches the one-wave sampler (kernels.hip) on a stream of its own;
// the caller then runs whatever it wants measured and, once THAT work is complete (skl_ctx_synchronize:
// a device-wide synchronisation would wait for the sampler itself), calls stop(), which raises the flag,
// waits for the sampler and reduces its (shader counter, 100 MHz counter) pairs to clock readings, one
// per sampling interval.  The sampler also ends by itself after max_samples intervals.
extern "C" int skl_clock_sampler_start(skl_ctx *ctx, uint32_t interval_us, uint32_t max_samples)
{
    SKL_TRY(ctx_bind(ctx));
    if (ctx->sampler_running) return fail(SKL_ERR_INVALID_ARG, "the clock sampler is already running");
    if (max_samples < 2 || max_samples > (1u << 22)) return fail(SKL_ERR_INVALID_ARG, "max_samples out of range");
    // The sampler ends by itself after interval_us x max_samples: anything that synchronises the whole device while it runs
    // (hipMalloc / hipFree inside a sampled call) waits that long at worst, so the product is capped at 10 s.
    if ((uint64_t)std::max(4u, interval_us) * max_samples > 10000000ull) {
        return fail(SKL_ERR_INVALID_ARG, "clock sampler: interval_us x max_samples = %llu us exceeds the 10 s cap",
                    (unsigned long long)std::max(4u, interval_us) * max_samples);
    }
    if (!ctx->sampler_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->sampler_stream, hipStreamNonBlocking));
    if (!ctx->sampler_stop) HIP_TRY(hipHostMalloc((void **)&ctx->sampler_stop, sizeof(uint32_t), hipHostMallocMapped));
    if (!ctx->sampler_count) HIP_TRY(hipMalloc((void **)&ctx->sampler_count, sizeof(uint32_t)));
    if (ctx->sampler_max < max_samples) {
        if (ctx->sampler_buf) HIP_TRY(hipFree(ctx->sampler_buf));
        ctx->sampler_buf = nullptr;
        ctx->sampler_max = 0;
        HIP_TRY(hipMalloc((void **)&ctx->sampler_buf, (size_t)max_samples * 2 * sizeof(uint64_t)));
        ctx->sampler_max = max_samples;
    }
    *(volatile uint32_t *)ctx->sampler_stop = 0u;
    uint32_t *stop_dev = nullptr;
    HIP_TRY(hipHostGetDevicePointer((void **)&stop_dev, ctx->sampler_stop, 0));
    HIP_TRY(hipMemsetAsync(ctx->sampler_count, 0, sizeof(uint32_t), ctx->sampler_stream));
    const uint32_t sleeps = std::max(1u, interval_us / 4u);   // s_sleep 127 = 8 128 cycles ~ 4 us
    HIP_TRY(launch_clock_sampler(stop_dev, ctx->sampler_buf, max_samples, sleeps, ctx->sampler_count, ctx->sampler_stream));
    ctx->sampler_running = true;
    return SKL_OK;
}

extern "C" int skl_clock_sampler_stop(skl_ctx *ctx, double *ghz_median, double *ghz_p10, double *ghz_p90, double *ghz_mean,
                                      int *n_intervals)
{
    SKL_TRY(ctx_bind(ctx));
    if (!ctx->sampler_running) return fail(SKL_ERR_INVALID_ARG, "the clock sampler is not running");
    *(volatile uint32_t *)ctx->sampler_stop = 1u;
    ctx->sampler_running = false;
    HIP_TRY(hipStreamSynchronize(ctx->sampler_stream));
    uint32_t count = 0;
    HIP_TRY(hipMemcpy(&count, ctx->sampler_count, sizeof count, hipMemcpyDeviceToHost));
    std::vector<uint64_t> s((size_t)count * 2);
    if (count) HIP_TRY(hipMemcpy(s.data(), ctx->sampler_buf, s.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    std::vector<double> ghz;
    for (uint32_t i = 1; i < count; ++i) {
        const uint64_t dt = s[2 * i] - s[2 * i - 2], dr = s[2 * i + 1] - s[2 * i - 1];
        if (dr > 0) ghz.push_back((double)dt / (double)dr * 0.1);   // shader cycles per 10 ns tick
    }
    std::sort(ghz.begin(), ghz.end());
    const auto at = [&](double q) { return ghz.empty() ? 0.0 : ghz[std::min(ghz.size() - 1, (size_t)(q * (double)ghz.size()))]; };
    if (ghz_median) *ghz_median = at(0.5);
    if (ghz_p10) *ghz_p10 = at(0.1);
    if (ghz_p90) *ghz_p90 = at(0.9);
    if (ghz_mean) *ghz_mean = count >= 2 && s[2 * count - 1] > s[1] ? (double)(s[2 * count - 2] - s[0]) / (double)(s[2 * count - 1] - s[1]) * 0.1 : 0.0;
    if (n_intervals) *n_intervals = (int)ghz.size();
    return SKL_OK;
}

extern "C" const char *skl_ctx_last_kernel(skl_ctx *ctx) { return ctx ? ctx->last_kernel.c_str() : ""; }

extern "C" int skl_ctx_timing_reset(skl_ctx *ctx)
{
    SKL_TRY(ctx_bind(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->events_used = 0;
    ctx->launches_seen = 0;   // the every-N-th count starts here: the first launch after a reset is bracketed
    return SKL_OK;
}

extern "C" int skl_ctx_kernel_ms(skl_ctx *ctx, float *total_ms, int *n_launches)
{
    SKL_TRY(ctx_bind(ctx));
    if (!total_ms) return fail(SKL_ERR_INVALID_ARG, "total_ms is null");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float total = 0.f;
    for (size_t i = 0; i < ctx->events_used; ++i) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, ctx->events[i].first, ctx->events[i].second));
        total += t;
    }
    *total_ms = total;
    if (n_launches) *n_launches = (int)ctx->events_used;
    return SKL_OK;
}

std::pair<hipEvent_t, hipEvent_t> *timing_slot(skl_ctx *ctx)
{
    if (ctx->timing_every <= 0) return nullptr;
    if (ctx->events_used == ctx->events.size() && ctx->events.size() < 4096) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess) return nullptr;
        if (hipEventCreate(&b) != hipSuccess) {
            (void)hipEventDestroy(a);
            return nullptr;
        }
        ctx->events.emplace_back(a, b);
    }
    return ctx->events_used < ctx->events.size() ? &ctx->events[ctx->events_used++] : nullptr;
}
