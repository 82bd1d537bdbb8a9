// capi.cpp -- implementation of include/sketchlib_dist.h on top of kernels.hip.
//
// Host-side responsibilities: device slabs (the MultiSketch bins in the two layouts
// the pair kernel wants), the samebits -> ln(J) / distance tables (computed with the
// host libm, i.e. bit-identical to what the reference's f64::ln produces on this
// machine), banding of large pair spaces through bounded scratch, and mapping the
// reference's panics to status codes.
//
// There is deliberately no CPU compute path here: if HIP cannot run, calls fail.
#include "capi_internal.hpp"
#include "glibc_log.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
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

static std::mutex g_registry_mutex;
static std::set<const void *> g_live_ctx, g_live_sketches;

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

static void free_sketches_locked(skl_sketches *s);
void free_plans(skl_ctx *ctx);
uint64_t next_generation();

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

static long long env_int(const char *name, long long dflt)
{
    const char *e = getenv(name);
    return (e && *e) ? atoll(e) : dflt;
}

Knobs read_knobs()
{
    Knobs k;
    // The product library reads EIGHTEEN switches: the timing cadence, the device topology the tile order assumes, and the knobs
    // with which the tests force the banded / sliced / 32-row / striped / cost-ordered forms (and the inverted query's bands, the sketching call's upload batches, where and how far its streams are finished, the pair list's bands) on inputs small enough for the oracle.  Everything that
    // exists only to time one form against another ("A/B only, results identical") is read by the A/B build alone (-DSKL_AB),
    // where scripts/ab_sweep.py, scripts/forced_switch_suites.sh and the tests marked `ab_library` find it.
    k.timing_every = std::max(0ll, env_int("SKL_TIMING_EVERY", 0));
    k.sliced_max_pairs = env_int("SKL_SLICED_MAX_PAIRS", -1);
    k.knn_band_rows = std::max(0ll, env_int("SKL_KNN_BAND_ROWS", 0));
    k.invq_band_bytes = std::max(0ll, env_int("SKL_INVQ_BAND_BYTES", 0));
    k.invq_top_digit_bits = std::max(0ll, env_int("SKL_INVQ_TOP_DIGIT_BITS", 0));
    {
        const long long w = env_int("SKL_SKETCH_BATCH_WORDS", 0);   // 0 or unset: 8 Mi; any other value: at least 1
        k.sketch_batch_words = w == 0 ? 0 : std::max(1ll, w);
    }
    k.aa_batch_sign_bytes = std::max(0ll, env_int("SKL_AA_BATCH_SIGN_BYTES", 0));
    k.aa_long_min = std::max(0ll, env_int("SKL_AA_LONG_MIN", 0));
    k.pairs_band = std::max(0ll, env_int("SKL_PAIRS_BAND", 0));
    k.finish_max_attempts = std::max(0ll, env_int("SKL_FINISH_MAX_ATTEMPTS", 0));
    {
        const char *fin = getenv("SKL_SKETCH_FINISH");
        k.sketch_finish_host = fin && strcmp(fin, "host") == 0;
    }
    k.tail_slices = (int)std::min(8ll, std::max(0ll, env_int("SKL_TAIL_SLICES", 4)));
    k.tail_max_pct = env_int("SKL_TAIL_MAX_PCT", 90);
    k.tile32_min = env_int("SKL_TILE32_MIN", 8ll << 20);
    k.group_span = (int)std::min(64ll, std::max(1ll, env_int("SKL_GROUP_SPAN", 2)));
    k.xcds = (int)std::min(8ll, std::max(0ll, env_int("SKL_XCDS", 0)));
    k.eb_stripes = (int)std::min(1ll, std::max(-1ll, env_int("SKL_EB_STRIPES", -1)));
    k.tile_cost_order = (int)std::min(1ll, std::max(-1ll, env_int("SKL_TILE_COST_ORDER", -1)));
#ifdef SKL_AB
    k.k_slices = (int)env_int("SKL_K_SLICES", 0);
    k.round_priority = env_int("SKL_ROUND_PRIORITY", 1) != 0;
    k.half_tiles = env_int("SKL_HALF_TILES", 1) != 0;
    k.mid_band = env_int("SKL_MID_BAND", 1) != 0;
    k.knn_symmetric = env_int("SKL_KNN_SYMMETRIC", 1) != 0;
    k.knn_overlap = env_int("SKL_KNN_OVERLAP", 1) != 0;
    k.knn_prune = env_int("SKL_KNN_PRUNE", 1) != 0;
    k.knn_panel = env_int("SKL_KNN_PANEL", 0);
    k.knn_sparse = env_int("SKL_KNN_SPARSE", 1) != 0;
    k.early_break = (int)std::min(7ll, std::max(0ll, env_int("SKL_EARLY_BREAK", 1)));
    k.epilogue_r5 = env_int("SKL_EPILOGUE_R5", 0) != 0;
    k.eb_pipeline = (int)env_int("SKL_EB_PIPELINE", -1);
    k.eb_pipeline_min = std::max(2ll, env_int("SKL_EB_PIPELINE_MIN", 64ll << 20));
    k.counts_u16 = env_int("SKL_COUNTS_U16", 1) != 0;
    k.eb_lds_rows = env_int("SKL_EB_LDS_ROWS", 1) != 0;
    k.eb_ahead = env_int("SKL_EB_AHEAD", 1) != 0;
    k.eb_lean = env_int("SKL_EB_LEAN", 1) != 0;
    k.knn_epi_blocked = (int)std::min(2ll, std::max(0ll, env_int("SKL_KNN_EPI_BLOCKED", 1)));
    k.eb_blocked = (int)env_int("SKL_EB_BLOCKED", -1);
    k.eb_blk_row_shift = (int)env_int("SKL_EB_BLK_ROW_SHIFT", 10);
    k.fuse_epilogue = env_int("SKL_FUSE_EPILOGUE", 0) != 0;
    k.refheap_wave = env_int("SKL_REFHEAP_WAVE", 1) != 0;
    k.knn_row_flags = env_int("SKL_KNN_ROW_FLAGS", 1) != 0;
    k.topk_stream = env_int("SKL_TOPK_STREAM", 1) != 0;
    k.cand_symmetric = env_int("SKL_CAND_SYMMETRIC", 1) != 0;
    k.cand_row_order = env_int("SKL_CAND_ROW_ORDER", 1) != 0;
    {
        const char *ck = getenv("SKL_CAND_KERNEL");
        k.cand_lanes = ck && strcmp(ck, "lanes") == 0;
    }
    k.inline_prefix = env_int("SKL_INLINE_PREFIX", 1) != 0;
    const char *sk = getenv("SKL_SKETCH_KERNEL");
    k.sketch_global = sk && strcmp(sk, "global") == 0;
    // SKL_KERNEL = ksplit | kslice forces one implementation (0: dispatcher's choice)
    if (const char *e = getenv("SKL_KERNEL")) k.kernel = strcmp(e, "ksplit") == 0 ? 3 : strcmp(e, "kslice") == 0 ? 4 : 0;
    k.kslice_shape = (int)env_int("SKL_KSLICE_SHAPE", 0);
    k.ksplit_rows = (int)env_int("SKL_KSPLIT_ROWS", 0);
    k.kslice_ablate = (int)env_int("SKL_KSLICE_ABLATE", 0);
#endif
    return k;
}

#ifdef SKL_AB
int ab_forced_log_variant() { return (int)std::max(-2ll, std::min(1ll, env_int("SKL_FORCE_LOG_VARIANT", -2))); }   // -2: not forced
#endif

uint32_t ctx_xcd_shift(const skl_ctx *ctx) { return plan_xcd_shift(ctx->n_cu, ctx->knobs.xcds); }

int forced_kernel(const skl_ctx *ctx)
{
#ifdef SKL_AB
    // a forced tile shape or ablation counts as a forced kernel (no chunk slices, no mid-band rule)
    if (ctx->knobs.kernel == 0 && (ctx->knobs.kslice_shape || ctx->knobs.kslice_ablate)) return 4;
    return ctx->knobs.kernel;
#else
    (void)ctx;
    return 0;
#endif
}

// One launch of the pair kernel: which tile shape and form it takes is plan_pair_shape()'s answer (dense_plan.hpp); whether the
// chunk-split kernel takes the launch is the kernel's own knowledge (kslice_supported, pair_kslice.hip).
static hipError_t dispatch_pair_kernel(skl_ctx *ctx, const PairArgs &args_in, int mode, hipStream_t stream)
{
    PairArgs args = args_in;
    args.group_span = (uint32_t)ctx->knobs.group_span;
    args.xcd_shift = ctx_xcd_shift(ctx);
    args.inline_prefix_ok = ctx->knobs.inline_prefix ? 1u : 0u;
    PairLaunch a;
    a.mode = mode;
    a.self_mode = args.self_mode != 0;
    a.rows = args.row_end - args.row_begin;
    a.nB = args.nB;
    a.k_count = args.k_count;
    a.ss64 = args.ss64;
    a.k_sliced = args.k_sliced != 0;
    a.mid_band = args.mid_band != 0;
    a.tail_slices = args.tail_slices;
    a.xcd_interleave = args.xcd_interleave != 0;
    a.n_cu = ctx->n_cu;
    a.xcd_shift = args.xcd_shift;
    a.knobs = ctx->knobs;
#ifdef SKL_AB
    a.ab_build = true;
    a.ab_kernel = ctx->knobs.kernel;
    a.ab_kslice_shape = ctx->knobs.kslice_shape;
    a.ab_ksplit_rows = ctx->knobs.ksplit_rows;
    a.ab_kslice_ablate = ctx->knobs.kslice_ablate;
#endif
    const PairShape s = plan_pair_shape(a);
    args.no_half_tiles = s.no_half_tiles ? 1u : 0u;
    args.round_size = s.round_size;
    if (args.tail_slices > 1u) args.tail_resident = s.tail_resident;
    const bool kslice = s.try_kslice && kslice_supported(args, mode, s.sliced_launch);
    ctx->last_kernel = pair_kernel_name(s, kslice);
    args.tile_cost_order = args_in.tile_cost_order != 0u && s.tile_cost_order && kslice ? 1u : 0u;   // (asked for by the dense calls' counts launches alone)
    if (args.tile_cost_order) ctx->last_kernel += " [tiles dealt by cost, half tiles last]";
    if (kslice) return launch_pair_kernel_kslice(args, mode, s.shape, s.sliced_launch, s.ablate, ctx->tile_scratch, stream);
    return launch_pair_kernel_ksplit(args, mode, s.ksplit_rows, ctx->tile_scratch, stream);
}

// Launch the pair kernel bracketed by HIP events on the context's stream.
int timed_pair_launch(skl_ctx *ctx, const PairArgs &args, int mode)
{
    constexpr size_t MAX_EVENTS = 4096;
    // skl_ctx_timing_enable(N) / SKL_TIMING_EVERY = N brackets every N-th launch (default 0 = none: an event
    // record is a barrier packet on the queue, and two per launch cost a sub-millisecond launch ~5 us)
    const bool sampled = ctx->timing_every > 0 && (ctx->launches_seen++ % (size_t)ctx->timing_every) == 0;
    if (!sampled || ctx->events_used >= MAX_EVENTS) {
        HIP_TRY(dispatch_pair_kernel(ctx, args, mode, ctx->stream));
        return SKL_OK;
    }
    if (ctx->events_used == ctx->events.size()) {
        hipEvent_t a, b;
        HIP_TRY(hipEventCreate(&a));
        const hipError_t eb = hipEventCreate(&b);
        if (eb != hipSuccess) {
            (void)hipEventDestroy(a);
            return fail(SKL_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(eb));
        }
        ctx->events.emplace_back(a, b);
    }
    auto &ev = ctx->events[ctx->events_used++];
    HIP_TRY(hipEventRecord(ev.first, ctx->stream));
    HIP_TRY(dispatch_pair_kernel(ctx, args, mode, ctx->stream));
    HIP_TRY(hipEventRecord(ev.second, ctx->stream));
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

// ---------------------------------------------------------------------------
// the host libm's logarithm on the device (completeness path; glibc_log.hpp)
// ---------------------------------------------------------------------------

static double probe_uniform(uint64_t &state)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(state >> 11) * 0x1p-53;
}

int host_log_variant()
{
    static const int variant = [] {
#ifdef SKL_AB
        // A/B build only: SKL_FORCE_LOG_VARIANT=-1 | 0 | 1 takes the place of the probe (tests of the "neither form" branch)
        const int forced = ab_forced_log_variant();
        if (forced >= -1) return forced;
#endif
        // arguments of the kind the path takes logarithms of: Jaccard values in (0, 1], the
        // |x - 1| < 1/16 branch, and the values every k-mer length of a sketch size can give
        uint64_t st = 0x5EED0001ull;
        size_t bad[2] = {0, 0};
        auto check = [&](double x) {
            volatile double xv = x;   // a run-time call into libm, never folded
            const double ref = std::log(xv);
            for (int v = 0; v < 2; ++v) {
                if (skl_as_u64(glibc_log(x, v)) != skl_as_u64(ref)) ++bad[v];
            }
        };
        for (int i = 0; i < 150000; ++i) check(probe_uniform(st));
        for (int i = 0; i < 150000; ++i) check(0.9375 + 0.13 * probe_uniform(st));
        for (uint32_t b = 1; b <= 4096; ++b) check((double)b / 4096.0);
        if (bad[SKL_LOG_FMA] == 0) return (int)SKL_LOG_FMA;
        if (bad[SKL_LOG_SSE2] == 0) return (int)SKL_LOG_SSE2;
        return -1;   // reported through skl_ctx_flags() / skl_log_variant(); the caller decides what to print
    }();
    return variant;
}

extern "C" int skl_log_variant(void) { return host_log_variant(); }

extern "C" unsigned skl_ctx_flags(const skl_ctx *ctx)
{
    unsigned flags = 0;
    if (host_log_variant() < 0) flags |= SKL_CTX_FLAG_LOG_UNMATCHED;
    if (ctx && ctx->n_cu != 256) flags |= SKL_CTX_FLAG_NOT_SPX;
    return flags;
}

extern "C" int skl_device_log(skl_ctx *ctx, const double *x_host, size_t n, double *out_host)
{
    SKL_TRY(ctx_bind(ctx));
    if (n == 0) return SKL_OK;
    if (!x_host || !out_host) return fail(SKL_ERR_INVALID_ARG, "null argument");
    DevBuf dx, dy;
    HIP_TRY(hipMalloc(&dx.p, n * sizeof(double)));
    HIP_TRY(hipMalloc(&dy.p, n * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(dx.p, x_host, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const int v = host_log_variant();
    HIP_TRY(launch_device_log((const double *)dx.p, (double *)dy.p, n, v < 0 ? (int)SKL_LOG_FMA : v, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out_host, dy.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SKL_OK;
}

// ---------------------------------------------------------------------------
// sketch slabs
// ---------------------------------------------------------------------------


// jaccard.rs:14,26-33 with no completeness: J as a function of samebits alone.
static double host_jaccard(uint32_t samebits, size_t ss64)
{
    const double unionsize = (double)(64u * ss64);
    const uint32_t maxnbits = (uint32_t)ss64 * 64u;
    const uint32_t expected = maxnbits >> BBITS;
    const uint32_t diff = samebits > expected ? samebits - expected : 0u;
    const double intersize = ((double)diff * (double)maxnbits) / (double)(maxnbits - expected);
    return intersize / unionsize;
}

static int ensure_lanes(const skl_sketches *cs)
{
    skl_sketches *s = const_cast<skl_sketches *>(cs);
    if (s->d_lanes || s->n == 0) return SKL_OK;
    const size_t n_jb = (s->n + 63) / 64;
    const size_t bytes = n_jb * s->nk * s->ss64 * 7 * 64 * sizeof(uint4);
    HIP_TRY(hipMalloc((void **)&s->d_lanes, bytes));
    HIP_TRY(launch_relayout(s->d_rows, s->d_lanes, (uint32_t)s->n, (uint32_t)s->nk,
                            (uint32_t)s->ss64, s->ctx->stream));
    return SKL_OK;
}

static int ensure_ytab(const skl_sketches *cs)
{
    skl_sketches *s = const_cast<skl_sketches *>(cs);
    if (s->d_ytab) return SKL_OK;
    const size_t m = 64 * s->ss64 + 1;
    std::vector<double> tab(m);
    for (size_t b = 0; b < m; ++b) tab[b] = std::log(host_jaccard((uint32_t)b, s->ss64));
    {   // the break test of jaccard.rs:89-91 on the count itself: ln J(count) < tolerance <=> count < min_alive -- if the table is
        // monotone there (it is; checked, not assumed: 0xFFFFFFFF makes the kernels ask the table)
        const double tolerance = std::log(2.0 / (double)((s->ss64 * 64ull) * 64ull));
        size_t first = 0;
        while (first < m && tab[first] < tolerance) ++first;
        bool monotone = true;
        for (size_t b = first; b < m; ++b) monotone = monotone && !(tab[b] < tolerance);
        s->min_alive = monotone ? (uint32_t)first : 0xFFFFFFFFu;
    }
    double *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, m * sizeof(double)));
    const hipError_t e = hipMemcpy(d, tab.data(), m * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(SKL_ERR_HIP, "ln J table upload: %s", hipGetErrorString(e));
    }
    s->d_ytab = d;
    return SKL_OK;
}

static int ensure_dtab(const skl_sketches *cs, int jout, size_t k_idx, float **out)
{
    skl_sketches *s = const_cast<skl_sketches *>(cs);
    const size_t key_k = jout == JOUT_DIST ? 0 : k_idx;
    auto it = s->d_dtab.find({jout, key_k});
    if (it != s->d_dtab.end()) {
        *out = it->second;
        return SKL_OK;
    }
    const size_t m = 64 * s->ss64 + 1;
    const double k = (double)s->kmers[k_idx];
    std::vector<float> tab(m);
    for (size_t b = 0; b < m; ++b) {
        const double j = host_jaccard((uint32_t)b, s->ss64);
        if (jout == JOUT_DIST) {
            tab[b] = (float)(1.0 - j);  // mod.rs:99
        } else {
            // jaccard.rs:49-51
            const double ani = std::fmax(0.0, 1.0 + 1.0 / k * std::log((2.0 * j) / (1.0 + j)));
            tab[b] = jout == JOUT_ANI ? (float)ani : (float)(1.0 - ani);  // mod.rs:97 / :173-176
        }
    }
    float *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, m * sizeof(float)));
    const hipError_t e = hipMemcpy(d, tab.data(), m * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(SKL_ERR_HIP, "distance table upload: %s", hipGetErrorString(e));
    }
    s->d_dtab[{jout, key_k}] = d;
    *out = d;
    return SKL_OK;
}

// A slab of n_samples rows with nothing in them yet: registered, its pad rows zeroed (queued on the context's stream) and its
// k-mer table uploaded.  Rows [0, n_samples) are the caller's to fill on that stream (skl_sketches_create: a copy;
// capi_slab.cpp: a gather or two device copies); on an error the caller destroys *out.
int slab_alloc(skl_ctx *ctx, size_t n_samples, size_t nk, const size_t *kmers, size_t sketchsize64, skl_sketches **out)
{
    if (nk == 0 || sketchsize64 == 0 || !kmers) {
        return fail(SKL_ERR_INVALID_ARG, "need at least one k-mer length and a non-zero sketch size");
    }
    if (n_samples >= (1ull << 31) || sketchsize64 >= (1ull << 25) || nk >= (1ull << 16)) {
        return fail(SKL_ERR_INVALID_ARG, "dimensions out of range");
    }
    skl_sketches *s = new skl_sketches();
    s->ctx = ctx;
    s->gen = next_generation();
    {
        std::lock_guard<std::mutex> lock(g_registry_mutex);
        g_live_sketches.insert(s);
        ctx->sketches.insert(s);
    }
    s->n = n_samples;
    s->nk = nk;
    s->ss64 = sketchsize64;
    s->kmers.assign(kmers, kmers + nk);
    const size_t words = s->sample_words();
    const size_t total = (n_samples + A_PAD_ROWS) * words;
    hipError_t e = hipMalloc((void **)&s->d_rows, total * sizeof(uint64_t));
    if (e != hipSuccess) {
        skl_sketches_destroy(s);
        return fail(e == hipErrorOutOfMemory ? SKL_ERR_OOM : SKL_ERR_HIP, "hipMalloc(slab %zu B): %s",
                    total * sizeof(uint64_t), hipGetErrorString(e));
    }
    do {
        e = hipMemsetAsync(s->d_rows + n_samples * words, 0, A_PAD_ROWS * words * sizeof(uint64_t),
                           ctx->stream);
        if (e != hipSuccess) break;
        std::vector<double> kf(nk);
        for (size_t i = 0; i < nk; ++i) kf[i] = (double)kmers[i];
        e = hipMalloc((void **)&s->d_kf, nk * sizeof(double));
        if (e != hipSuccess) break;
        e = hipMemcpy(s->d_kf, kf.data(), nk * sizeof(double), hipMemcpyHostToDevice);
    } while (0);
    if (e != hipSuccess) {
        const int rc = fail(SKL_ERR_HIP, "slab upload: %s", hipGetErrorString(e));
        skl_sketches_destroy(s);
        return rc;
    }
    *out = s;
    return SKL_OK;
}

extern "C" int skl_sketches_create(skl_ctx *ctx, const uint64_t *bins, int on_device,
                                   size_t n_samples, size_t nk, const size_t *kmers,
                                   size_t sketchsize64, skl_sketches **out)
{
    SKL_TRY(ctx_bind(ctx));
    if (!out) return fail(SKL_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    if (nk == 0 || sketchsize64 == 0 || !kmers) {
        return fail(SKL_ERR_INVALID_ARG, "need at least one k-mer length and a non-zero sketch size");
    }
    if (n_samples && !bins) return fail(SKL_ERR_INVALID_ARG, "bins is null");
    skl_sketches *s = nullptr;
    SKL_TRY(slab_alloc(ctx, n_samples, nk, kmers, sketchsize64, &s));
    hipError_t e = hipSuccess;
    if (n_samples) {
        e = hipMemcpyAsync(s->d_rows, bins, n_samples * s->sample_words() * sizeof(uint64_t),
                           on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        const int rc = fail(SKL_ERR_HIP, "slab upload: %s", hipGetErrorString(e));
        skl_sketches_destroy(s);
        return rc;
    }
    *out = s;
    return SKL_OK;
}

extern "C" int skl_sketches_set_completeness(skl_sketches *s, const double *comp)
{
    if (!s) return fail(SKL_ERR_INVALID_ARG, "null sketches");
    SKL_TRY(ctx_bind(s->ctx));
    s->gen = next_generation();   // (a sampled early-break decision belongs to the slab AND its completeness vector)
    if (!comp) {
        if (s->d_comp) {
            HIP_TRY(hipStreamSynchronize(s->ctx->stream));
            HIP_TRY(hipFree(s->d_comp));
            s->d_comp = nullptr;
        }
        return SKL_OK;
    }
    if (!s->d_comp) {
        HIP_TRY(hipMalloc((void **)&s->d_comp, (s->n + A_PAD_ROWS + 64) * sizeof(double)));
        HIP_TRY(hipMemset(s->d_comp, 0, (s->n + A_PAD_ROWS + 64) * sizeof(double)));
    }
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    HIP_TRY(hipMemcpy(s->d_comp, comp, s->n * sizeof(double), hipMemcpyHostToDevice));
    s->comp_unit = true;
    for (size_t x = 0; x < s->n; ++x) {
        if (!(comp[x] > 0.0 && comp[x] <= 1.0)) {   // (NaN fails both)
            s->comp_unit = false;
            break;
        }
    }
    return SKL_OK;
}

static void free_sketches_locked(skl_sketches *s)
{
    if (!g_live_sketches.erase(s)) return;
    s->ctx->sketches.erase(s);
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    if (s->d_rows) (void)hipFree(s->d_rows);
    if (s->d_lanes) (void)hipFree(s->d_lanes);
    if (s->d_comp) (void)hipFree(s->d_comp);
    if (s->d_ytab) (void)hipFree(s->d_ytab);
    if (s->d_kf) (void)hipFree(s->d_kf);
    for (auto &kv : s->d_dtab) (void)hipFree(kv.second);
    delete s;
}

extern "C" int skl_sketches_destroy(skl_sketches *s)
{
    if (!s) return SKL_OK;
    std::lock_guard<std::mutex> lock(g_registry_mutex);
    free_sketches_locked(s);  // no-op if the handle (or its context) is already gone
    return SKL_OK;
}

extern "C" size_t skl_sketches_n_samples(const skl_sketches *s) { return s ? s->n : 0; }

// mod.rs:25-37
extern "C" int skl_set_k(const skl_sketches *s, size_t kmer, int ani, double cutoff,
                         skl_dist_params *out)
{
    if (!s || !out) return fail(SKL_ERR_INVALID_ARG, "null argument");
    out->completeness_cutoff = cutoff;
    out->k_idx = 0;
    out->ani = 0;
    if (kmer == 0) {
        out->dist_type = SKL_DIST_COREACC;
        return SKL_OK;
    }
    for (size_t i = 0; i < s->nk; ++i) {
        if (s->kmers[i] == kmer) {
            out->dist_type = SKL_DIST_JACCARD;
            out->k_idx = i;
            out->ani = ani ? 1 : 0;
            return SKL_OK;
        }
    }
    return fail(SKL_ERR_KMER_NOT_FOUND, "K-mer size %zu not found in file", kmer);
}

// ---------------------------------------------------------------------------
// shared launch preparation
// ---------------------------------------------------------------------------

int check_params(const skl_sketches *a, const skl_sketches *b, const skl_dist_params *p)
{
    if (!a || !b || !p) return fail(SKL_ERR_INVALID_ARG, "null argument");
    if (a->ctx != b->ctx) return fail(SKL_ERR_INVALID_ARG, "sketches belong to different contexts");
    if (a->nk != b->nk || a->ss64 != b->ss64 || a->kmers != b->kmers) {
        // MultiSketch::is_compatible_with, multisketch.rs:222-226
        return fail(SKL_ERR_INCOMPATIBLE, "reference and query sketches are not compatible (k-mer lengths / sketch size differ)");
    }
    if (p->dist_type == SKL_DIST_COREACC) {
        if (a->nk < 2) {
            return fail(SKL_ERR_KMER_COUNT,
                        "Need at least two k-mer lengths to calculate core/accessory distances");
        }
    } else if (p->dist_type == SKL_DIST_JACCARD) {
        if (p->k_idx >= a->nk) return fail(SKL_ERR_INVALID_ARG, "k_idx %llu out of range", (unsigned long long)p->k_idx);
    } else {
        return fail(SKL_ERR_INVALID_ARG, "unknown dist_type %d", p->dist_type);
    }
    return SKL_OK;
}

bool fused_coreacc_ok(const skl_sketches *s)
{
    return s->nk <= (size_t)MAX_FUSED_K && 64 * s->ss64 <= 0xFFFFu;
}

// Fill the operand / epilogue fields common to every launch.  `rows` is the scalar
// operand (A), `cols` the lane operand (B).
int fill_args(const skl_sketches *rows, const skl_sketches *cols, const skl_dist_params *p,
                     int mode, int jout, PairArgs *g)
{
    SKL_TRY(ensure_lanes(cols));
    return fill_args_ref_layout(rows, cols, p, mode, jout, g);
}

// ... for the kernels that read BOTH sides in the reference layout (pair_list.hip): the lane-layout copy of `cols` is not
// made; g->B is whatever the slab already has (possibly null)
int fill_args_ref_layout(const skl_sketches *rows, const skl_sketches *cols, const skl_dist_params *p,
                         int mode, int jout, PairArgs *g)
{
    memset(g, 0, sizeof *g);
    g->A = rows->d_rows;
    g->B = cols->d_lanes;
    g->nA = (uint32_t)rows->n;
    g->nB = (uint32_t)cols->n;
    g->nk = (uint32_t)rows->nk;
    g->ss64 = (uint32_t)rows->ss64;
    g->has_comp = (rows->d_comp && cols->d_comp) ? 1 : 0;  // both Some, jaccard.rs:36
    if (g->has_comp) {
        const int v = host_log_variant();
        g->log_variant = v < 0 ? (int)SKL_LOG_FMA : v;
    }
    g->compA = rows->d_comp;
    g->compB = cols->d_comp;
    g->cutoff = p ? p->completeness_cutoff : 0.0;
    g->tolerance = std::log(2.0 / (double)((rows->ss64 * 64ull) * 64ull));  // jaccard.rs:75
    g->jout = jout;
    if (mode == MODE_COUNTS) {
        g->k_begin = 0;
        g->k_count = (uint32_t)rows->nk;
        g->cnt_pair_stride = rows->nk;   // [pair][k] records
        g->cnt_k_stride = 1;
    } else if (mode == MODE_JACCARD) {
        g->k_begin = (uint32_t)p->k_idx;
        g->k_count = 1;
        g->kf[0] = (double)rows->kmers[p->k_idx];
        if (!g->has_comp) {
            float *d = nullptr;
            SKL_TRY(ensure_dtab(rows, jout, p->k_idx, &d));
            g->dtab = d;
        }
    } else {
        g->k_begin = 0;
        g->k_count = (uint32_t)rows->nk;
        for (size_t i = 0; i < rows->nk && i < (size_t)MAX_FUSED_K; ++i) g->kf[i] = (double)rows->kmers[i];
        SKL_TRY(ensure_ytab(rows));
        g->ytab = rows->d_ytab;
    }
    return SKL_OK;
}

static std::atomic<uint64_t> g_next_gen{1};
uint64_t next_generation() { return g_next_gen.fetch_add(1); }

static void free_plan(EbPlan *p)
{
    if (!p) return;
    if (p->d_block_ke) (void)hipFree(p->d_block_ke);
    delete p;
}
struct EbPlanFree {
    void operator()(EbPlan *p) const { free_plan(p); }
};

void free_plans(skl_ctx *ctx)
{
    for (EbPlan *p : ctx->eb_plans) free_plan(p);
    ctx->eb_plans.clear();
    ctx->eb_last_plan = nullptr;
}

// The early break's sample: `g.samples` pairs of every block run the reference's loop on the device; *hist = [block][EB_HIST]
// pairs that pass the test at exactly their first m lengths.
static int eb_sample(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, double cutoff, const EbGeometry &g, std::vector<uint32_t> *hist)
{
    const bool has_comp = rows->d_comp != nullptr && cols->d_comp != nullptr;
    SKL_TRY(ensure_ytab(rows));
    DevBuf d_hist;
    hist->assign((size_t)g.n_blocks() * EB_HIST, 0u);
    HIP_TRY(hipMalloc(&d_hist.p, hist->size() * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(d_hist.p, 0, hist->size() * sizeof(uint32_t), ctx->stream));
    EbSampleArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.rows_ref = rows->d_rows;
    sa.cols_ref = cols->d_rows;
    sa.n_rows = (uint32_t)rows->n;
    sa.n_cols = (uint32_t)cols->n;
    sa.nk = (uint32_t)rows->nk;
    sa.ss64 = (uint32_t)rows->ss64;
    sa.self_mode = g.self_mode ? 1u : 0u;
    sa.samples = g.samples;
    sa.blk_shift_r = g.shift_r;
    sa.blk_shift_c = g.shift_c;
    sa.blk_rows = g.blk_rows;
    sa.blk_cols = g.blk_cols;
    sa.min_alive = rows->min_alive;
    sa.has_comp = has_comp ? 1 : 0;
    if (has_comp) {
        const int v = host_log_variant();
        sa.log_variant = v < 0 ? (int)SKL_LOG_FMA : v;
    }
    sa.ytab = rows->d_ytab;
    sa.compA = rows->d_comp;
    sa.compB = cols->d_comp;
    sa.cutoff = cutoff;
    sa.tolerance = std::log(2.0 / (double)((rows->ss64 * 64ull) * 64ull));  // jaccard.rs:75
    sa.hist = (uint32_t *)d_hist.p;
    HIP_TRY(launch_early_break_sample(sa, ctx->stream));
    HIP_TRY(hipMemcpyAsync(hist->data(), d_hist.p, hist->size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SKL_OK;
}

// The decision for a slab pair (eb_plan.hpp): applicable? -> kept from an earlier call? -> forced, or sampled and decided -> kept.
int early_break_plan(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, int self_mode, double cutoff, const EbPlan **out)
{
    *out = nullptr;
    const int knob = ctx->knobs.early_break;
    if (!eb_applicable(knob, rows->nk, rows->n, cols->n)) return SKL_OK;
    if (!ctx->eb_counter) {
        HIP_TRY(hipMalloc((void **)&ctx->eb_counter, 1024 * sizeof(uint32_t)));   // 1 024 counter slots (diagnostic)
        HIP_TRY(hipMemsetAsync(ctx->eb_counter, 0, 1024 * sizeof(uint32_t), ctx->stream));
    }
    const bool has_comp = rows->d_comp != nullptr && cols->d_comp != nullptr;
    for (const EbPlan *p : ctx->eb_plans) {
        if (p->rows_gen == rows->gen && p->cols_gen == cols->gen && p->self_mode == self_mode && p->knob == knob && (!has_comp || p->cutoff == cutoff)) {
            *out = p;
            return SKL_OK;
        }
    }
    EbGeometry geo;
    EbDecision decision;
    if (knob >= 2) {
        decision = eb_forced(knob, rows->nk);
    } else {
        geo = eb_geometry(rows->n, cols->n, self_mode != 0);
        std::vector<uint32_t> hist;
        SKL_TRY(eb_sample(ctx, rows, cols, cutoff, geo, &hist));
        decision = eb_decide(geo, rows->nk, eb_cost((uint32_t)rows->ss64, rows->n, cols->n, self_mode != 0), hist.data());
    }
    // (owned here until it is kept: an upload that fails takes the plan and its table with it)
    std::unique_ptr<EbPlan, EbPlanFree> plan(new EbPlan());
    plan->rows_gen = rows->gen;
    plan->cols_gen = cols->gen;
    plan->self_mode = self_mode;
    plan->cutoff = cutoff;
    plan->knob = knob;
    plan->geo = geo;
    plan->decision = std::move(decision);
    if (plan->decision.mixed) {
        const std::vector<uint8_t> &ke = plan->decision.block_ke;
        HIP_TRY(hipMalloc((void **)&plan->d_block_ke, ke.size()));
        HIP_TRY(hipMemcpy(plan->d_block_ke, ke.data(), ke.size(), hipMemcpyHostToDevice));
    }
    if (ctx->eb_plans.size() >= EB_PLANS_KEPT) {
        // (nothing in flight may still read the oldest plan's table: the streams are drained before it goes)
        if (ctx->eb_plans.front()->d_block_ke != nullptr) {
            (void)hipStreamSynchronize(ctx->stream);
            if (ctx->epi_stream) (void)hipStreamSynchronize(ctx->epi_stream);
        }
        if (ctx->eb_last_plan == ctx->eb_plans.front()) ctx->eb_last_plan = nullptr;
        free_plan(ctx->eb_plans.front());
        ctx->eb_plans.erase(ctx->eb_plans.begin());
    }
    ctx->eb_plans.push_back(plan.get());
    *out = plan.release();
    return SKL_OK;
}

int early_break_lengths(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, int self_mode, int *lengths)
{
    *lengths = 0;
    // (the kNN bands' epilogue has no completeness branch and no segmented counts: capi_knn.cpp)
    if (rows->d_comp != nullptr || cols->d_comp != nullptr || rows->ss64 > (size_t)KSLICE_MAX_U16_CHUNKS) return SKL_OK;
    const EbPlan *plan = nullptr;
    SKL_TRY(early_break_plan(ctx, rows, cols, self_mode, 0.0, &plan));
    if (plan) *lengths = plan->decision.lengths;
    return SKL_OK;
}

extern "C" int skl_ctx_early_break_blocks(skl_ctx *ctx, uint32_t *blk_rows, uint32_t *blk_cols, uint32_t *shift_rows, uint32_t *shift_cols,
                                          int *pooled_lengths, int *mixed, uint8_t *block_lengths, size_t capacity)
{
    SKL_TRY(ctx_bind(ctx));
    const EbPlan *p = ctx->eb_last_plan;
    if (blk_rows) *blk_rows = p ? p->geo.blk_rows : 0u;
    if (blk_cols) *blk_cols = p ? p->geo.blk_cols : 0u;
    if (shift_rows) *shift_rows = p ? p->geo.shift_r : 0u;
    if (shift_cols) *shift_cols = p ? p->geo.shift_c : 0u;
    if (pooled_lengths) *pooled_lengths = p ? p->decision.lengths : 0;
    if (mixed) *mixed = p && p->decision.mixed ? 1 : 0;
    if (p && p->decision.mixed && block_lengths) {
        const std::vector<uint8_t> &ke = p->decision.block_ke;
        if (capacity < ke.size()) return fail(SKL_ERR_INVALID_ARG, "skl_ctx_early_break_blocks: %zu blocks, room for %zu", ke.size(), capacity);
        memcpy(block_lengths, ke.data(), ke.size());
    }
    return SKL_OK;
}

static_assert(PLAN_MODE_COUNTS == MODE_COUNTS && PLAN_MODE_JACCARD == MODE_JACCARD && PLAN_MODE_COREACC == MODE_COREACC &&
              PLAN_MAX_U16_CHUNKS == (uint32_t)KSLICE_MAX_U16_CHUNKS && PLAN_SEG_CHUNKS == (uint32_t)KSLICE_SEG_CHUNKS,
              "dense_plan.hpp restates these constants of kernels.h");

// Which counts buffer a band's launch uses, and whether its epilogue runs on the second stream beside the next band's counts kernel.
struct BandSlot {
    int buf = 0;
    bool overlapped = false;
};

// rows [r0, r1) of the call into `out`
static void set_rows(PairArgs *g, const DenseCall &c, uint64_t r0, uint64_t r1, void *out)
{
    g->row_begin = (uint32_t)r0;
    g->row_end = (uint32_t)r1;
    g->self_mode = c.self_mode ? 1 : 0;
    g->out_base = c.out_base(r0);
    g->out = out;
}

// PLANE 1 of the counts scratch, which the tail slices ADD into: all zero on entry, re-zeroed by the epilogue.  The context
// remembers the one (pointer, bytes) it knows to be zero.  Before the pair launch: zero `plane1` unless it is that one (null: this
// launch writes the scratch in another layout), and mark it dirty -- it holds partial counts from the pair launch on ...
static int plane1_before_launch(skl_ctx *ctx, void *plane1, size_t bytes)
{
    if (plane1 && (ctx->clean_plane1 != plane1 || ctx->clean_plane1_bytes != bytes)) HIP_TRY(hipMemsetAsync(plane1, 0, bytes, ctx->stream));
    ctx->clean_plane1 = nullptr;
    return SKL_OK;
}
// ... and is "clean" again only once the epilogue that re-zeroes it is enqueued.  Any early return in between leaves it marked dirty.
static void plane1_after_epilogue(skl_ctx *ctx, void *plane1, size_t bytes)
{
    ctx->clean_plane1 = plane1;
    ctx->clean_plane1_bytes = bytes;
}

// The epilogue fields both counts forms set: where launch `g` left its counts, which pairs they are, where the output goes.
static void fill_epilogue(EpilogueArgs *e, const skl_sketches *rows, const skl_sketches *cols, const skl_dist_params *p, const PairArgs &g,
                          const CountsLaunch &L, void *dst)
{
    memset(e, 0, sizeof *e);
    e->counts = (uint32_t *)g.out;
    e->pair_stride = g.cnt_pair_stride;
    e->k_stride = g.cnt_k_stride;
    e->n_pairs = L.pairs;
    e->nk = L.lengths;
    e->ss64 = (uint32_t)rows->ss64;
    e->n_slices = L.two_planes ? 2u : L.k_slices;
    e->rezero_plane1 = L.tail ? 1u : 0u;
    e->nA_rows = (uint32_t)rows->n;
    e->nB_cols = (uint32_t)cols->n;
    e->row_begin = g.row_begin;
    e->self_mode = g.self_mode;
    e->n_total = (uint32_t)cols->n;
    e->out_base = g.out_base;
    e->has_comp = g.has_comp;
    e->log_variant = g.log_variant;
    e->compA = rows->d_comp;
    e->compB = cols->d_comp;
    e->cutoff = p->completeness_cutoff;
    e->out = (float *)dst;
}

// Core/accessory, unfused: counts -> scratch -> epilogue kernel.
static int run_counts_epilogue(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, const skl_dist_params *p, const DenseCall &c,
                               const EbPlan *plan, const CountsLaunch &L, uint64_t r0, uint64_t r1, BandSlot slot, void *dst_dev)
{
    // (a stream of its own: the banded host output copies band i back on aux_stream while band i + 1 is computed, and must not
    // queue behind that band's epilogues)
    if (slot.overlapped && !ctx->epi_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->epi_stream, hipStreamNonBlocking));
    hipStream_t epi_stream = slot.overlapped ? ctx->epi_stream : ctx->stream;
    PairArgs g;
    SKL_TRY(fill_args(rows, cols, p, MODE_COUNTS, 0, &g));
    if (L.early) {
        g.k_count = L.lengths;
        g.cnt_pair_stride = L.lengths;
    }
    if (L.mixed) {
        g.xcd_interleave = 1;
        g.block_ke = plan->d_block_ke;
        g.blk_shift_r = plan->geo.shift_r;
        g.blk_shift_c = plan->geo.shift_c;
        g.blk_cols = plan->geo.blk_cols;
    }
    void *counts = nullptr;
    SKL_TRY(ctx_scratch(ctx, L.plane_bytes * L.planes, &counts, slot.overlapped && slot.buf ? SCRATCH_COUNTS_2 : SCRATCH_COUNTS));
    g.cnt_u16 = L.cnt_u16 ? 1u : 0u;
    if (L.sliced) {   // k-major scratch: coalesced stores from the (tile, k[, chunk slice]) workgroups
        g.cnt_pair_stride = 1;
        g.cnt_k_stride = L.pairs;
        g.k_sliced = 1;
        g.k_slices = L.k_slices;
        g.tail_slices = L.tail_slices;
        g.slice_chunks = L.slice_chunks;
        g.mid_band = L.mid_band ? 1u : 0u;
    }
    g.tile_cost_order = 1;   // (a request: plan_pair_shape decides)
    set_rows(&g, c, r0, r1, counts);
    SKL_TRY(ensure_ytab(rows));   // (before the pair launch: nothing may fail between it and the epilogue)
    // FUSED EPILOGUE (round 5): a plain k-sliced launch -- one workgroup per (tile, k-mer length), no chunk slices -- finishes
    // its pairs itself: the workgroup that completes a tile's k-mer lengths reads the tile's counts back and stores (core, acc)
    // (pair_kslice.hip, FUSE).  The second launch (10 us at cfg 2, 6 of them the cost of any dependent launch) is gone.
    bool fused = false;
#ifdef SKL_AB
    // (A/B build only, SKL_FUSE_EPILOGUE=1: measured SLOWER than the second launch at cfg 2 -- 0.154 against 0.145 ms per step:
    // the arrival pattern itself is free, but with the k-major dispatch order every tile completes in the launch's last round
    // and one workgroup then does a whole tile's regressions alone while the chip empties; profiles/r05_fused_epilogue.md)
    if (L.fuse_epilogue && rows->nk <= (size_t)MAX_FUSED_K && kslice_supported(g, MODE_COUNTS, true)) {
        // arrival counters, one per tile of the launch (16-row tiles at most), counted modulo nk: zero once per (buffer, nk)
        const size_t tiles_max = ((r1 - r0 + 15) / 16 + 1) * ((cols->n + 127) / 128 + 1) + 64;
        void *fc = nullptr;
        const size_t had = ctx->scratch_bytes[SCRATCH_FUSE_COUNTERS];
        SKL_TRY(ctx_scratch(ctx, tiles_max * sizeof(uint32_t), &fc, SCRATCH_FUSE_COUNTERS));
        if (ctx->scratch_bytes[SCRATCH_FUSE_COUNTERS] != had || ctx->fuse_counter_k != rows->nk) {
            HIP_TRY(hipMemsetAsync(fc, 0, ctx->scratch_bytes[SCRATCH_FUSE_COUNTERS], ctx->stream));
            ctx->fuse_counter_k = rows->nk;
        }
        g.fuse_counter = (uint32_t *)fc;
        g.fuse_variant = (uint32_t)env_int("SKL_FUSE_VARIANT", 0);
        g.fuse_out = (float *)dst_dev;
        g.ytab = rows->d_ytab;
        for (size_t t = 0; t < rows->nk; ++t) g.kf[t] = (double)rows->kmers[t];
        g.cutoff = p->completeness_cutoff;
        fused = true;
    }
#endif
    void *const plane1 = L.two_planes ? (char *)counts + L.plane_bytes : nullptr;
    SKL_TRY(plane1_before_launch(ctx, plane1, L.plane_bytes));
    SKL_TRY(timed_pair_launch(ctx, g, MODE_COUNTS));
    if (fused) {
        ctx->last_kernel += " + fused core/accessory epilogue (last workgroup of a tile)";
        return SKL_OK;
    }
    EpilogueArgs e;
    fill_epilogue(&e, rows, cols, p, g, L, dst_dev);
    e.nk_total = (uint32_t)rows->nk;
    if (L.early) {
        e.rows_ref = rows->d_rows;
        e.cols_ref = cols->d_rows;
        e.alive_count = ctx->eb_counter;
        ctx->eb_pairs += L.pairs;
        if (L.mixed) {
            e.block_ke = plan->d_block_ke;
            e.blk_shift_r = plan->geo.shift_r;
            e.blk_shift_c = plan->geo.shift_c;
            e.blk_cols = plan->geo.blk_cols;
            ctx->last_kernel += " + early break: block by block (" + std::to_string(plan->geo.blk_rows) + " x " + std::to_string(plan->geo.blk_cols) + " blocks of sample ids), the pairs still in the running completed by the epilogue";
        } else {
            ctx->last_kernel += " + early break: " + std::to_string(L.lengths) + " of " + std::to_string(rows->nk) + " k-mer lengths counted, the pairs still in the running completed by the epilogue";
        }
    }
    e.min_alive = rows->min_alive;
    e.cnt_u16 = g.cnt_u16;
    e.row_end = (uint32_t)r1;
    e.xcd_shift = ctx_xcd_shift(ctx);
    e.blocked = L.blocked ? 1u : 0u;
    e.blk_row_shift = (uint32_t)ctx->knobs.eb_blk_row_shift;
    if (e.blocked) ctx->last_kernel += " (epilogue in blocks of 1 024 x 256 pairs per XCD)";
    e.ahead = L.ahead ? 1u : 0u;
    e.lean = L.lean ? 1u : 0u;
    e.comp_lean = L.comp_lean ? 1u : 0u;
    e.lds_rows = L.lds_rows ? 1u : 0u;
    e.striped = L.striped ? 1u : 0u;
    e.ytab = rows->d_ytab;
    e.tolerance = g.tolerance;
    e.kf = rows->d_kf;
    if (slot.overlapped) {   // this band's epilogue on the second stream, behind its counts kernel
        HIP_TRY(hipEventRecord(ctx->eb_events[slot.buf], ctx->stream));
        HIP_TRY(hipStreamWaitEvent(epi_stream, ctx->eb_events[slot.buf], 0));
    }
#ifdef SKL_AB
    if (L.epilogue_r5) {
        if (!L.early) e.nk_total = 0;
        HIP_TRY(launch_coreacc_epilogue(e, epi_stream));   // round 5's epilogue: alive pairs completed where they are found (A/B timing)
    } else
#endif
    {
        if (coreacc_epilogue_is_lean(e)) ctx->last_kernel += e.cnt_u16 ? " [lean epilogue]" : " [lean epilogue, sliced counts]";
        if (coreacc_epilogue_stages_rows(e)) ctx->last_kernel += " [row slices staged in LDS]";
        if (coreacc_epilogue_is_striped(e)) ctx->last_kernel += " [column stripes folded onto the XCDs]";
        HIP_TRY(launch_coreacc_epilogue_r6(e, epi_stream));
    }
    if (slot.overlapped) HIP_TRY(hipEventRecord(ctx->eb_events[2 + slot.buf], epi_stream));
    if (plane1) plane1_after_epilogue(ctx, plane1, L.plane_bytes);
    return SKL_OK;
}

// Single k, smaller than the chip: bin-match counts in tail slices per tile + an epilogue launch that turns the summed counts
// into the f32 output (dense_plan.hpp tail_slicing).
static int run_single_k_tail(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, const skl_dist_params *p, const DenseCall &c,
                             const CountsLaunch &L, int jout, uint64_t r0, uint64_t r1, void *dst_dev)
{
    PairArgs g;
    SKL_TRY(fill_args(rows, cols, p, MODE_JACCARD, jout, &g));
    void *counts = nullptr;
    SKL_TRY(ctx_scratch(ctx, L.plane_bytes * L.planes, &counts, SCRATCH_COUNTS));
    g.cnt_pair_stride = 1;
    g.cnt_k_stride = L.pairs;
    g.k_sliced = 1;
    g.k_slices = 1;
    g.tail_slices = L.tail_slices;
    g.slice_chunks = L.slice_chunks;
    set_rows(&g, c, r0, r1, counts);
    void *const plane1 = (char *)counts + L.plane_bytes;
    SKL_TRY(plane1_before_launch(ctx, plane1, L.plane_bytes));
    SKL_TRY(timed_pair_launch(ctx, g, MODE_COUNTS));
    EpilogueArgs e;
    fill_epilogue(&e, rows, cols, p, g, L, dst_dev);
    e.jaccard_out = 1;
    e.jout = jout;
    e.kf0 = g.kf[0];
    e.dtab = g.dtab;
    HIP_TRY(launch_coreacc_epilogue(e, ctx->stream));
    plane1_after_epilogue(ctx, plane1, L.plane_bytes);
    return SKL_OK;
}

// One launch of the mode's own kernel: fused all-k core/accessory, single k, bin-match counts.
static int run_direct(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, const skl_dist_params *p, const DenseCall &c, int jout,
                      uint64_t r0, uint64_t r1, void *dst_dev)
{
    PairArgs g;
    SKL_TRY(fill_args(rows, cols, p, c.mode, jout, &g));
    g.tile_cost_order = 1;   // (a request: plan_pair_shape takes it for bin-match counts in self mode)
    set_rows(&g, c, r0, r1, dst_dev);
    return timed_pair_launch(ctx, g, c.mode);
}

static const char *dense_range_name(int mode)
{
    return mode == MODE_COREACC ? "skl:dense_band core/accessory" : mode == MODE_JACCARD ? "skl:dense_band single k" : "skl:dense_band bin-match counts";
}

// Core of every dense call: rows [r0, r1) of the pair space into `dst` (device).  HOW it is launched -- the form, the
// counts' width, slices and planes, the epilogue's order, the row bands -- is decided in dense_plan.hpp; here the decision's
// input is gathered and its answer executed, band by band.
int dense_band(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols,
                      const skl_dist_params *p, int mode, int jout, int self_mode, uint64_t r0,
                      uint64_t r1, void *dst_dev)
{
    DenseCall c;
    c.mode = mode;
    c.self_mode = self_mode != 0;
    c.n_cols = cols->n;
    c.r0 = r0;
    c.r1 = r1;
    if (c.pairs(r0, r1) == 0) return SKL_OK;
    const RoctxRange range_(dense_range_name(mode));
    c.nk = (uint32_t)rows->nk;
    c.ss64 = (uint32_t)rows->ss64;
    c.has_comp = rows->d_comp && cols->d_comp;
    c.comp_unit = rows->comp_unit && cols->comp_unit;
    c.n_cu = ctx->n_cu;
    c.forced_kernel = forced_kernel(ctx);
    c.fused_coreacc_ok = fused_coreacc_ok(rows);
    c.knobs = ctx->knobs;
    const EbPlan *plan = nullptr;
    if (mode == MODE_COREACC && (c.forced_kernel == 0 || c.forced_kernel == 4)) {
        SKL_TRY(early_break_plan(ctx, rows, cols, self_mode, p ? p->completeness_cutoff : 0.0, &plan));
        ctx->eb_last_plan = plan;
    }
    if (plan) {
        c.eb_plan = true;
        c.eb_lengths = plan->decision.lengths;
        c.eb_mixed = plan->decision.mixed;
        c.eb_alive_share = plan->decision.alive_share;
        if (plan->decision.mixed || plan->decision.lengths > 0) SKL_TRY(ensure_ytab(rows));   // (min_alive, which the rules read, is set with the table)
    }
    c.min_alive = rows->min_alive;

    const RowBands bands = plan_row_bands(c);
    const size_t n_bands = bands.cuts.size() - 1;
    if (bands.overlap && !ctx->eb_events[0]) {
        for (auto &ev : ctx->eb_events) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    int rc = SKL_OK;
    for (size_t b = 0; b < n_bands && rc == SKL_OK; ++b) {
        std::optional<RoctxRange> band_range_;   // (a banded call: one range per band inside the call's)
        if (n_bands > 1) band_range_.emplace(dense_range_name(mode));
        const BandSlot slot = {bands.overlap ? (int)(b & 1) : 0, bands.overlap};
        // (the epilogue that read this counts buffer two bands ago must be done before the counts kernel rewrites it)
        if (bands.overlap && b >= 2) {
            const hipError_t e = hipStreamWaitEvent(ctx->stream, ctx->eb_events[2 + slot.buf], 0);
            if (e != hipSuccess) rc = fail(SKL_ERR_HIP, "hipStreamWaitEvent: %s", hipGetErrorString(e));
        }
        if (rc != SKL_OK) break;
        const uint64_t b0 = bands.cuts[b], b1 = bands.cuts[b + 1];
        void *dst = (char *)dst_dev + (c.out_base(b0) - c.out_base(r0)) * 2 * sizeof(float);   // (only core/accessory calls are cut: (core, acc) records)
        const CountsLaunch L = plan_counts_launch(c, b0, b1);
        if (L.form == FORM_COUNTS_EPILOGUE) rc = run_counts_epilogue(ctx, rows, cols, p, c, plan, L, b0, b1, slot, dst);
        else if (L.form == FORM_SINGLE_K_TAIL) rc = run_single_k_tail(ctx, rows, cols, p, c, L, jout, b0, b1, dst);
        else rc = run_direct(ctx, rows, cols, p, c, jout, b0, b1, dst);
    }
    if (bands.overlap) {   // the output belongs to the context's stream again
        for (int buf = 0; buf < 2; ++buf) {
            const hipError_t e = hipStreamWaitEvent(ctx->stream, ctx->eb_events[2 + buf], 0);
            if (e != hipSuccess && rc == SKL_OK) rc = fail(SKL_ERR_HIP, "hipStreamWaitEvent: %s", hipGetErrorString(e));
        }
        if (rc == SKL_OK) ctx->last_kernel += "; " + std::to_string(n_bands) + " row bands, each band's epilogue beside the next band's counts kernel";
    }
    return rc;
}

static size_t record_bytes(const skl_sketches *s, int mode)
{
    if (mode == MODE_COUNTS) return s->nk * sizeof(uint32_t);
    return mode == MODE_COREACC ? 2 * sizeof(float) : sizeof(float);
}

// Dense driver: whole row range either straight into a device destination, or banded
// through scratch and copied back to a host destination.
static int dense_rows(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols,
                      const skl_dist_params *p, int mode, int jout, int self_mode, uint64_t r0,
                      uint64_t r1, void *out, int out_on_device)
{
    SKL_TRY(ctx_bind(ctx));
    if (!out) return fail(SKL_ERR_INVALID_ARG, "out is null");
    const uint64_t n_cols = cols->n;
    const uint64_t row_limit = self_mode ? (n_cols ? n_cols - 1 : 0) : rows->n;
    if (r0 > r1 || r1 > (self_mode ? n_cols : rows->n)) {
        return fail(SKL_ERR_INVALID_ARG, "row range [%llu, %llu) out of bounds", (unsigned long long)r0,
                    (unsigned long long)r1);
    }
    r1 = std::min<uint64_t>(r1, row_limit);
    if (r1 <= r0 || n_cols == 0) return SKL_OK;
    const size_t rec = record_bytes(rows, mode);
    if (out_on_device) {
        return dense_band(ctx, rows, cols, p, mode, jout, self_mode, r0, r1, out);
    }
    // host destination: the bands of plan_host_bands() (dense_plan.hpp) through two device buffers -- band i is
    // copied back on the auxiliary stream while band i + 1 is computed
    const HostBands plan = plan_host_bands(self_mode != 0, n_cols, r0, r1, rec, BAND_BYTES);
    const uint64_t first = self_mode ? cond_index(r0, r0 + 1, n_cols) : r0 * n_cols;
    void *dev[2] = {nullptr, nullptr};
    SKL_TRY(ctx_scratch(ctx, plan.band_alloc, &dev[0], SCRATCH_KEY_BAND));
    SKL_TRY(ctx_scratch(ctx, plan.second_alloc, &dev[1], SCRATCH_KEY_BAND_2));
    // A copy into pageable host memory does not return before it is done (the runtime stages it), so the copy of band i is
    // ISSUED after band i + 1's kernels are in the queue: the host blocks in the copy while the device computes.
    struct PendingCopy {
        void *dst = nullptr;
        const void *src = nullptr;
        size_t bytes = 0;
        int buf = 0;
    } pending;
    auto issue_copy = [&](const PendingCopy &c) -> int {
        HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ctx->knn_pair_done[c.buf], 0));
        HIP_TRY(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, ctx->aux_stream));
        HIP_TRY(hipEventRecord(ctx->knn_topk_done[c.buf], ctx->aux_stream));
        return SKL_OK;
    };
    for (size_t it = 0; it < plan.bands.size(); ++it) {
        const HostBand &b = plan.bands[it];
        if (b.own_buffer) {   // a single row wider than a band: its own buffer
            if (pending.bytes) {
                SKL_TRY(issue_copy(pending));
                pending.bytes = 0;
            }
            HIP_TRY(hipStreamSynchronize(ctx->aux_stream));
            SKL_TRY(ctx_scratch(ctx, b.pairs * rec, &dev[b.buf], b.buf == 0 ? SCRATCH_KEY_BAND : SCRATCH_KEY_BAND_2));
        }
        void *band = dev[b.buf];
        // the copy that read this buffer two bands ago must be done before it is overwritten
        if (it >= 2) HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->knn_topk_done[b.buf], 0));
        SKL_TRY(dense_band(ctx, rows, cols, p, mode, jout, self_mode, b.r0, b.r1, band));
        HIP_TRY(hipEventRecord(ctx->knn_pair_done[b.buf], ctx->stream));
        if (pending.bytes) SKL_TRY(issue_copy(pending));   // the previous band's, behind this band's kernels
        const uint64_t off = (self_mode ? cond_index(b.r0, b.r0 + 1, n_cols) : b.r0 * n_cols) - first;
        pending.dst = (char *)out + off * rec;
        pending.src = band;
        pending.bytes = b.pairs * rec;
        pending.buf = b.buf;
    }
    if (pending.bytes) SKL_TRY(issue_copy(pending));
    HIP_TRY(hipStreamSynchronize(ctx->aux_stream));   // host memory is complete on return
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SKL_OK;
}

static int dense_mode(const skl_dist_params *p, int *mode, int *jout)
{
    if (p->dist_type == SKL_DIST_COREACC) {
        *mode = MODE_COREACC;
        *jout = 0;
    } else {
        *mode = MODE_JACCARD;
        *jout = p->ani ? JOUT_ANI : JOUT_DIST;
    }
    return SKL_OK;
}

// ---------------------------------------------------------------------------
// dense entry points
// ---------------------------------------------------------------------------

extern "C" int skl_self_dists_rows(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p,
                                   size_t row_begin, size_t row_end, float *out, int out_on_device)
{
    SKL_TRY(check_params(s, s, p));
    int mode, jout;
    dense_mode(p, &mode, &jout);
    return dense_rows(ctx, s, s, p, mode, jout, 1, row_begin, row_end, out, out_on_device);
}

extern "C" int skl_self_dists_all(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p,
                                  float *out, int out_on_device)
{
    if (!s) return fail(SKL_ERR_INVALID_ARG, "null sketches");
    if (s->n < 2) {
        SKL_TRY(check_params(s, s, p));
        return SKL_OK;  // empty upper triangle
    }
    return skl_self_dists_rows(ctx, s, p, 0, s->n, out, out_on_device);
}

extern "C" int skl_cross_dists_rows(skl_ctx *ctx, const skl_sketches *ref,
                                    const skl_sketches *query, const skl_dist_params *p,
                                    size_t ref_begin, size_t ref_end, float *out,
                                    int out_on_device)
{
    SKL_TRY(check_params(ref, query, p));
    int mode, jout;
    dense_mode(p, &mode, &jout);
    return dense_rows(ctx, ref, query, p, mode, jout, 0, ref_begin, ref_end, out, out_on_device);
}

extern "C" int skl_cross_dists_all(skl_ctx *ctx, const skl_sketches *ref,
                                   const skl_sketches *query, const skl_dist_params *p, float *out,
                                   int out_on_device)
{
    if (!ref || !query) return fail(SKL_ERR_INVALID_ARG, "null sketches");
    return skl_cross_dists_rows(ctx, ref, query, p, 0, ref->n, out, out_on_device);
}

extern "C" int skl_self_binmatch(skl_ctx *ctx, const skl_sketches *s, uint32_t *out,
                                 int out_on_device)
{
    if (!s) return fail(SKL_ERR_INVALID_ARG, "null sketches");
    if (s->n < 2) return SKL_OK;
    skl_dist_params p = {SKL_DIST_JACCARD, 0, 0, 0.0};
    return dense_rows(ctx, s, s, &p, MODE_COUNTS, 0, 1, 0, s->n, out, out_on_device);
}

extern "C" int skl_cross_binmatch(skl_ctx *ctx, const skl_sketches *ref,
                                  const skl_sketches *query, uint32_t *out, int out_on_device)
{
    skl_dist_params p = {SKL_DIST_JACCARD, 0, 0, 0.0};
    SKL_TRY(check_params(ref, query, &p));
    return dense_rows(ctx, ref, query, &p, MODE_COUNTS, 0, 0, 0, ref->n, out, out_on_device);
}

// ---------------------------------------------------------------------------
// one-shot host forms
// ---------------------------------------------------------------------------

extern "C" int skl_self_dists_all_host(const uint64_t *bins, size_t n_samples, size_t nk,
                                       const size_t *kmers, size_t sketchsize64,
                                       const skl_dist_params *p, const double *completeness,
                                       float *out)
{
    skl_ctx *ctx = nullptr;
    SKL_TRY(skl_ctx_create(0, &ctx));
    skl_sketches *s = nullptr;
    int rc = skl_sketches_create(ctx, bins, 0, n_samples, nk, kmers, sketchsize64, &s);
    if (rc == SKL_OK && completeness) rc = skl_sketches_set_completeness(s, completeness);
    if (rc == SKL_OK) rc = skl_self_dists_all(ctx, s, p, out, 0);
    skl_sketches_destroy(s);
    skl_ctx_destroy(ctx);
    return rc;
}

extern "C" int skl_cross_dists_all_host(const uint64_t *ref_bins, size_t n_ref,
                                        const uint64_t *query_bins, size_t n_query, size_t nk,
                                        const size_t *kmers, size_t sketchsize64,
                                        const skl_dist_params *p, const double *ref_completeness,
                                        const double *query_completeness, float *out)
{
    skl_ctx *ctx = nullptr;
    SKL_TRY(skl_ctx_create(0, &ctx));
    skl_sketches *r = nullptr, *q = nullptr;
    int rc = skl_sketches_create(ctx, ref_bins, 0, n_ref, nk, kmers, sketchsize64, &r);
    if (rc == SKL_OK) rc = skl_sketches_create(ctx, query_bins, 0, n_query, nk, kmers, sketchsize64, &q);
    if (rc == SKL_OK && ref_completeness) rc = skl_sketches_set_completeness(r, ref_completeness);
    if (rc == SKL_OK && query_completeness) rc = skl_sketches_set_completeness(q, query_completeness);
    if (rc == SKL_OK) rc = skl_cross_dists_all(ctx, r, q, p, out, 0);
    skl_sketches_destroy(q);
    skl_sketches_destroy(r);
    skl_ctx_destroy(ctx);
    return rc;
}
