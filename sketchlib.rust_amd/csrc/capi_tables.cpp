// capi_tables.cpp -- what the host libm decides for the device: which restated form of its logarithm the kernels run (the
// completeness path; glibc_log.hpp), and the upload of a slab's samebits -> ln J / distance tables.  The tables' arithmetic is
// dist_tables.hpp's (pure); here they are only allocated and copied.
#include "capi_internal.hpp"
#include "dist_tables.hpp"
#include "glibc_log.hpp"

#include <cmath>
#include <vector>

using namespace skl;

static_assert(TABLE_BBITS == BBITS && TABLE_JOUT_DIST == JOUT_DIST && TABLE_JOUT_ANI == JOUT_ANI,
              "dist_tables.hpp restates these constants of kernels.h");

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
// a slab's tables on the device, made on first use
// ---------------------------------------------------------------------------

int ensure_ytab(const skl_sketches *cs)
{
    skl_sketches *s = const_cast<skl_sketches *>(cs);
    if (s->d_ytab) return SKL_OK;
    const LnjTable tab = lnj_table(s->ss64);
    const size_t m = tab.lnj.size();
    s->min_alive = tab.min_alive;
    double *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, m * sizeof(double)));
    const hipError_t e = hipMemcpy(d, tab.lnj.data(), m * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return fail(SKL_ERR_HIP, "ln J table upload: %s", hipGetErrorString(e));
    }
    s->d_ytab = d;
    return SKL_OK;
}

int ensure_dtab(const skl_sketches *cs, int jout, size_t k_idx, float **out)
{
    skl_sketches *s = const_cast<skl_sketches *>(cs);
    const size_t key_k = jout == JOUT_DIST ? 0 : k_idx;
    auto it = s->d_dtab.find({jout, key_k});
    if (it != s->d_dtab.end()) {
        *out = it->second;
        return SKL_OK;
    }
    const std::vector<float> tab = dist_table(jout, (double)s->kmers[k_idx], s->ss64);
    const size_t m = tab.size();
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
