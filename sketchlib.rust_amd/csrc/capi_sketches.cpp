// capi_sketches.cpp -- device slabs (the MultiSketch bins in the two layouts the pair kernel wants) and the launch preparation
// every kind of call shares: parameter checks that map the reference's panics to status codes, and the operand / epilogue
// fields of a launch.
#include "capi_internal.hpp"
#include "dist_tables.hpp"
#include "glibc_log.hpp"

#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

using namespace skl;

// ---------------------------------------------------------------------------
// sketch slabs
// ---------------------------------------------------------------------------

static std::atomic<uint64_t> g_next_gen{1};
uint64_t next_generation() { return g_next_gen.fetch_add(1); }

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

void free_sketches_locked(skl_sketches *s)
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
    g->tolerance = break_tolerance(rows->ss64);
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
