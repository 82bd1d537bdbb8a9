// capi_slab.cpp -- the entry points of include/sketchlib_dist.h that make a NEW slab from resident ones:
// skl_sketches_select (MultiSketch::remove_genomes' keep list, multisketch.rs:305-348; a subset or a reordering) and
// skl_sketches_concat (merge_sketches / `append`, multisketch.rs:247-267).  The inputs are never written: the result has
// its own allocations and its own generation id, so no early-break plan kept for an input goes stale and no pointer a
// caller holds moves.  The rows go from slab to slab on the device (slab_ops.hip's gather; two device copies for a
// concatenation), straight into the new slab's row allocation; the lane slab and the tables of the result are built on
// demand like any other slab's.  A completeness vector follows its samples through skl_sketches_set_completeness, which
// recomputes everything derived from it: those n doubles are all that is read back.
#include "capi_internal.hpp"

#include <vector>

using namespace skl;

namespace {

// the completeness values of `s` on the host (the context's stream has been waited for)
int read_completeness(const skl_sketches *s, double *dst)
{
    HIP_TRY(hipMemcpy(dst, s->d_comp, s->n * sizeof(double), hipMemcpyDeviceToHost));
    return SKL_OK;
}

// wait for the rows, then install `comp` (or none) in the new slab; on any failure the slab is gone
int finish_slab(skl_ctx *ctx, skl_sketches *s, const std::vector<double> *comp, hipError_t queued, skl_sketches **out)
{
    hipError_t e = queued;
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    int rc = e == hipSuccess ? SKL_OK : fail(SKL_ERR_HIP, "slab copy: %s", hipGetErrorString(e));
    if (rc == SKL_OK && comp) rc = skl_sketches_set_completeness(s, comp->data());
    if (rc != SKL_OK) {
        skl_sketches_destroy(s);
        return rc;
    }
    *out = s;
    return SKL_OK;
}

}  // namespace

extern "C" int skl_sketches_select(skl_ctx *ctx, const skl_sketches *s, const uint32_t *ids_host, size_t n_ids,
                                   skl_sketches **out)
{
    const RoctxRange range_("skl:sketches select");
    if (!out) return fail(SKL_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    SKL_TRY(ctx_bind(ctx));
    if (!s || !ids_host) return fail(SKL_ERR_INVALID_ARG, "null argument");
    if (s->ctx != ctx) return fail(SKL_ERR_INVALID_ARG, "sketches belong to another context");
    if (n_ids == 0) return fail(SKL_ERR_INVALID_ARG, "select: the id list is empty");
    if (n_ids >= (1ull << 31)) return fail(SKL_ERR_INVALID_ARG, "select: %zu ids, a slab holds fewer than 2^31 samples", n_ids);
    for (size_t i = 0; i < n_ids; ++i) {   // everything is checked before anything is allocated or launched
        if (ids_host[i] >= s->n) {
            return fail(SKL_ERR_INVALID_ARG, "select: ids[%zu] = %u, the slab has %zu samples", i, (unsigned)ids_host[i], s->n);
        }
    }
    std::vector<double> comp;
    if (s->d_comp) {
        std::vector<double> all(s->n);
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        SKL_TRY(read_completeness(s, all.data()));
        comp.resize(n_ids);
        for (size_t i = 0; i < n_ids; ++i) comp[i] = all[ids_host[i]];
    }
    DevBuf d_ids;
    HIP_TRY(hipMalloc(&d_ids.p, n_ids * sizeof(uint32_t)));
    skl_sketches *r = nullptr;
    SKL_TRY(slab_alloc(ctx, n_ids, s->nk, s->kmers.data(), s->ss64, &r));
    hipError_t e = hipMemcpyAsync(d_ids.p, ids_host, n_ids * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        SlabGatherArgs a;
        a.src = reinterpret_cast<const uint4 *>(s->d_rows);
        a.dst = reinterpret_cast<uint4 *>(r->d_rows);
        a.ids = static_cast<const uint32_t *>(d_ids.p);
        a.n_ids = n_ids;
        a.row_vec = (uint64_t)s->sample_words() * sizeof(uint64_t) / sizeof(uint4);   // 14 words per chunk: always even
        std::pair<hipEvent_t, hipEvent_t> *ev = timing_slot(ctx);   // (skl_ctx_timing_enable: bracketed like the pair kernels)
        if (ev) e = hipEventRecord(ev->first, ctx->stream);
        if (e == hipSuccess) e = launch_slab_gather(a, ctx->n_cu, ctx->stream);
        if (e == hipSuccess && ev) e = hipEventRecord(ev->second, ctx->stream);
        ctx->last_kernel = "skl::slab_gather_kernel";
    }
    // (finish_slab waits for the stream: the id list is freed after the kernel has read it)
    return finish_slab(ctx, r, s->d_comp ? &comp : nullptr, e, out);
}

extern "C" int skl_sketches_concat(skl_ctx *ctx, const skl_sketches *a, const skl_sketches *b, skl_sketches **out)
{
    const RoctxRange range_("skl:sketches concat");
    if (!out) return fail(SKL_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    SKL_TRY(ctx_bind(ctx));
    if (!a || !b) return fail(SKL_ERR_INVALID_ARG, "null argument");
    if (a->ctx != ctx || b->ctx != ctx) return fail(SKL_ERR_INVALID_ARG, "sketches belong to another context");
    if (a->nk != b->nk || a->ss64 != b->ss64 || a->kmers != b->kmers) {   // MultiSketch::is_compatible_with, multisketch.rs:222-226
        return fail(SKL_ERR_INCOMPATIBLE, "Databases are not compatible for merging.");
    }
    if ((a->d_comp == nullptr) != (b->d_comp == nullptr)) {
        return fail(SKL_ERR_INVALID_ARG, "concat: one slab has a completeness vector and the other has none");
    }
    if (a->n + b->n >= (1ull << 31)) return fail(SKL_ERR_INVALID_ARG, "concat: %zu samples, a slab holds fewer than 2^31", a->n + b->n);
    std::vector<double> comp;
    if (a->d_comp) {
        comp.resize(a->n + b->n);
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        SKL_TRY(read_completeness(a, comp.data()));
        SKL_TRY(read_completeness(b, comp.data() + a->n));
    }
    skl_sketches *r = nullptr;
    SKL_TRY(slab_alloc(ctx, a->n + b->n, a->nk, a->kmers.data(), a->ss64, &r));
    const size_t words = a->sample_words();
    hipError_t e = hipSuccess;
    if (a->n) e = hipMemcpyAsync(r->d_rows, a->d_rows, a->n * words * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess && b->n) {
        e = hipMemcpyAsync(r->d_rows + a->n * words, b->d_rows, b->n * words * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream);
    }
    return finish_slab(ctx, r, a->d_comp ? &comp : nullptr, e, out);
}
