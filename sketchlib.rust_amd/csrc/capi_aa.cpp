// capi_aa.cpp -- skl_sketch_signs_aa and skl_sketch_usigs_aa of include/sketchlib_dist.h: GPU sketching of amino-acid sequences.
// Kernels: aa_sketch_kernel.hip; who hashes what: aa_plan.hpp (pure); seeds and roll values: aa_seeds.hpp.
#include "capi_internal.hpp"

#include <algorithm>
#include <cstring>

#include "aa_seeds.hpp"
#include "nthash.hpp"

using namespace skl;

// fin: every stream is finished on the device behind its batch's bin minima and goes there; out_signs unused
static int sketch_signs_aa_impl(skl_ctx *ctx, const uint8_t *residues, const uint64_t *res_begin, size_t n_samples,
                                const size_t *kmers, size_t nk, uint64_t num_bins, int level, int concat_end_rule,
                                uint64_t *out_signs, const FinishDest *fin)
{
    SKL_TRY(ctx_bind(ctx));
    if (!res_begin || !kmers || (!out_signs && !fin)) return fail(SKL_ERR_INVALID_ARG, "null argument");
    if (n_samples == 0 || nk == 0) return SKL_OK;
    if (num_bins == 0 || num_bins > 0xFFFFFFFFull) return fail(SKL_ERR_INVALID_ARG, "num_bins out of range");
    if (n_samples >= 0xFFFFFFFFull) return fail(SKL_ERR_INVALID_ARG, "too many samples");
    const uint64_t *seeds = aa_seed_table(level);
    if (!seeds) return fail(SKL_ERR_INVALID_ARG, "aaHash level must be 1, 2 or 3");
    for (size_t s = 0; s < n_samples; ++s) {
        if (res_begin[s + 1] < res_begin[s]) return fail(SKL_ERR_INVALID_ARG, "sample ranges must not decrease");
    }
    const uint64_t r_first = res_begin[0], r_last = res_begin[n_samples];
    if (r_last > r_first && !residues) return fail(SKL_ERR_INVALID_ARG, "null argument");
    {   // the kernels index their 21-row tables with these bytes
        uint8_t worst = 0;
        for (uint64_t x = r_first; x < r_last; ++x) worst = std::max(worst, residues[x]);
        if (worst >= AA_N_CODES) return fail(SKL_ERR_INVALID_ARG, "residue code above 20");
    }
    size_t kmax = 0;
    std::vector<uint32_t> k32(nk);
    std::vector<uint64_t> roll(nk * AA_N_CODES);
    for (size_t ki = 0; ki < nk; ++ki) {
        if (kmers[ki] == 0 || kmers[ki] > 0xFFFFu) return fail(SKL_ERR_INVALID_ARG, "k-mer length out of range");
        k32[ki] = (uint32_t)kmers[ki];
        kmax = std::max(kmax, kmers[ki]);
        aa_roll_table(seeds, kmers[ki], roll.data() + ki * AA_N_CODES);
    }
    const uint64_t long_min = ctx->knobs.aa_long_min > 0 ? (uint64_t)ctx->knobs.aa_long_min : AA_LONG_MIN;
    const AaPlan plan = aa_plan(res_begin, n_samples, kmax, long_min);
    const uint64_t max_sign_bytes = ctx->knobs.aa_batch_sign_bytes > 0 ? (uint64_t)ctx->knobs.aa_batch_sign_bytes : AA_BATCH_SIGN_BYTES;
    const std::vector<size_t> cuts = aa_batches(res_begin, n_samples, nk, num_bins, max_sign_bytes, AA_BATCH_RESIDUES);
    uint64_t most_samples = 0, most_residues = 0;
    for (size_t b = 0; b + 1 < cuts.size(); ++b) {
        most_samples = std::max<uint64_t>(most_samples, cuts[b + 1] - cuts[b]);
        most_residues = std::max(most_residues, res_begin[cuts[b + 1]] - res_begin[cuts[b]]);
    }
    const size_t per_sample = nk * num_bins;

    void *d_codes = nullptr, *d_signs = nullptr, *d_small = nullptr;
    SKL_TRY(ctx_scratch(ctx, most_residues + 16, &d_codes, SCRATCH_SKETCH_BASES));   // (8 readable bytes past the last residue)
    SKL_TRY(ctx_scratch(ctx, most_samples * per_sample * sizeof(uint64_t), &d_signs, SCRATCH_SKETCH_SIGNS));
    FinishDev fin_dev;
    if (fin) SKL_TRY(finish_reserve(ctx, most_samples * nk, num_bins, &fin_dev));
    std::vector<uint64_t> small;
    auto put = [&](const uint64_t *v, size_t count) {
        const size_t at = small.size();
        small.insert(small.end(), v, v + count);
        return at;
    };
    const size_t at_rb = put(res_begin, n_samples + 1), at_wg = put(plan.wg_begin.data(), n_samples + 1),
                 at_sp = put(plan.span_begin.data(), n_samples + 1), at_seed = put(seeds, AA_N_CODES),
                 at_roll = put(roll.data(), roll.size());
    const size_t at_k = small.size();
    small.resize(at_k + (nk + 1) / 2, 0);
    memcpy(small.data() + at_k, k32.data(), nk * sizeof(uint32_t));
    SKL_TRY(ctx_scratch(ctx, small.size() * sizeof(uint64_t), &d_small, SCRATCH_SKETCH_SMALL));
    HIP_TRY(hipMemcpyAsync(d_small, small.data(), small.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // (`small` is pageable: uploaded before it dies)

    AaSketchArgs a;
    memset(&a, 0, sizeof a);
    const uint64_t *ds = (const uint64_t *)d_small;
    a.codes = (const uint8_t *)d_codes;
    a.res_begin = ds + at_rb;
    a.n_samples = (uint32_t)n_samples;
    a.nk = (uint32_t)nk;
    a.kmers = (const uint32_t *)(ds + at_k);
    a.seeds = ds + at_seed;
    a.roll = ds + at_roll;
    a.num_bins = num_bins;
    a.bin_size = bin_size_of(num_bins);
    a.inv_bin_size = 1.0 / (double)a.bin_size;
    a.end_rule = concat_end_rule ? 1u : 0u;
    a.short_span = plan.short_span;
    a.signs = (uint64_t *)d_signs;

    // Batch after batch on one stream: residues up, bins to u64::MAX, the unstaged and the staged launch, signs back.  (The
    // copies are to and from the caller's pageable memory: nothing here overlaps them with the kernels.)
    bool any_staged = false, any_unstaged = false;
    for (size_t b = 0; b + 1 < cuts.size(); ++b) {
        const size_t s0 = cuts[b], s1 = cuts[b + 1];
        const uint64_t bytes = res_begin[s1] - res_begin[s0];
        if (bytes) HIP_TRY(hipMemcpyAsync(d_codes, residues + res_begin[s0], bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemsetAsync((uint8_t *)d_codes + bytes, 0, 16, ctx->stream));
        HIP_TRY(hipMemsetAsync(d_signs, 0xFF, (s1 - s0) * per_sample * sizeof(uint64_t), ctx->stream));
        a.res_base = res_begin[s0];
        a.sample_base = (uint32_t)s0;
        for (int staged = 0; staged < 2; ++staged) {
            const std::vector<uint64_t> &begin = staged ? plan.wg_begin : plan.span_begin;
            a.staged = (uint32_t)staged;
            a.item_begin = ds + (staged ? at_wg : at_sp);
            a.first_item = begin[s0];
            a.n_items = begin[s1] - begin[s0];
            if (a.n_items == 0) continue;
            (staged ? any_staged : any_unstaged) = true;
            std::pair<hipEvent_t, hipEvent_t> *tev = timing_slot(ctx);   // (bracketed like the pair kernels, launch by launch)
            if (tev) HIP_TRY(hipEventRecord(tev->first, ctx->stream));
            HIP_TRY(launch_aa_sketch_signs(a, ctx->stream));
            if (tev) HIP_TRY(hipEventRecord(tev->second, ctx->stream));
        }
        if (fin) {   // densify + transpose behind the batch's bin minima; the words, first signs and flags come back
            SKL_TRY(finish_launch(ctx, (const uint64_t *)d_signs, (s1 - s0) * nk, num_bins, fin_dev, 0));
            SKL_TRY(finish_download(fin_dev, 0, (s1 - s0) * nk, num_bins, *fin, s0 * nk, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            SKL_TRY(finish_fallback((const uint64_t *)d_signs, (s1 - s0) * nk, num_bins, *fin, s0 * nk));   // (before the next batch overwrites the signs)
            continue;
        }
        HIP_TRY(hipMemcpyAsync(out_signs + s0 * per_sample, d_signs, (s1 - s0) * per_sample * sizeof(uint64_t),
                               hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    const char *staged_name = num_bins <= (uint64_t)AA_LDS_BINS_MAX
                                  ? "skl::aahash_binmin_lds_kernel (residue codes, seed and roll tables and bin minima in LDS, 64 window starts per thread)"
                                  : "skl::aahash_binmin_lds_kernel (residue codes, seed and roll tables in LDS, 64 window starts per thread, bin minima in global memory)";
    const char *unstaged_name = "skl::aahash_binmin_kernel (a thread per span of any sample, packed without padding, bin minima in global memory)";
    ctx->last_kernel = any_staged && any_unstaged ? std::string(staged_name) + " + " + unstaged_name
                       : any_staged               ? staged_name
                                                  : unstaged_name;
    if (fin) ctx->last_kernel += std::string(" + ") + finish_kernel_name(ctx, num_bins);
    return sketch_scratch_release(ctx, false);
}

extern "C" int skl_sketch_signs_aa(skl_ctx *ctx, const uint8_t *residues, const uint64_t *res_begin, size_t n_samples,
                                   const size_t *kmers, size_t nk, uint64_t num_bins, int level, int concat_end_rule,
                                   uint64_t *out_signs)
{
    return sketch_signs_aa_impl(ctx, residues, res_begin, n_samples, kmers, nk, num_bins, level, concat_end_rule, out_signs, nullptr);
}

// The same call with every (sample, k) stream finished (SKL_SKETCH_FINISH=host: the signs come back and host threads finish them).
extern "C" int skl_sketch_usigs_aa(skl_ctx *ctx, const uint8_t *residues, const uint64_t *res_begin, size_t n_samples,
                                   const size_t *kmers, size_t nk, uint64_t num_bins, int level, int concat_end_rule,
                                   uint64_t *out_usigs, uint64_t *out_first_sign, uint8_t *out_flags)
{
    SKL_TRY(ctx_bind(ctx));
    if (!out_usigs || !out_flags) return fail(SKL_ERR_INVALID_ARG, "null argument");
    SKL_TRY(finish_check_bins(num_bins));
    return sketch_finished_call(ctx, n_samples * nk, num_bins, FinishDest{out_usigs, out_first_sign, out_flags},
                                [&](uint64_t *signs, const FinishDest *fin) {
                                    return sketch_signs_aa_impl(ctx, residues, res_begin, n_samples, kmers, nk, num_bins, level,
                                                                concat_end_rule, signs, fin);
                                });
}

// the shapes a caller (and the tests) can ask for
extern "C" int skl_sketch_aa_shape(int what, size_t kmax)
{
    switch (what) {
    case 0: return (int)AA_SPAN_LDS;         // window starts per thread of the staged form
    case 1: return (int)AA_WG_LDS;           // its threads per workgroup
    case 2: return (int)AA_LDS_BINS_MAX;     // most bins it keeps in LDS
    case 3: return (int)AA_K_STAGED_MAX;     // longest k-mer it takes
    case 4: return (int)AA_LONG_MIN;         // residues from which a sample is staged
    case 5: return (int)aa_short_span(kmax); // window starts per thread of the unstaged form at this longest k-mer
    case 6: return (int)AA_WG_SHORT;         // its threads per workgroup
    default: return -1;
    }
}
