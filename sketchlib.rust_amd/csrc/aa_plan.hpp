// aa_plan.hpp -- HOW the amino-acid sketching call (skl_sketch_signs_aa, aa_sketch_kernel.hip) deals window starts to threads
// and samples to batches, as data computed by pure functions.
//
// Two workload shapes go through one call: proteomes (few samples of 10^5 - 10^7 residues) and single proteins (10^5 - 10^7
// samples of 50 - 2 000 residues).  A sample of at least `long_min` residues takes the STAGED form: one workgroup per chunk of
// AA_WG_LDS x AA_SPAN_LDS window starts, residues and bin minima in LDS.  Every other sample takes the UNSTAGED form: one thread
// per span of `short_span` window starts, threads of consecutive samples packed into workgroups without padding, bins in global
// memory -- a 300-residue protein costs 19 threads, not a workgroup.  A k-mer length beyond AA_K_STAGED_MAX sends every sample
// to the unstaged form.  Which form a sample takes never changes its signs.
//
// The two locators (aa_long_item, aa_short_item) are compiled for the host and the device: the kernels call what
// tests/native/aa_plan_check.cpp checks on the CPU.  No HIP header.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "sketch_plan.hpp"   // cut_before

#if defined(__HIPCC__)
#define SKL_AA_HD __host__ __device__
#else
#define SKL_AA_HD
#endif

namespace skl {

constexpr uint32_t AA_SPAN_LDS = 64;        // window starts per thread of the staged form (= residues per staged row)
constexpr uint32_t AA_WG_LDS = 256;         // threads per workgroup of the staged form
constexpr uint32_t AA_CHUNK = AA_SPAN_LDS * AA_WG_LDS;   // window starts per workgroup
constexpr uint32_t AA_K_STAGED_MAX = 256;   // longest k-mer the staged form takes (its windows reach k - 1 residues past the chunk)
constexpr uint32_t AA_LDS_BINS_MAX = 4096;  // most bins whose minima the staged form keeps in LDS
constexpr uint64_t AA_LONG_MIN = 8192;      // residues from which a sample is worth a workgroup of its own (half a chunk)
constexpr uint32_t AA_WG_SHORT = 256;       // threads per workgroup of the unstaged form
// a batch of whole samples: its signs (what comes back: 8 bytes x bins x k-mer lengths per sample, 8 KiB for a protein at
// 1 024 bins) and its residues (what goes up)
constexpr uint64_t AA_BATCH_SIGN_BYTES = 256ull << 20, AA_BATCH_RESIDUES = 256ull << 20;

struct AaPlan {
    uint32_t short_span = 16;           // window starts per thread of the unstaged form
    std::vector<uint64_t> wg_begin;     // [n + 1] prefix sum: workgroups of the staged form per sample (0 for the others)
    std::vector<uint64_t> span_begin;   // [n + 1] prefix sum: threads of the unstaged form per sample (0 for the others)
};

// A thread of the unstaged form seeds k - 1 residues for its span: spans grow with the longest k-mer, in steps of 16, 16 to 256.
inline uint32_t aa_short_span(size_t kmax)
{
    const size_t s = (std::max<size_t>(kmax, 1) + 15) / 16 * 16;
    return (uint32_t)std::min<size_t>(256, s);
}

// long_min: AA_LONG_MIN, or what the test knob forces (1: every non-empty sample staged)
inline AaPlan aa_plan(const uint64_t *res_begin, size_t n_samples, size_t kmax, uint64_t long_min)
{
    AaPlan p;
    p.short_span = aa_short_span(kmax);
    p.wg_begin.assign(n_samples + 1, 0);
    p.span_begin.assign(n_samples + 1, 0);
    const bool staged_ok = kmax <= AA_K_STAGED_MAX;
    for (size_t s = 0; s < n_samples; ++s) {
        const uint64_t len = res_begin[s + 1] - res_begin[s];
        const bool staged = staged_ok && len != 0 && len >= long_min;
        p.wg_begin[s + 1] = p.wg_begin[s] + (staged ? (len + AA_CHUNK - 1) / AA_CHUNK : 0);
        p.span_begin[s + 1] = p.span_begin[s] + (staged ? 0 : (len + p.short_span - 1) / p.short_span);
    }
    return p;
}

// Batches of whole samples [cuts[b], cuts[b + 1]): a batch closes before the sample that would take its signs past
// max_sign_bytes or its residues past max_residues (a single sample beyond either is a batch of its own).
inline std::vector<size_t> aa_batches(const uint64_t *res_begin, size_t n_samples, size_t nk, uint64_t num_bins,
                                      uint64_t max_sign_bytes, uint64_t max_residues)
{
    return cut_before(n_samples, [&](size_t s) { return res_begin[s + 1] - res_begin[s]; },
                      CutCaps{max_residues, (uint64_t)nk * num_bins * sizeof(uint64_t), max_sign_bytes});
}

// The sample whose items [begin[s], begin[s + 1]) hold item t: the last s with begin[s] <= t (samples without items are
// stepped over).  t < begin[n].
SKL_AA_HD inline uint32_t aa_find_sample(const uint64_t *begin, uint32_t n_samples, uint64_t t)
{
    uint32_t lo = 0, hi = n_samples;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (begin[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// The window starts [first, first + count) of `sample` a thread owns (count 0: none).
struct AaItem {
    uint32_t sample;
    uint64_t first;
    uint32_t count;
};

// thread `t` of the unstaged form
SKL_AA_HD inline AaItem aa_short_item(const uint64_t *span_begin, const uint64_t *res_begin, uint32_t n_samples, uint32_t span,
                                      uint64_t t)
{
    AaItem it;
    it.sample = aa_find_sample(span_begin, n_samples, t);
    const uint64_t len = res_begin[it.sample + 1] - res_begin[it.sample];
    it.first = (t - span_begin[it.sample]) * span;
    it.count = it.first < len ? (uint32_t)(len - it.first < span ? len - it.first : span) : 0u;
    return it;
}

// thread `tid` of workgroup `wg` of the staged form
SKL_AA_HD inline AaItem aa_long_item(const uint64_t *wg_begin, const uint64_t *res_begin, uint32_t n_samples, uint64_t wg,
                                     uint32_t tid)
{
    AaItem it;
    it.sample = aa_find_sample(wg_begin, n_samples, wg);
    const uint64_t len = res_begin[it.sample + 1] - res_begin[it.sample];
    it.first = (wg - wg_begin[it.sample]) * AA_CHUNK + (uint64_t)tid * AA_SPAN_LDS;
    it.count = it.first < len ? (uint32_t)(len - it.first < AA_SPAN_LDS ? len - it.first : AA_SPAN_LDS) : 0u;
    return it;
}

}  // namespace skl
