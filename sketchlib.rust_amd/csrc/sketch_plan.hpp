// sketch_plan.hpp -- HOW the DNA sketching calls (skl_sketch_signs*, sketch_kernel.hip; skl_reads_survivors, read_survivors.hip)
// deal window starts to threads and samples to batches, and how the host layer (host/sketch_gpu.cpp) cuts its inputs into calls,
// as data computed by pure functions.  The kernels and the host read the shapes below under the same names.  No HIP header;
// tests/native/sketch_plan_check.cpp checks it on the CPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace skl {

constexpr int SKETCH_SPAN = 256;            // window starts per thread of the unstaged kernel
constexpr int SKETCH_WG = 256;              // its threads per workgroup
constexpr int SKETCH_SPAN_LDS = 128;        // window starts per thread of the LDS-staged kernel: it takes k <= SKETCH_SPAN_LDS + 1
constexpr int SKETCH_WG_LDS = 512;          // its threads (= spans) per workgroup
constexpr int SKETCH_LDS_BINS_MAX = 4096;   // most bins whose minima it keeps in LDS; above it they stay in global memory
constexpr int READ_SURVIVOR_SPAN = 64;      // window starts per thread of the read-survivor kernel
constexpr int READ_SURVIVOR_WG = 256;       // its threads per workgroup
constexpr uint64_t SKETCH_BATCH_WORDS = 8ull << 20;   // upload batches of ~8 Mi words (128 Mi bases)

struct SketchPlan {
    bool lds_form = true;               // the LDS-staged kernel (every k-mer length up to its span + 1), or the unstaged one
    std::vector<uint64_t> span_begin;   // [n + 1] prefix sum: spans per sample, padded to whole workgroups
    std::vector<uint64_t> word_begin;   // [n + 1] prefix sum: packed words per sample (16 codes each, the last zero-padded)
};

// force_global: SKL_SKETCH_KERNEL=global (A/B).  code_begin must not decrease.
inline SketchPlan sketch_plan(const uint64_t *code_begin, size_t n_samples, size_t kmax, bool force_global)
{
    SketchPlan p;
    p.lds_form = kmax <= (size_t)SKETCH_SPAN_LDS + 1 && !force_global;
    const uint64_t span = (uint64_t)(p.lds_form ? SKETCH_SPAN_LDS : SKETCH_SPAN);
    const uint64_t wg = (uint64_t)(p.lds_form ? SKETCH_WG_LDS : SKETCH_WG);
    p.span_begin.assign(n_samples + 1, 0);
    p.word_begin.assign(n_samples + 1, 0);
    for (size_t s = 0; s < n_samples; ++s) {
        const uint64_t len = code_begin[s + 1] - code_begin[s];
        uint64_t spans = (len + span - 1) / span;
        spans = (spans + wg - 1) / wg * wg;   // whole workgroups per sample (the staged kernel needs it; batches of samples then
                                              // start on workgroup boundaries in either form)
        p.span_begin[s + 1] = p.span_begin[s] + spans;
        p.word_begin[s + 1] = p.word_begin[s] + (len + 15) / 16;
    }
    return p;
}

// Upload batches of whole samples [cuts[b], cuts[b + 1]): a batch is closed BEHIND the sample with which it reaches batch_words,
// unless that sample is the last.
inline std::vector<size_t> sketch_upload_batches(const uint64_t *word_begin, size_t n_samples, uint64_t batch_words)
{
    std::vector<size_t> cuts{0};
    for (size_t s = 0; s < n_samples; ++s) {
        if (word_begin[s + 1] - word_begin[cuts.back()] >= batch_words && s + 1 < n_samples) cuts.push_back(s + 1);
    }
    cuts.push_back(n_samples);
    return cuts;
}

// One launch of the read-survivor kernel: win_begin | win_end | span_begin ([n] [n] [n + 1], as uploaded).  The window range of a
// sample is clamped to the sample; its spans are padded to whole waves.
inline std::vector<uint64_t> read_survivor_spans(const uint64_t *code_begin, const uint64_t *win_begin, const uint64_t *win_end, size_t n)
{
    const uint64_t span = (uint64_t)READ_SURVIVOR_SPAN;
    std::vector<uint64_t> head(3 * n + 1, 0);
    for (size_t s = 0; s < n; ++s) {
        const uint64_t len = code_begin[s + 1] - code_begin[s];
        const uint64_t b = std::min(win_begin[s], len), e = std::max(b, std::min(win_end[s], len));
        head[s] = b;
        head[n + s] = e;
        const uint64_t spans = ((e - b + span - 1) / span + 63) / 64 * 64;   // whole waves per sample
        head[2 * n + s + 1] = head[2 * n + s] + spans;
    }
    return head;
}

// Batches of whole items [cuts[b], cuts[b + 1]) of items 0 .. n - 1: a batch closes BEFORE the item that would take its summed
// size past max_sum, or its count times unit_cost past max_cost (a single item beyond either is a batch of its own; n = 0: one
// empty batch).
struct CutCaps {
    uint64_t max_sum, unit_cost, max_cost;
};
template <class SizeOf>
inline std::vector<size_t> cut_before(size_t n, SizeOf size_of, const CutCaps &caps)
{
    std::vector<size_t> cuts{0};
    uint64_t sum = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t size = size_of(i);
        const size_t b0 = cuts.back();
        if (i > b0 && (sum + size > caps.max_sum || (i + 1 - b0) * caps.unit_cost > caps.max_cost)) {
            cuts.push_back(i);
            sum = 0;
        }
        sum += size;
    }
    cuts.push_back(n);
    return cuts;
}

// The caps of the host layer's calls (host/sketch_gpu.cpp), sizes in bases / residues:
// one skl_sketch_usigs_aa call: 1 Gi residues and 1 GiB of signs on the device
inline CutCaps caps_aa_call(size_t nk, uint64_t num_bins) { return {1ull << 30, (uint64_t)nk * num_bins * sizeof(uint64_t), 1ull << 30}; }
// one skl_sketch_usigs_packed call: ~4 G bases
inline CutCaps caps_dna_call() { return {4ull << 30, 0, 0}; }
// one skl_sketch_bins_u16_packed call: ~4 G bases and 1 GiB of signs on the device
inline CutCaps caps_u16_call(uint64_t num_bins) { return {4ull << 30, num_bins * sizeof(uint64_t), 1ull << 30}; }
// read sets under a count filter: at most max(64, nk) streams (one 24 MiB filter each) and ~1 G bases
inline CutCaps caps_filtered_reads(size_t nk) { return {1ull << 30, (uint64_t)nk, std::max<uint64_t>(64, nk)}; }

}  // namespace skl
