// capi_internal.hpp -- shared between the translation units that implement
// include/sketchlib_dist.h.  Not part of the public boundary.
//   capi_ctx.cpp       errors, the handle registry, a context's life cycle, streams, scratch, launch timing, the clock sampler
//   capi_knobs.cpp     the environment, read into `Knobs` (knobs.def, knobs.hpp) -- the one file that calls the C library's lookup
//   capi_tables.cpp    the probe of the host libm's logarithm; upload of the ln J / distance tables (dist_tables.hpp)
//   capi_sketches.cpp  slabs, parameter checks, the operand / epilogue fields of a launch
//   capi_eb.cpp        the early break's sample and the decisions a context keeps
//   capi_dense.cpp     one pair-kernel launch, the dense executors and entry points
//   capi_knn.cpp       the kNN drivers;  capi_cand.cpp  candidate lists;  capi_pairs.cpp  pair lists;  capi_rccl.cpp  the RCCL gather
//   capi_sketch.cpp    DNA sketching;  capi_reads.cpp  read survivors;  capi_aa.cpp  amino-acid sketching;  capi_inv.cpp  inverted query
//   capi_finish.cpp    finishing sketch streams on the device;  capi_slab.cpp  new slabs from resident ones
//   capi_within.cpp    the pairs of a dense call that lie within a distance cap;  capi_clusters.cpp  the clusters those pairs connect
//   capi_hist.cpp      the histogram of the values a dense call stores;  capi_mst.cpp  the minimum spanning forest of the distance graph
// Everything declared here is SKL_INTERNAL (hidden): the library exports the functions of the public header and nothing else of the host layer.
// How a dense call and each pair-kernel launch is shaped is decided in dense_plan.hpp (pure, no HIP), reached through kernels.h;
// the early break's decision in eb_plan.hpp; how the kNN drivers cut and feed their bands in knn_plan.hpp (both pure, no HIP).
#pragma once

#include "../../include/sketchlib_dist.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "kernels.h"
#include "eb_plan.hpp"
#include "knn_plan.hpp"
#include "knobs.hpp"
#include "roctx_ranges.hpp"

#define SKL_INTERNAL __attribute__((visibility("hidden")))

// ---- error plumbing: status code + message for skl_last_error() ----
SKL_INTERNAL int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            return fail(e_ == hipErrorOutOfMemory ? SKL_ERR_OOM : SKL_ERR_HIP, "%s: %s",   \
                        #expr, hipGetErrorString(e_));                                     \
        }                                                                                  \
    } while (0)

#define SKL_TRY(expr)             \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != SKL_OK) return rc_; \
    } while (0)

struct skl_sketches;

// the process environment as of now (capi_knobs.cpp): for skl_ctx_create, skl_ctx_reload_env and the A/B build's ctx_bind alone
SKL_INTERNAL Knobs read_knobs();
#ifdef SKL_AB
SKL_INTERNAL int ab_forced_log_variant();   // SKL_FORCE_LOG_VARIANT, for the cached probe of host_log_variant() (-2: not forced)
#endif

// EARLY BREAK of the core/accessory calls, as decided for one (row slab, column slab) pair: how many k-mer lengths the pair
// kernel counts before the epilogue completes the pairs still in the running -- for the whole pair space (`decision.lengths`;
// what the kNN drivers take) and, when its blocks of (row >> shift_r, column >> shift_c) sample ids disagree, per block.
// The rules -- when a decision is taken at all, the blocks, what the sampled histograms decide -- are eb_plan.hpp's (pure);
// capi_eb.cpp early_break_plan() samples and keeps the answer.  Kept by the CONTEXT, keyed by the slabs' generation ids (never
// reused), not written through the caller's const slab.
struct EbPlan {
    uint64_t rows_gen = 0, cols_gen = 0;
    int self_mode = 0, knob = 1;        // (knob: SKL_EARLY_BREAK as of the decision -- the A/B build may change it between calls)
    double cutoff = 0.0;                // completeness cutoff the sample was taken with (a correction changes ln J)
    skl::EbGeometry geo;                // the blocks
    skl::EbDecision decision;           // (decision.block_ke: host copy of the table, skl_ctx_early_break_blocks)
    uint8_t *d_block_ke = nullptr;      // the table on the device when the blocks disagree
};

// The context's grow-only scratch buffers (ctx_scratch).
enum ScratchSlot : int {
    SCRATCH_KEY_BAND = 0,          // key band of the kNN drivers; band of a host-destined dense call
    SCRATCH_COUNTS = 1,            // bin-match counts
    SCRATCH_KNN_STAGING = 2,       // kNN results on their way to the host
    SCRATCH_KEY_BAND_2 = 3,        // the second key band (bands that overlap)
    SCRATCH_TURNED_BAND = 4,       // turned key band (symmetric kNN) ...
    SCRATCH_TURNED_BAND_2 = 5,     // ... and the second one
    SCRATCH_KNN_FLAGS = 6,         // its row flags (2 x n u32)
    SCRATCH_KNN_ROW_BITS = 7,      // its block bits
    SCRATCH_PRUNE_BOUNDS = 8,      // tile-pruning bounds (n u32)
    SCRATCH_KNN_TURNED_BITS = 9,   // bits of the turned bands
    SCRATCH_PRUNE_COUNTERS = 10,   // pruning counters
    SCRATCH_FUSE_COUNTERS = 11,    // arrival counters of the fused epilogue
    SCRATCH_SKETCH_BASES = 12,     // GPU sketching: packed bases,
    SCRATCH_SKETCH_SIGNS = 13,     // signs,
    SCRATCH_SKETCH_SMALL = 14,     // small arrays
    SCRATCH_COUNTS_2 = 15,         // second counts band (early break of the core/accessory kNN; odd bands of an overlapped dense call)
    SCRATCH_SKETCH_FINISHED = 16,  // GPU sketching: finished words, first signs and flags on their way to the host,
    SCRATCH_SKETCH_TARGETS = 17,   // the finish kernel's target arrays (global form)
    SCRATCH_WITHIN = 18,           // pairs within a cap: running total, chunk offsets, chunk counts (within_plan.hpp)
    SCRATCH_CLUSTER_LABELS = 19,   // clusters within a cap: error word, root count, and the label array(s) of a caller whose own are on the host (cluster_plan.hpp)
    SCRATCH_HIST = 20,             // histogram of the stored values: the two outside words, and the counts of a caller whose own are on the host (hist_plan.hpp)
    SCRATCH_MST = 21,              // minimum spanning forest: counters, labels, best / component words, edge records; the staged edges of skl_clusters_from_edges (mst_plan.hpp)
    SCRATCH_SLOTS = 22
};

struct skl_ctx {
    int device = 0;
    int n_cu = 256;                     // compute units of the device (MI355X: 256)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // grow-only scratch
    void *scratch[SCRATCH_SLOTS] = {};
    size_t scratch_bytes[SCRATCH_SLOTS] = {};
    uint32_t *pinned = nullptr;         // pinned host ring of the sketching upload (two batches of packed bases; grow-only)
    uint64_t pinned_words = 0;
    size_t fuse_counter_k = 0;          // k-mer lengths the arrival counters of SCRATCH_FUSE_COUNTERS count modulo (fused epilogue)
    hipStream_t aux_stream = nullptr;   // top-k of band i runs here while band i+1 is computed
    hipStream_t epi_stream = nullptr;   // overlapped row bands of a large early-break call (dense_plan.hpp plan_row_bands): band i's epilogue beside band i+1's counts kernel
    // band pipelines (kNN: pair kernel -> top-k; dense to host: pair kernel -> D2H copy):
    // "producer finished buffer b" / "consumer finished buffer b"
    hipEvent_t knn_pair_done[2] = {nullptr, nullptr}, knn_topk_done[2] = {nullptr, nullptr};
    // timing of pair-kernel launches of the last call
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t events_used = 0;
    long long timing_every = 0;         // skl_ctx_timing_enable / SKL_TIMING_EVERY: 0 = launches are not bracketed (default)
    size_t launches_seen = 0;           // pair-kernel launches since the last skl_ctx_timing_reset
    std::string last_kernel;
    bool last_unit_table = false;       // the last pair launch read a unit table (unit_table.hpp; skl_ctx_unit_table)
    int unit_table_mode = -1;           // skl_ctx_set_unit_table: -1 the dense calls' launches ask for a table, 0 nobody does, 1 every launch does
    // plane 1 of the counts scratch as the tail slices need it: all zero.  Valid for exactly
    // this (pointer, bytes) until anything else writes the scratch.
    const void *clean_plane1 = nullptr;
    size_t clean_plane1_bytes = 0;
    // skl_clock_sampler_start/stop: one-wave shader-clock sampler on its own stream (diagnostic)
    hipStream_t sampler_stream = nullptr;
    uint32_t *sampler_stop = nullptr;   // pinned host flag the kernel polls
    uint64_t *sampler_buf = nullptr;    // [max][2] (s_memtime, s_memrealtime)
    uint32_t *sampler_count = nullptr;
    uint32_t sampler_max = 0;
    bool sampler_running = false;
    uint64_t knn_tiles_sparse = 0;         // tiles that survived the probe and were finished by the sparse walk (alive rows only)
    uint64_t knn_tiles_probe_pruned = 0;   // ... of the pruned tiles, those the plane-pair probe settled before the walk began
    uint64_t knn_pruned_stages = 0, knn_tile_stages = 0;   // ... stages the pruned tiles had walked / stages of a whole tile
    uint32_t *eb_counter = nullptr;        // device word: pairs the early-break epilogue completed (skl_ctx_early_break_stats)
    uint64_t eb_pairs = 0;                 // ... out of this many pairs of early-break launches since the context was made
    // overlapped row bands of a large early-break dense call: counts kernels on `stream`, epilogues on `epi_stream`
    hipEvent_t eb_events[4] = {nullptr, nullptr, nullptr, nullptr};   // counts of buffer b done / epilogue of buffer b done
    std::vector<EbPlan *> eb_plans;        // early-break decisions of the last few slab pairs (newest last)
    const EbPlan *eb_last_plan = nullptr;  // the plan of the last dense core/accessory call (skl_ctx_early_break_blocks)
    bool knn_prune_pending = false;        // the device counters (SCRATCH_PRUNE_COUNTERS) hold counts not yet read back
    uint64_t knn_tiles = 0, knn_tiles_pruned = 0;   // tile pruning of the last self kNN call (skl_ctx_knn_prune_stats)
    int knn_ties = SKL_KNN_TIES_REFERENCE;   // what self_dists_knn returns (mod.rs:133-224); skl_ctx_set_knn_ties(CANONICAL) opts out
    Knobs knobs;                        // environment switches as of skl_ctx_create
    skl::TileScratch tile_scratch;      // device table of the balanced tile enumeration
    std::set<skl_sketches *> sketches;  // slabs created on this context
};

struct skl_sketches {
    skl_ctx *ctx = nullptr;
    size_t n = 0, nk = 0, ss64 = 0;
    std::vector<size_t> kmers;
    uint64_t *d_rows = nullptr;  // reference layout + A_PAD_ROWS zero rows (scalar operand)
    uint4 *d_lanes = nullptr;    // lane-interleaved layout (vector operand), built on demand
    double *d_comp = nullptr;    // completeness or null
    bool comp_unit = false;      // every completeness value is finite and in (0, 1] (what the lean early-break epilogue's integer tests need)
    double *d_ytab = nullptr;    // ln J table [64*ss64+1]
    double *d_kf = nullptr;      // k-mer lengths as f64 [nk]
    std::map<std::pair<int, size_t>, float *> d_dtab;  // (jout, k_idx) -> f32 table
    uint64_t gen = 0;            // generation id, unique per slab AND per completeness vector over the life of the process
    uint32_t min_alive = 0xFFFFFFFFu;   // ln J(count) < tolerance <=> count < min_alive (set with d_ytab; 0xFFFFFFFF: ask the table)
    size_t sample_words() const { return nk * ss64 * skl::BBITS; }
};

// device allocation freed at scope exit
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

using skl::BAND_BYTES;   // (knn_plan.hpp: the kNN band heights read it too)

SKL_INTERNAL int ctx_bind(skl_ctx *ctx);
// the handle registry (capi_ctx.cpp): live slabs, and the lock that guards them and the live contexts
SKL_INTERNAL extern std::mutex g_registry_mutex;
SKL_INTERNAL extern std::set<const void *> g_live_sketches;
SKL_INTERNAL void free_sketches_locked(skl_sketches *s);   // (capi_sketches.cpp; the registry lock held; a handle already gone: no-op)
SKL_INTERNAL void free_plans(skl_ctx *ctx);                // the early-break decisions a context keeps (capi_eb.cpp)
SKL_INTERNAL uint64_t next_generation();                   // a slab's / completeness vector's generation id, never reused (capi_sketches.cpp)
// a registered slab whose rows [0, n_samples) are still to be written on the context's stream (capi_sketches.cpp; the pad rows are
// queued to zero, nothing is waited for); skl_sketches_create and the slab operations of capi_slab.cpp fill it
SKL_INTERNAL int slab_alloc(skl_ctx *ctx, size_t n_samples, size_t nk, const size_t *kmers, size_t sketchsize64, skl_sketches **out);
// a slab's tables on the device, made on first use (capi_tables.cpp): ln J with min_alive; the single-k distance / ANI table
SKL_INTERNAL int ensure_ytab(const skl_sketches *s);
SKL_INTERNAL int ensure_dtab(const skl_sketches *s, int jout, size_t k_idx, float **out);
// which glibc_log.hpp form reproduces this host's libm log(): probed once per process against
// std::log; SKL_LOG_FMA / SKL_LOG_SSE2, or -1 when neither does (the FMA form is then used and a
// warning printed once)
SKL_INTERNAL int host_log_variant();
// grow-only scratch slot `which` of the context, at least `bytes` large
SKL_INTERNAL int ctx_scratch(skl_ctx *ctx, size_t bytes, void **out, ScratchSlot which);
// log2 of the XCDs the tile order deals workgroups to
SKL_INTERNAL inline uint32_t ctx_xcd_shift(const skl_ctx *ctx) { return skl::plan_xcd_shift(ctx->n_cu, ctx->knobs.xcds); }
// A/B build: SKL_KERNEL, and a forced tile shape or ablation counts as a forced kernel (no chunk slices, no mid-band rule);
// product library: always 0
SKL_INTERNAL inline int forced_kernel(const skl_ctx *ctx)
{
    if (ctx->knobs.kernel == 0 && (ctx->knobs.kslice_shape || ctx->knobs.kslice_ablate)) return 4;
    return ctx->knobs.kernel;
}
// the pair kernel bracketed by HIP events on the context's stream (skl_ctx_kernel_ms)
SKL_INTERNAL int timed_pair_launch(skl_ctx *ctx, const skl::PairArgs &args, int mode);
// records [first, second) events around a launch of another kernel the same way; returns the
// slot to record into or null when the event budget is used up
SKL_INTERNAL std::pair<hipEvent_t, hipEvent_t> *timing_slot(skl_ctx *ctx);
SKL_INTERNAL int check_params(const skl_sketches *a, const skl_sketches *b, const skl_dist_params *p);
SKL_INTERNAL bool fused_coreacc_ok(const skl_sketches *s);
// early break of the core/accessory calls (capi_eb.cpp): the decision for this slab pair (sampled once, kept by the context);
// *plan = null: not applicable (eb_plan.hpp eb_applicable: fewer than 3 or more than 8 k-mer lengths, a tiny pair space, switched off)
SKL_INTERNAL int early_break_plan(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, int self_mode, double cutoff,
                                  const EbPlan **plan);
// ... its pooled form, for the kNN drivers: k-mer lengths the pair kernel should count (0: all of them)
SKL_INTERNAL int early_break_lengths(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, int self_mode, int *lengths);
// operand / epilogue fields common to every launch: `rows` is the scalar operand (A), `cols` the lane operand (B)
SKL_INTERNAL int fill_args(const skl_sketches *rows, const skl_sketches *cols, const skl_dist_params *p, int mode,
                           int jout, skl::PairArgs *g);
// ... the same without making the lane-layout copy of `cols` (kernels that read both sides in the reference layout)
SKL_INTERNAL int fill_args_ref_layout(const skl_sketches *rows, const skl_sketches *cols, const skl_dist_params *p, int mode,
                                      int jout, skl::PairArgs *g);
// rows [r0, r1) of the pair space into `dst_dev` (device memory), launched as dense_plan.hpp decides
SKL_INTERNAL int dense_band(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols,
                            const skl_dist_params *p, int mode, int jout, int self_mode, uint64_t r0, uint64_t r1,
                            void *dst_dev);

// ---- finishing streams of bin minima on the device (capi_finish.cpp; sketch_finish.hip, finish_plan.hpp) ----
// where a call's finished streams go on the host: [streams][finish_words(num_bins)], [streams] (may be null), [streams];
// bins_u16 set: the u16 form instead -- rows [streams][num_bins] and the flags, usigs / first_sign unused
struct FinishDest {
    uint64_t *usigs, *first_sign;
    uint8_t *flags;
    uint16_t *bins_u16 = nullptr;
};
// ... and where the kernel leaves them on the device (SCRATCH_SKETCH_FINISHED), with the global form's target arrays
struct FinishDev {
    uint64_t *usigs = nullptr, *first_sign = nullptr;
    uint8_t *flags = nullptr;
    uint32_t *targets = nullptr;
    uint16_t *bins_u16 = nullptr;   // u16 form: the rows (usigs / first_sign null)
};
SKL_INTERNAL int finish_check_bins(uint64_t num_bins);   // a multiple of 64 that a u32 indexes, or SKL_ERR_INVALID_ARG
SKL_INTERNAL int finish_check_bins_u16(uint64_t num_bins);   // the u16 form: 1 to 2^32 - 1
SKL_INTERNAL int finish_reserve(skl_ctx *ctx, uint64_t streams, uint64_t num_bins, FinishDev *dev, bool u16 = false);
// streams [0, n_streams) of d_signs into dev's streams [at, at + n_streams), on the context's stream
SKL_INTERNAL int finish_launch(skl_ctx *ctx, const uint64_t *d_signs, uint64_t n_streams, uint64_t num_bins, const FinishDev &dev, uint64_t at);
// dev's streams [at, at + n_streams) to dst's [dst_at, ...), queued on `stream`
SKL_INTERNAL int finish_download(const FinishDev &dev, uint64_t at, uint64_t n_streams, uint64_t num_bins, const FinishDest &dst, uint64_t dst_at,
                                 hipStream_t stream);
// once the download has landed: dst's streams [dst_at, dst_at + n_streams) that are flagged FINISH_UNFINISHED are finished on
// the host from their signs in d_signs (stream s of the range at d_signs + s * num_bins); they keep the flag
SKL_INTERNAL int finish_fallback(const uint64_t *d_signs, uint64_t n_streams, uint64_t num_bins, const FinishDest &dst, uint64_t dst_at);
// every stream (or only those flagged FINISH_UNFINISHED) of host signs [n_streams][num_bins] on host threads
SKL_INTERNAL void finish_on_host(const uint64_t *signs, uint64_t n_streams, uint64_t num_bins, const FinishDest &dst, bool only_unfinished);
SKL_INTERNAL const char *finish_kernel_name(const skl_ctx *ctx, uint64_t num_bins, bool u16 = false);   // what skl_ctx_last_kernel() says of the finish

// ---- shared by the sketching entry points (capi_sketch.cpp, capi_aa.cpp) ----
// The sketching buffers belong to the context so that a run of sketch calls does not allocate per call -- but beyond 1 GiB they
// would sit in the way of what follows (the kNN drivers size their bands by the free memory): released, with the pinned ring of
// the DNA upload when asked.  Both streams must be idle.
SKL_INTERNAL int sketch_scratch_release(skl_ctx *ctx, bool pinned_ring);
// A sketching call whose `streams` streams come back finished in dst.  impl(out_signs, fin) is the call itself: finished on the
// device behind each batch's bin minima (out_signs null, fin = &dst), or -- SKL_SKETCH_FINISH=host -- its signs come back
// (fin null) and host threads finish them, as callers did before.
template <class Impl>
inline int sketch_finished_call(skl_ctx *ctx, size_t streams, uint64_t num_bins, const FinishDest &dst, const Impl &impl)
{
    if (!ctx->knobs.sketch_finish_host) return impl(nullptr, &dst);
    std::unique_ptr<uint64_t[]> signs(new uint64_t[std::max<size_t>(streams * num_bins, 1)]);   // (not zero-filled: the call writes every word)
    SKL_TRY(impl(signs.get(), nullptr));
    finish_on_host(signs.get(), streams, num_bins, dst, false);
    ctx->last_kernel += std::string(" + ") + finish_kernel_name(ctx, num_bins, dst.bins_u16 != nullptr);
    return SKL_OK;
}
