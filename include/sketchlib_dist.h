/*
 * sketchlib_dist.h -- C ABI of the MI355X (gfx950) pairwise-distance engine.
 *
 * This is the drop-in boundary for bacpop/sketchlib.rust's `distances` module:
 * each entry point names the reference function it replaces (file:line relative
 * to the reference tree, v0.3.0).  Signatures use plain pointers and sizes only,
 * so the same library binds from Rust (`extern "C"`), C++
 * (sketchlib.rust_amd/csrc/host) and Python ctypes (sketchlib.rust_amd/capi.py).
 *
 * Sketch bins cross the boundary in the reference's own layout -- the `.skd`
 * byte order, MultiSketch::sketch_bins (src/sketch/multisketch.rs:36-40,
 * 213-219): little-endian u64,
 *     word(sample, k_idx, chunk, plane) =
 *         sample*sample_stride + k_idx*kmer_stride + chunk*14 + plane
 *     kmer_stride = sketchsize64*14 (BBITS, src/sketch/mod.rs:34),
 *     sample_stride = kmer_stride*nk.
 * Any device-side re-layout is internal to the library.
 *
 * Error handling: every function returns SKL_OK (0) or a positive SKL_ERR_*;
 * skl_last_error() returns a thread-local message.  Where the reference
 * panics (jaccard.rs:70-72, mod.rs:318-323) the ABI returns the matching code
 * and the same message text.  There is no CPU fallback: without a usable GPU
 * every compute entry point fails with SKL_ERR_NO_DEVICE.
 *
 * LIMITS (one place; each is checked and reported with SKL_ERR_INVALID_ARG / SKL_ERR_OOM, never silently):
 *   - samples per slab: < 2^31; the library keeps TWO copies of every slab in HBM (row layout + lane layout,
 *     2 x n x nk x sketchsize64 x 112 B): ~7 M genomes per 288 GB GPU at sketchsize64 = 32, nk = 5.
 *   - skl_sketches_select / skl_sketches_concat return a NEW slab and leave their inputs resident: source and result are both
 *     in HBM (their row slabs, and the lane slab of each once a call has used it as the column side) until the caller
 *     destroys one.  Dropping 10 % of a 18 GB slab therefore needs 16 GB more for as long as the old slab lives.
 *   - sketchsize64: < 2^25.  Up to 1 023 (65 472 bins) a k-mer length's counts live in u16 fields; larger sketches
 *     (the reference's "100000-1000000 for SNP level resolution", lib.rs:41-42) take the same kernel, walked in
 *     segments of 1 016 chunks; their core/accessory distances go through a bin-match count scratch of at most
 *     4 GiB per launch (bands of rows).  nk x sketchsize64 < 1 198 372 for the fast kernel (32-bit row offsets).
 *   - k-mer lengths: < 2^16; the fused core/accessory kernel takes up to 6, more go counts + epilogue.
 *   - knn: 1 <= knn <= candidates.  Up to 2 048 neighbours the running lists live in LDS (one-evaluation self kNN,
 *     skl_self_dists_knn_partial, skl_knn_merge_states); longer lists go row by row through global memory.
 *   - skl_self_dists_knn_shared_bins: at most skl_shared_bins_max_samples() = 1 294 336 samples per call.
 *   - timing: at most 4 096 bracketed pair-kernel launches between two skl_ctx_timing_reset();
 *     skl_clock_sampler_start: interval_us x max_samples <= 10 s.
 */
#ifndef SKETCHLIB_DIST_H
#define SKETCHLIB_DIST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKL_ABI_VERSION 1

/* ---- status codes ---- */
#define SKL_OK 0
#define SKL_ERR_INVALID_ARG 1
#define SKL_ERR_NO_DEVICE 2   /* no HIP device / wrong architecture */
#define SKL_ERR_HIP 3         /* a HIP runtime call failed */
#define SKL_ERR_OOM 4
#define SKL_ERR_KMER_COUNT 5  /* "Need at least two k-mer lengths ..." jaccard.rs:70-72 */
#define SKL_ERR_EMPTY_DB 6    /* "... database has no loaded samples" mod.rs:318-323 */
#define SKL_ERR_KMER_NOT_FOUND 7 /* "K-mer size {k} not found in file" mod.rs:28-30 */
#define SKL_ERR_INCOMPATIBLE 8   /* ref/query differ in k-mers or sketch size */

/* DistType (src/distances/distance_matrix.rs:55-61) */
#define SKL_DIST_COREACC 0
#define SKL_DIST_JACCARD 1

typedef struct skl_ctx skl_ctx;           /* one per (host thread, device) */
typedef struct skl_sketches skl_sketches; /* device-resident MultiSketch bins */

/* Parameters shared by all distance calls.  Mirrors DistType::Jaccard(k_idx, k,
 * ani) / DistType::CoreAcc plus the completeness_cutoff argument every driver in
 * src/distances/mod.rs takes. */
typedef struct {
    int32_t dist_type;           /* SKL_DIST_COREACC | SKL_DIST_JACCARD */
    int32_t ani;                 /* Jaccard only: report ANI (jaccard.rs:49-51) */
    uint64_t k_idx;              /* Jaccard only: index into the k-mer list */
    double completeness_cutoff;  /* cli.rs:229 default 0.64 */
} skl_dist_params;

const char *skl_last_error(void);
int skl_abi_version(void);
/* Number of visible gfx950 devices (0 if none; never fails). */
int skl_device_count(void);

/* ---- context ---- */
int skl_ctx_create(int device, skl_ctx **out);
int skl_ctx_destroy(skl_ctx *ctx);
/* Run all subsequent work of this context on a caller-owned hipStream_t
 * (e.g. torch.cuda.current_stream().cuda_stream).  NULL restores the context's
 * own stream. */
int skl_ctx_set_stream(skl_ctx *ctx, void *hip_stream);
/* Run on the device's (legacy) default stream -- hipStream_t 0, which is what
 * torch.cuda.current_stream().cuda_stream is unless the caller entered a stream context.
 * The context's own stream is non-blocking, i.e. NOT ordered with work queued on the default
 * stream; a caller that fills or reads buffers with default-stream work and does not
 * synchronise explicitly wants this. */
int skl_ctx_use_default_stream(skl_ctx *ctx);
int skl_ctx_synchronize(skl_ctx *ctx);
/* The library's few environment switches (INTEGRATION.md "Building") are read when a context is
 * created and never on the launch path; this re-reads them for an existing context (tests and
 * benchmarks that compare two drivers inside one process). */
int skl_ctx_reload_env(skl_ctx *ctx);
/* Pair-kernel timing -- a diagnostic, OFF by default (an event record is a barrier packet on the queue: two per
 * launch cost a sub-millisecond launch ~5 us).  enable(every): every = 0 turns it off, N >= 1 brackets every N-th
 * launch of the pair kernel (dense / binmatch / knn calls; also the candidate-list and the sketching kernel) with HIP
 * events recorded on the context's stream (the environment variable SKL_TIMING_EVERY sets the initial value).
 * reset() forgets the recorded events; kernel_ms() synchronises and returns the summed device time and the number of
 * launches recorded since the last reset (at most 4096 are kept). */
int skl_ctx_timing_enable(skl_ctx *ctx, int every);
int skl_ctx_timing_reset(skl_ctx *ctx);
int skl_ctx_kernel_ms(skl_ctx *ctx, float *total_ms, int *n_launches);
/* Name (with tile shape) of the pair kernel the last call dispatched, e.g.
 * "pair_kernel_ksplit<R=4>" -- for benchmark reports.  Valid until the next call. */
const char *skl_ctx_last_kernel(skl_ctx *ctx);

/* Diagnostic (no reference counterpart): the shader clock the chip holds while the context's kernels
 * run.  start() launches a one-wave sampler on a stream of its own (it stamps the shader-clock counter
 * against the constant 100 MHz counter every interval_us, at most max_samples times, then ends by
 * itself); run the work to be measured, wait for it with skl_ctx_synchronize() -- NOT a device-wide
 * synchronisation, which would wait for the sampler -- and call stop(): clock readings in GHz, one
 * per interval (median, 10th / 90th percentile, and the mean over the whole window). */
int skl_clock_sampler_start(skl_ctx *ctx, uint32_t interval_us, uint32_t max_samples);
int skl_clock_sampler_stop(skl_ctx *ctx, double *ghz_median, double *ghz_p10, double *ghz_p90, double *ghz_mean,
                           int *n_intervals);

/* The reference takes ln J with Rust's f64::ln = the platform libm's log() (jaccard.rs:51,88), and
 * the core/accessory regression amplifies its last bit without bound on flat fits, so the
 * device evaluates a restatement of glibc's log() (csrc/glibc_log.hpp) whenever the argument is
 * not a function of the bin-match count alone (completeness correction).  skl_log_variant(): the
 * form that reproduces THIS host's log() bit for bit on a probe set: 0 = glibc 2.35 x86-64 FMA
 * form, 1 = its SSE2 form, -1 = neither (form 0 is used; flat-fit pairs may then differ from a
 * CPU run on this host).  skl_device_log(): y[i] = that logarithm of x[i], evaluated on the
 * device (host pointers) -- for tests. */
int skl_log_variant(void);
/* Conditions a caller may want to tell its user about (a null context is accepted and reports the flags that are
 * properties of the host process).  SKL_CTX_FLAG_LOG_UNMATCHED: skl_log_variant() == -1 -- this host's libm
 * log() is neither form the device can reproduce, so completeness-corrected core distances of FLAT fits
 * (jaccard.rs:120-133: the same bin-match count at every k-mer length) may come out 0 where a CPU run of
 * the reference on this host gives 1, or the reverse.  Everything else is unaffected. */
#define SKL_CTX_FLAG_LOG_UNMATCHED 1u
/* SKL_CTX_FLAG_NOT_SPX (needs a context): the device does not report the 256 compute units of an unpartitioned (SPX)
 * MI355X.  Results do not depend on it.  The tile order follows the device (workgroups are dealt to CUs / 32 XCDs, the
 * resident-round sizes use the CU count); the launch sizes at which tile shapes and chunk slicing switch were tuned on
 * SPX only (DESIGN.md "Topology assumptions"). */
#define SKL_CTX_FLAG_NOT_SPX 2u
unsigned skl_ctx_flags(const skl_ctx *ctx);
int skl_device_log(skl_ctx *ctx, const double *x_host, size_t n, double *out_host);

/* ---- sketch slabs: MultiSketch::read_sketch_data / get_sketch_slice
 *      (src/sketch/multisketch.rs:167-219) ---- */
/* bins: n_samples*nk*sketchsize64*14 u64 in the reference layout.  `on_device`
 * != 0 means `bins` is already a device pointer on the context's device. */
int skl_sketches_create(skl_ctx *ctx, const uint64_t *bins, int on_device, size_t n_samples,
                        size_t nk, const size_t *kmers, size_t sketchsize64, skl_sketches **out);
/* Option<&Vec<f64>> completeness vector (src/io.rs:240-324); NULL == None. */
int skl_sketches_set_completeness(skl_sketches *s, const double *completeness_host);
int skl_sketches_destroy(skl_sketches *s);
size_t skl_sketches_n_samples(const skl_sketches *s);
/* New slabs from resident ones, without a trip through host memory.  Both return a NEW handle with its own
 * generation id (what early-break decisions are kept under) and never touch their inputs, which stay valid and are the
 * caller's to destroy; the rows are copied slab to slab on the context's stream, and the call returns when they are in
 * place.  A completeness vector follows its samples and is installed in the result the way
 * skl_sketches_set_completeness installs one (everything derived from it is recomputed for the result).
 * select: samples ids[0 .. n_ids) of `s`, in that order; repeats are allowed (remove_genomes' keep list,
 * multisketch.rs:305-348; a subset; a reordering).  n_ids == 0 or an id >= the slab's sample count is
 * SKL_ERR_INVALID_ARG, found before anything is allocated or launched. */
int skl_sketches_select(skl_ctx *ctx, const skl_sketches *s, const uint32_t *ids_host, size_t n_ids, skl_sketches **out);
/* concat: a's samples, then b's (merge_sketches, multisketch.rs:247-267; `append`).  Different k-mer lists or
 * sketchsize64: SKL_ERR_INCOMPATIBLE (is_compatible_with, multisketch.rs:222-226); a completeness vector on one side
 * only: SKL_ERR_INVALID_ARG. */
int skl_sketches_concat(skl_ctx *ctx, const skl_sketches *a, const skl_sketches *b, skl_sketches **out);

/* set_k (src/distances/mod.rs:25-37): kmer == 0 means Option::None -> CoreAcc. */
int skl_set_k(const skl_sketches *s, size_t kmer, int ani, double completeness_cutoff,
              skl_dist_params *out);

/* ---- dense distances ----
 * `out_on_device` != 0: `out` is a device pointer and the call only enqueues work
 * on the context's stream; == 0: `out` is host memory and the call returns after
 * the copy back. */

/* self_dists_all (src/distances/mod.rs:58-130).  out: n(n-1)/2 * ncols f32,
 * condensed upper triangle, ncols = 2 (core, acc interleaved) or 1. */
int skl_self_dists_all(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, float *out,
                       int out_on_device);
/* Rows [row_begin, row_end) of the same condensed matrix -- the slice
 * [square_to_condensed(row_begin,row_begin+1), square_to_condensed(row_end,row_end+1))
 * -- written to out[0..]; the multi-GPU pair-block partition. */
int skl_self_dists_rows(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p,
                        size_t row_begin, size_t row_end, float *out, int out_on_device);
/* cross_dists_all (src/distances/mod.rs:227-297).  out: n_ref*n_query*ncols,
 * index (i_ref*n_query + j_query)*ncols. */
int skl_cross_dists_all(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query,
                        const skl_dist_params *p, float *out, int out_on_device);
/* Reference rows [ref_begin, ref_end) of the same matrix. */
int skl_cross_dists_rows(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query,
                         const skl_dist_params *p, size_t ref_begin, size_t ref_end, float *out,
                         int out_on_device);

/* ---- all pairs within a distance cap (no reference counterpart): the dense listing with lines removed ----
 * What network building, threshold clustering and dereplication ask of a pair space: every pair closer than a cap, however
 * many a sample has.  The calls evaluate rows [row_begin, row_end) exactly as skl_self_dists_rows / skl_cross_dists_rows do
 * (same row-range rules: an empty range, or fewer than two samples, is SKL_OK with *n_found = 0; completeness vectors and
 * completeness_cutoff apply unchanged) and keep the pairs that pass, compacted on the device (csrc/within.hip).
 * ORDER: the dense call's own -- ascending condensed index (i < j) for the self call, ascending i_ref * n_query + j_query for
 * the cross call -- so the result is the dense listing with lines removed and never depends on scheduling.
 * RECORD r: out_i[r], out_j[r] = the pair's samples, indices into the whole slab(s), not into the row range (self: i < j;
 * cross: reference, query); out_d[r * ncols ...) = the f32 values the dense call stores, ncols = 2 (core, acc) or 1.
 * PREDICATE, on those f32 values (v0, v1):
 *     distance in the first column (core; single-k Jaccard distance):  v0 <= (float)max_first
 *     ANI (p->ani):                                                    v0 >= (float)(1.0 - (double)max_first)
 *                                     -- the cap is a distance in every mode; the bound is formed in double and rounded once
 *     core/accessory, additionally:                                    v1 <= (float)max_second
 *                                     -- max_second = INFINITY: the second column is not tested; ignored when ncols == 1
 * A NaN in a tested column never passes.  max_first or max_second NaN, or max_first < 0: SKL_ERR_INVALID_ARG.
 * CAPACITY: *n_found is always the number of pairs that pass.  Records [0, min(*n_found, capacity)) are written -- the first
 * ones in order -- and nothing beyond them is touched; the status is SKL_OK either way and the caller compares *n_found with
 * capacity.  capacity == 0 is the COUNT-ONLY form: the outputs may be NULL and the scatter pass is not launched.  capacity > 0
 * with a NULL output is SKL_ERR_INVALID_ARG.  The context keeps nothing between calls.
 * `out_on_device` != 0: out_i / out_j / out_d are device pointers.  Either way the call returns with the stream idle and the
 * records in place (it has *n_found to hand back).  The row range is evaluated in bands of the host-destined dense calls'
 * scratch budget (512 MiB; each band fewer than 2^32 pairs), a band's records appended behind the previous band's: a
 * whole-matrix call over a million samples needs no 4 TB buffer. */
int skl_self_dists_within(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t row_begin, size_t row_end,
                          double max_first, double max_second, uint32_t *out_i, uint32_t *out_j, float *out_d, uint64_t capacity,
                          int out_on_device, uint64_t *n_found);
int skl_cross_dists_within(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query, const skl_dist_params *p,
                           size_t ref_begin, size_t ref_end, double max_first, double max_second, uint32_t *out_i,
                           uint32_t *out_j, float *out_d, uint64_t capacity, int out_on_device, uint64_t *n_found);

/* ---- single-linkage clusters under a distance cap (no reference counterpart): the pairs above, followed to their components ----
 * What dereplication, outbreak detection and "one representative per strain" ask for is not the edge list but the clusters it
 * connects: one label per sample instead of one record per pair.  skl_self_clusters_within applies EXACTLY the pairs that
 * skl_self_dists_within would list for rows [row_begin, row_end) with the same p, max_first and max_second -- the same
 * PREDICATE on the same stored f32 values (ANI turns the test round, a NaN never passes, completeness vectors and
 * completeness_cutoff apply unchanged), the same row-range and cap errors -- and joins the two samples of each; no record is
 * written (csrc/cluster.hip: a lock-free union-find on the device behind each dense band).
 * LABELS: one u32 per sample of the slab -- all n of them, whatever the row range.  Two samples are in one cluster when a chain of
 * passing pairs connects them.  On return labels[i] is the LOWEST sample index of i's cluster: a property of the data alone,
 * never of scheduling, and labels[labels[i]] == labels[i].  *n_clusters is the number of i with labels[i] == i.
 * `labels_on_device` != 0: labels is a device pointer.  Either way the call returns with the stream idle and the labels in place.
 * FLAGS: 0 -- the labels are set to 0..n-1 first.  SKL_CLUSTERS_CONTINUE -- the labels hold the result of earlier calls and are
 * built upon: calls over consecutive row ranges chained this way give the whole call's labels.  The input must then satisfy
 * labels[i] <= i for every i (any output of these two calls does); it is checked on the device before anything follows a
 * label, and a violation is SKL_ERR_INVALID_ARG with labels unchanged.
 * EDGES: labels or n_clusters NULL: SKL_ERR_INVALID_ARG.  A slab of 0 samples: SKL_OK, *n_clusters = 0.  A single sample or an
 * empty row range applies no pair: the labels are still initialised (or checked and kept, with CONTINUE) and counted.  The row
 * range is evaluated in the bands of the within calls (same budget); the labels stay on the device between them. */
#define SKL_CLUSTERS_CONTINUE 1   /* labels hold the result of earlier calls; without it they are set to 0..n-1 first */
int skl_self_clusters_within(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t row_begin, size_t row_end,
                             double max_first, double max_second, uint32_t *labels, int labels_on_device, int flags,
                             uint64_t *n_clusters);
/* MERGE: joins two partitions of the same n samples, for instance the results of two row ranges computed on two devices, each
 * from the identity.  On return labels holds the clusters connected through either partition, in the same lowest-index form,
 * and *n_clusters their number; `other` is only read.  Both arrays live on the same side (`on_device`) and both are checked
 * as above (SKL_ERR_INVALID_ARG, labels unchanged).  No slab and no distances are involved.  n == 0: SKL_OK, *n_clusters = 0. */
int skl_clusters_merge(skl_ctx *ctx, uint32_t *labels, const uint32_t *other, uint64_t n, int on_device, uint64_t *n_clusters);

/* ---- histogram of the stored values (no reference counterpart): where a collection's distances lie ----
 * The calls above answer questions under a cap the caller already has; this one helps to choose it.  The answer to "where do the
 * distances of this collection lie" is a few kilobytes -- a histogram -- where the dense matrix is 40 GB at 100 000 genomes.
 * PAIRS: skl_self_dists_hist / skl_cross_dists_hist evaluate EXACTLY the pairs skl_self_dists_rows / skl_cross_dists_rows would
 * for the same row range: the same row-range rules and out-of-bounds error; an empty range, or fewer than two samples, is SKL_OK
 * with nothing counted; completeness vectors and completeness_cutoff apply unchanged.  The values binned are the f32 values the
 * dense call stores -- with p->ani the first column is the ANI itself -- and the grid is on stored values in every mode.
 * COUNTS: n0 * n1 u64, the cell (c0, c1) at c0 * n1 + c1.  One stored column (single-k Jaccard, ANI): lo1, hi1 and n1 are
 * ignored and n1 counts as 1.  `counts_on_device` != 0: counts is a device pointer.  Either way the call returns with the stream
 * idle and the results in place.
 * OUTSIDE: 2 u64, always on the host.  outside[0]: the pairs with a non-NaN value off the grid in some column; outside[1]: the
 * pairs with a NaN in some column (a NaN wins over off-grid).  sum(counts) + outside[0] + outside[1] is the number of pairs of
 * the range.
 * THE CELL RULE of a column, in f32 exactly as written: lo = (float)lo0, hi = (float)hi0, scale = (float)((double)n0 / ((double)hi
 * - (double)lo)).  A value v with v < lo || v > hi is outside (so is +-inf, unless that test admits it).  Otherwise
 * c = (uint32_t)((v - lo) * scale) -- one f32 subtract, one f32 multiply (never fused), truncation -- and c = min(c, n0 - 1): v == hi
 * lands in the last cell, v == lo in cell 0.  The second column likewise.  numpy float32 reproduces it bit for bit.
 * FLAGS: 0 -- counts and outside are zeroed first.  SKL_HIST_ACCUMULATE -- they hold earlier results and are added to: calls over
 * consecutive row ranges chained this way give the whole call's histogram.  Histograms of two devices merge by plain addition.
 * ERRORS, all SKL_ERR_INVALID_ARG with counts and outside untouched: grid, counts or outside NULL; n0 == 0, or n1 == 0 with two
 * columns; a bound that is NaN or infinite, hi <= lo after rounding to float, or a range so narrow that scale is not a finite
 * float; more than 2^20 cells (8 MiB of counts); unknown flag bits; a row range out of bounds.  The row range is evaluated in the
 * bands of the within calls (same budget); nothing crosses to the host between them (csrc/hist.hip). */
typedef struct skl_hist_grid {
    double lo0, hi0;      /* first stored column: [lo0, hi0] cut into n0 equal cells */
    double lo1, hi1;      /* second stored column (core/accessory only): n1 cells */
    uint32_t n0, n1;      /* ncols == 1: lo1, hi1, n1 are ignored and n1 counts as 1 */
} skl_hist_grid;
#define SKL_HIST_ACCUMULATE 1   /* counts and outside hold earlier results and are added to; without it they are zeroed first */
int skl_self_dists_hist(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t row_begin, size_t row_end,
                        const skl_hist_grid *grid, uint64_t *counts, int counts_on_device, int flags, uint64_t *outside);
int skl_cross_dists_hist(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query, const skl_dist_params *p,
                         size_t ref_begin, size_t ref_end, const skl_hist_grid *grid, uint64_t *counts, int counts_on_device,
                         int flags, uint64_t *outside);

/* ---- minimum spanning tree of the distances (no reference counterpart): the whole single-linkage hierarchy in n - 1 records ----
 * skl_self_clusters_within answers one cap; the histogram shows that there is usually more than one plausible cap.  The minimum
 * spanning tree of the distance graph holds every answer at once: cut at any threshold it gives exactly the single-linkage
 * clusters at that threshold, and sorted by weight it IS the single-linkage dendrogram -- 12 bytes a sample where the dense
 * matrix is 4 TB at a million samples.  Every rule below is on the f32 values of the dense listing, so numpy reproduces the
 * result from skl_self_dists_all alone (Kruskal over the edges sorted by the EDGE ORDER).
 * GRAPH: the vertices are all n samples of the slab -- there is no row range, every round needs every pair.
 * WEIGHTS: the weight of {i, j} is the f32 value the dense call stores for the pair in `column`: 0 -- the core distance, or the
 * single-k Jaccard distance; 1 -- the accessory distance, core/accessory only.  Completeness vectors and completeness_cutoff
 * apply unchanged.  p->ani != 0 is SKL_ERR_INVALID_ARG (the tree is defined on distances); so is column 1 with one stored
 * column, and any other column.
 * EDGES: a pair is an edge where w <= (float)max_dist.  max_dist = INFINITY: no cap.  A NaN weight is never an edge.  max_dist
 * NaN or negative: SKL_ERR_INVALID_ARG, as for the within calls.  So the result is in general a spanning FOREST; with a cap and
 * column 0 its components are exactly those of skl_self_clusters_within(max_first = max_dist, max_second = INFINITY).
 * EDGE ORDER: edges compare by (w, i, j) with i < j, w as a float with -0.0f == +0.0f (on the device: a monotone u32 key of
 * w + 0.0f, csrc/mst_plan.hpp).  The order is strict and total, so the minimum spanning forest under it is UNIQUE: the edges
 * Kruskal keeps when it takes them in that order.  The result is a property of the data alone, never of scheduling.
 * OUTPUT, all on the host: *n_edges = n minus the number of components; records r < *n_edges in ascending edge order -- the
 * order in which single linkage merges -- with out_i[r] < out_j[r] and out_w[r] the stored f32 (as w + 0.0f: a stored -0.0f is
 * reported as +0.0f).  The arrays have room for n - 1 records; nothing beyond *n_edges is touched.  labels may be NULL;
 * otherwise n u32 in the form of the cluster calls: the lowest index of the sample's component, flat.  *rounds: the Boruvka
 * rounds that added an edge (<= log2 n; each is one evaluation of the whole triangle, in the bands of the within calls).
 * EDGE CASES: n == 0: SKL_OK, *n_edges = 0.  n == 1: SKL_OK, *n_edges = 0, labels[0] = 0.  out_i, out_j, out_w, n_edges or
 * rounds NULL: SKL_ERR_INVALID_ARG.  More than 2^32 - 1 samples: SKL_ERR_INVALID_ARG. */
int skl_self_mst(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, int column, double max_dist,
                 uint32_t *out_i, uint32_t *out_j, float *out_w, uint32_t *labels,
                 uint64_t *n_edges, uint32_t *rounds);
/* CUTS: the clusters a list of edges connects among n samples -- union(edge_i[k], edge_j[k]) for every k from the identity, then
 * flattened and counted; labels (n u32) and *n_clusters in the form of skl_self_clusters_within.  Everything lives on the host.
 * Because the tree comes sorted by weight, "the clusters at threshold t" is this call on the prefix of its edges with w <= t:
 * O(n) per threshold instead of a dense pass.  An index >= n is SKL_ERR_INVALID_ARG, found on the device before anything
 * follows it, with labels untouched; so are labels or n_clusters NULL and an edge array NULL with n_edges_in > 0.  n == 0 with
 * no edge: SKL_OK, *n_clusters = 0. */
int skl_clusters_from_edges(skl_ctx *ctx, const uint32_t *edge_i, const uint32_t *edge_j, uint64_t n_edges_in,
                            uint64_t n, uint32_t *labels, uint64_t *n_clusters);

/* ---- sparse k-nearest-neighbour distances ----
 * Output rows hold `knn` items sorted ascending by key, where key = d0 for Jaccard / core for
 * CoreAcc, or 1-ANI for ANI (mod.rs:173-176).  out_d1 is written for CoreAcc only and may be NULL
 * otherwise.  knn is bounded only by the number of candidates (lib.rs:379-382, mod.rs:325): up to
 * 2 048 neighbours the running lists live in LDS, longer ones go through global memory.
 *
 * Equal keys (common: every genome without knn relatives ties at 1.0, and single-k Jaccard values are
 * quantised) -- skl_ctx_set_knn_ties() chooses between two rules for every kNN call of the context:
 *   SKL_KNN_TIES_REFERENCE (default)  the list the reference's self_dists_knn / cross_dists_knn return: candidates j
 *                                     ascending through push_heap (mod.rs:41-48: strict `<` against the heap's
 *                                     maximum) into std::collections::BinaryHeap, then into_sorted_vec (mod.rs:156-191,
 *                                     :335-391) -- which of several equal keys survive, and their order, follow from
 *                                     the heap's history, which the device replays.  skl_self_dists_knn over the whole
 *                                     matrix still evaluates every pair ONCE: a row's heap lives in device memory
 *                                     between the row bands and is fed its candidates in ascending id (rows above its
 *                                     band reach it through the band's turned copy); row ranges, cross kNN and lists
 *                                     longer than 2 048 go row by row (every pair of those rows, as the reference does).
 *   SKL_KNN_TIES_CANONICAL            smallest (key, neighbour index) first: a property of the data alone.  The
 *                                     distance multiset of every row equals the reference's. */
#define SKL_KNN_TIES_CANONICAL 0
#define SKL_KNN_TIES_REFERENCE 1
int skl_ctx_set_knn_ties(skl_ctx *ctx, int mode);

/* Diagnostic (no reference counterpart): the early break of the core/accessory calls.  core_acc_dist leaves its loop over
 * the k-mer lengths at the first one whose ln J lies below the tolerance -- a pair that shares no more bins than chance,
 * expected_samebits (src/distances/jaccard.rs:26-31, :89-91) -- and a fit over fewer than three lengths is (1, 1) (:117).
 * With three to eight lengths the dense calls therefore count only the first two to four for the pairs of a BLOCK of the
 * pair space and complete the pairs still in the running afterwards, grouped by row (csrc/epilogue.hip) -- where a sample
 * of the block's pairs, taken the first time a slab meets a column slab, says that pays (between unrelated genomes ~1 % of
 * the pairs stay in the running at 4 096 bins, 0.2 % at 2 048; between close relatives all of them: such blocks count every
 * length as before).  With or without a completeness correction, any sketch size.  Same (core, acc) bit for bit either way.
 * pairs: pairs of the early-break launches since the context was made; completed_one_by_one: those among them that were
 * still in the running (counter wraps at 2^32).  Either argument may be null.  (The A/B build reads SKL_EARLY_BREAK=0: off.) */
int skl_ctx_early_break_stats(skl_ctx *ctx, uint64_t *pairs, uint64_t *completed_one_by_one);
/* ... and what the last dense core/accessory call of the context decided: the pair space is cut into blk_rows x blk_cols blocks
 * of (row sample >> shift_rows, column sample >> shift_cols); pooled_lengths = the k-mer lengths counted when all blocks agree
 * (0: every length, no early break); mixed = 1 when they do not, and block_lengths[r * blk_cols + c] (capacity >= blk_rows x
 * blk_cols bytes) then holds each block's count (nk: every length).  Any pointer may be null.  Reference behaviour matched:
 * the per-pair `break` of jaccard.rs:89-91 -- the result never depends on the decision, only the time does. */
int skl_ctx_early_break_blocks(skl_ctx *ctx, uint32_t *blk_rows, uint32_t *blk_cols, uint32_t *shift_rows, uint32_t *shift_cols,
                               int *pooled_lengths, int *mixed, uint8_t *block_lengths, size_t capacity);

/* Diagnostic (no reference counterpart): the unit table of the chunk-split pair kernel.  What each workgroup of a k-sliced
 * launch computes -- its tile, k-mer length, chunk range -- is a function of the launch's shape alone; the dense calls' launches
 * of up to 65 536 workgroups read it from a table of 16-byte descriptors that the host builds once per shape and the context
 * keeps (the last four shapes), instead of decoding the workgroup index in every wave.  Same results bit for bit either way.
 * last_launch_read_one: 1 when the context's last pair-kernel launch read such a table, 0 when it decoded in the kernel;
 * hits / builds: launches since the context was made that found their table in the cache / had it built and uploaded.  Any
 * pointer may be null.
 * skl_ctx_set_unit_table chooses the path for the context's later launches: SKL_UNIT_TABLE_BY_RULE (default) as above,
 * SKL_UNIT_TABLE_NEVER the decode in the kernel everywhere, SKL_UNIT_TABLE_ALWAYS every launch whose form allows a table, the kNN
 * drivers' bands included (tests and A/B timing; a table is then built for every new band shape). */
#define SKL_UNIT_TABLE_BY_RULE (-1)
#define SKL_UNIT_TABLE_NEVER 0
#define SKL_UNIT_TABLE_ALWAYS 1
int skl_ctx_unit_table(skl_ctx *ctx, int *last_launch_read_one, uint64_t *hits, uint64_t *builds);
int skl_ctx_set_unit_table(skl_ctx *ctx, int mode);

/* Diagnostic (no reference counterpart): tile pruning of the last skl_self_dists_knn / _partial call of the context.  The
 * whole-matrix self kNN with single-k keys (Jaccard / ANI, no completeness correction) leaves a 32 x 128 tile of the pair
 * space unfinished once every pair of it is, on the bins compared so far, already beyond both its samples' current knn-th
 * best (the key is monotone in the mismatch count).  The neighbour lists are those of the unpruned run in
 * either tie rule.  tiles: tiles of the launches that could prune; tiles_pruned: those left early -- most of them by a probe
 * over two of the fourteen planes before the walk begins (no stage walked), the rest at a stage boundary of the walk;
 * stages_per_tile: stage boundaries of a whole tile's walk (4 chunks each); stages_walked_in_pruned_tiles: how many of them
 * the pruned tiles had walked when they left (so the share of the pair space's full bin comparisons actually made is known);
 * tiles_sparse: tiles the probe could NOT dismiss but in which at most 4 rows held a pair still in the running -- typically one
 * relative among the tile's 4 096 pairs -- and whose walk was made for those rows only (every other pair of the tile gets the
 * worst key there is: it lies beyond both its samples' bounds, like a pruned tile's pairs).  Any argument may be null.  (The A/B
 * build of the library reads SKL_KNN_PRUNE=0: every tile walked, same lists; SKL_KNN_SPARSE=0: survivors walked whole.) */
int skl_ctx_knn_prune_stats(skl_ctx *ctx, uint64_t *tiles, uint64_t *tiles_pruned, uint64_t *stages_per_tile,
                            uint64_t *stages_walked_in_pruned_tiles, uint64_t *tiles_sparse);

/* self_dists_knn (src/distances/mod.rs:133-224); requires 1 <= knn < n. */
int skl_self_dists_knn(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t knn,
                       uint64_t *out_idx, float *out_d0, float *out_d1, int out_on_device);
int skl_self_dists_knn_rows(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p,
                            size_t knn, size_t row_begin, size_t row_end, uint64_t *out_idx,
                            float *out_d0, float *out_d1, int out_on_device);
/* self_dists_knn split over several devices with every pair evaluated ONCE (the reference
 * evaluates (i, j) and (j, i), mod.rs:148-171; distances are symmetric).  The rows are cut into
 * bands of band_rows samples (skl_knn_band_rows gives a size every participant agrees on); a
 * participant takes a subset of the bands (ascending band indices; deal them so that costs
 * balance: band b costs ~ n - b*band_rows) and gets back, for ALL n rows, the knn best
 * candidates seen in its share: state_key = order-preserving u32 image of the f32 key (empty
 * entries 0xFFFFFFFF), state_idx = neighbour, state_d1 = accessory distance (CoreAcc only, may
 * be NULL otherwise), each [n][knn], sorted ascending per row.  The participants then exchange
 * row shards of these states (an all-to-all: the one data-path collective of this library) and
 * skl_knn_merge_states turns the n_states partial states of a row shard -- stacked
 * [n_states][rows][knn] -- into the rows of skl_self_dists_knn's output.
 * Returns SKL_ERR_INVALID_ARG when the configuration has no one-evaluation form (CoreAcc with more than 6
 * k-mer lengths or sketchsize64 > 1023; knn > 2 048): shard rows with skl_self_dists_knn_rows then; and in the reference
 * tie order (partial heaps do not merge): use skl_self_dists_knn_window below. */
size_t skl_knn_band_rows(const skl_sketches *s, const skl_dist_params *p, size_t n_participants);
int skl_self_dists_knn_partial(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t knn,
                               size_t band_rows, const uint32_t *bands, size_t n_bands,
                               uint32_t *state_key, uint32_t *state_idx, float *state_d1, int out_on_device);
int skl_knn_merge_states(skl_ctx *ctx, size_t n_states, size_t rows, size_t knn, const uint32_t *state_key,
                         const uint32_t *state_idx, const float *state_d1, int states_on_device, int ani,
                         uint64_t *out_idx, float *out_d0, float *out_d1, int out_on_device);

/* self_dists_knn in the REFERENCE's tie order over several devices, every pair evaluated once: the column-window pipeline.
 * A row's BinaryHeap must meet its candidates in ascending id (mod.rs:156-181), so partial heaps of disjoint candidate sets
 * cannot be merged -- but a heap can travel.  Participant r owns the column window [lo_r, hi_r) (windows ascending with r;
 * cut them at n * sqrt(r / R) so that the pair counts balance, ROUNDED TO BAND BOUNDARIES: col_lo and col_hi must be multiples
 * of band_rows -- col_hi may also be n -- or the call fails with SKL_ERR_INVALID_ARG: a window starting inside a band would
 * lose candidates; so every cut but the last lies at or below n rounded down to a band boundary, and participants between
 * that cut and n get the EMPTY window [cut, cut)) and, for every row band b = rows [b * band_rows, ...) that
 * starts below hi_r, in ascending order, calls skl_self_dists_knn_window: the band's rows take the columns
 * [max(band start, lo_r), hi_r) as candidates, the window's rows below the band take the band's samples.  Before a band
 * whose rows lie below lo_r, participant r receives those rows' heaps from participant r - 1 (which has finished that band);
 * after any band it sends the band's rows on to r + 1; the last participant ends up with every row's final heap
 * (skl_knn_heaps_finalize).  Rows of a participant's own window start empty (skl_knn_heaps_clear).  The heap arrays are the
 * caller's (device memory): h_key f32 / h_id u32 / h_d1 f32 (CoreAcc only) [n][knn] in heap order, h_len u32 [n], thr u32 [n]
 * (order-preserving image of the heap's maximum once it is full, 0xFFFFFFFF before).  Tile pruning applies as in the
 * single-device call.  An empty window (col_lo == col_hi <= n, aligned or not) holds no pair: the call (and the _logged one
 * below) returns SKL_OK at once, launches nothing and leaves the heaps and logs as they are.
 * sketchlib.rust_amd/multi_gpu.py (self_knn_once_reference) is the driver over torch.distributed. */
int skl_self_dists_knn_window(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t knn,
                              size_t band_rows, size_t band, size_t col_lo, size_t col_hi,
                              float *h_key, uint32_t *h_id, float *h_d1, uint32_t *h_len, uint32_t *thr);
int skl_knn_heaps_clear(skl_ctx *ctx, size_t row_begin, size_t row_end, uint32_t *h_len, uint32_t *thr);
/* The same pipeline DECOUPLED (round 6): no participant waits for another.  A BinaryHeap that starts EMPTY on a window takes a
 * superset of what the row's true heap (the one that has met every earlier window) would take there -- its maximum is never
 * lower, and push_heap pushes on `key < maximum` (mod.rs:41-48).  So every participant clears ALL its heaps, runs its window
 * band by band with skl_self_dists_knn_window_logged, which also appends every candidate a heap takes to the row's ACCEPT LOG,
 * in order: log_rec [n][log_cap] records of 1 float (the key) or 2 (CoreAcc: key, second distance), log_id [n][log_cap],
 * log_len [n] (zeroed by the caller; it counts past log_cap -- an overflowed row's log is useless and the caller falls back
 * to the travelling heaps; random candidate order takes ~knn (1 + ln(window / knn)) entries).  The row's true list is then
 * skl_knn_heaps_replay of the participants' logs for that row in WINDOW ORDER into one empty heap (rows: the pointers are at
 * the first of them; logs of participants that own no column of a row's candidates are empty), then skl_knn_heaps_finalize.
 * Exactness: a candidate missing from a log was refused by a heap whose maximum was at least the true heap's.  What it
 * costs: tile pruning sees only the window's own relatives (scripts/knn_pipeline_model.py). */
int skl_self_dists_knn_window_logged(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t knn,
                                     size_t band_rows, size_t band, size_t col_lo, size_t col_hi,
                                     float *h_key, uint32_t *h_id, float *h_d1, uint32_t *h_len, uint32_t *thr,
                                     float *log_rec, uint32_t *log_id, uint32_t *log_len, size_t log_cap);
int skl_knn_heaps_replay(skl_ctx *ctx, size_t rows, size_t knn, int coreacc, const float *log_rec, const uint32_t *log_id,
                         const uint32_t *log_len, size_t log_cap, float *h_key, uint32_t *h_id, float *h_d1, uint32_t *h_len,
                         uint32_t *thr);
/* For callers without a device runtime of their own (the C++ host layer sees only this header): device memory on the
 * context's device for the heap arrays above, and copies between it and host memory (to_device != 0: host -> device),
 * ordered with the context's stream and complete on return. */
int skl_device_malloc(skl_ctx *ctx, size_t bytes, void **out);
int skl_device_free(skl_ctx *ctx, void *ptr);
int skl_device_memcpy(skl_ctx *ctx, void *dst, const void *src, size_t bytes, int to_device);
int skl_ctx_get_knn_ties(const skl_ctx *ctx);   /* SKL_KNN_TIES_* of the context */
/* into_sorted_vec of `rows` heaps (the arrays point at the first of them) -> rows of skl_self_dists_knn's output; device pointers. */
int skl_knn_heaps_finalize(skl_ctx *ctx, size_t rows, size_t knn, const float *h_key, const uint32_t *h_id, const float *h_d1,
                           const uint32_t *h_len, int ani, uint64_t *out_idx, float *out_d0, float *out_d1);

/* Assembling a dense matrix that several devices of ONE process computed in row bands (skl_self_dists_rows /
 * skl_cross_dists_rows with device outputs) on the first context's device, over xGMI: "the N x N pair space block-partitioned
 * across the GPUs of one node with a RCCL gather to assemble the output matrix" (the reference has one address space and no
 * counterpart).  ctxs[d] made band_dev[d] (band_bytes[d] bytes, device memory of ITS device, produced on ITS stream); the bands
 * land at dst_dev_root + dst_offsets[d] on ctxs[0]'s device: the root's own band by a copy inside its HBM, the others by
 * grouped ncclSend / ncclRecv in messages of at most 1 GiB, each send behind the kernels of its context's stream, the receives
 * on the root's stream.  Asynchronous: skl_ctx_synchronize(ctxs[0]) completes it.  One context per device (RCCL takes one rank
 * per device: a device listed twice is SKL_ERR_INVALID_ARG).  librccl.so.1 is looked up at run time; the communicators of a
 * device list are made once per process.  loopback_through_rccl != 0 with ONE context sends that band to itself through RCCL
 * (what a one-GPU box can test of the transport).  The torch.distributed rendering (one process per GPU) is
 * sketchlib.rust_amd/multi_gpu.py. */
int skl_gather_bands_rccl(skl_ctx *const *ctxs, size_t n_ctx, const void *const *band_dev, const size_t *band_bytes,
                          void *dst_dev_root, const size_t *dst_offsets, int loopback_through_rccl);

/* The same with the candidate lists built on the device as well: skq holds the index sketch
 * (u16 bins, `.skq` layout [sample][sketch_size]) of every sample of `s`, row i = sample i (the
 * caller applies the .ski -> .skd order map); candidates of i = samples sharing at least one
 * bin value at the same position, i excluded (Inverted::any_shared_bins, inverted.rs:259-268).
 * At most 1 294 336 samples per call (an n-bit bitmap per row lives in LDS).
 * out_n_candidates (nullable): total number of candidate pairs found. */
size_t skl_shared_bins_max_samples(void);
int skl_self_dists_knn_shared_bins(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p,
                                   size_t knn, const uint16_t *skq, size_t sketch_size,
                                   uint64_t *out_idx, float *out_d0, uint64_t *out_n_candidates);

/* ---- inverted query (src/inverted.rs:229-269): Inverted::query_against_inverted_index, all_shared_bins,
 *      any_shared_bins for many queries at once ----
 * An index held on the device: `bins` is the dense form of a `.ski` ([n_samples][sketch_size] u16, the `.skq`
 * layout, row = .ski sample index; a .ski written by `inverted build` holds exactly one value per (sample, bin)).
 * count(q, s) = #{ b : bins[s][b] == query_bins[q][b] }; the query is NOT excluded.
 *   SKL_INVQ_MATCH_COUNT: out = u32 [n_queries][n_samples], the counts (query_against_inverted_index, :229-241)
 *   SKL_INVQ_ANY_BINS:    out = u64 [n_queries][ceil(n_samples / 64)], bit s % 64 of word s / 64 set iff count > 0
 *                         (any_shared_bins, :259-268)
 *   SKL_INVQ_ALL_BINS:    the same bitmap, bit set iff count == sketch_size (all_shared_bins, :243-257)
 * Host pointers.  Queries run in bands sized by a device-memory budget (SKL_INVQ_BAND_BYTES, default 1 GiB), so
 * n_queries x n_samples never has to fit at once; skl_inverted_band_queries tells how many queries one band takes.
 * Destroy an index before its context.  At most 2^32 - 257 samples per index. */
typedef struct skl_inverted skl_inverted;
#define SKL_INVQ_MATCH_COUNT 0
#define SKL_INVQ_ANY_BINS 1
#define SKL_INVQ_ALL_BINS 2
int skl_inverted_create(skl_ctx *ctx, const uint16_t *bins, size_t n_samples, size_t sketch_size, skl_inverted **out);
int skl_inverted_destroy(skl_inverted *ix);
int skl_inverted_query(skl_ctx *ctx, const skl_inverted *ix, const uint16_t *query_bins, size_t n_queries, int mode,
                       void *out);
size_t skl_inverted_band_queries(skl_ctx *ctx, const skl_inverted *ix, int mode);

/* The best hits of every query (the reference's identification query, SketchlibData::query / get_probs,
 * src/lib.rs:1019-1109: match counts -> d / (2 S - d), a stable ascending sort, reverse(), the first nouts), selected on
 * the device behind the counts: hit r of a query is the indexed sample with the r-th largest key
 * (count << 32) | index compared as u64 -- counts descend and at equal count the HIGHER .ski index comes first, which
 * is what that sort-and-reverse gives.  out_ids / out_counts: u32 [n_queries][top], host pointers; with
 * n_eff = min(top, n_samples), entries [n_eff, top) of a row are id 0xFFFFFFFF, count 0 (an empty index: every entry).
 * Queries run in the bands of SKL_INVQ_MATCH_COUNT (skl_inverted_band_queries); a band's counts stay on the device
 * and n_queries x top x 8 bytes come back.  The hits of a query live in the workgroup's LDS: top is 1 to
 * SKL_INVQ_TOP_MAX, anything else is SKL_ERR_INVALID_ARG (not a slower path). */
#define SKL_INVQ_TOP_MAX 1024
int skl_inverted_query_top(skl_ctx *ctx, const skl_inverted *ix, const uint16_t *query_bins, size_t n_queries, size_t top,
                           uint32_t *out_ids, uint32_t *out_counts);

/* GPU sketching: bin minima of `canonical ntHash % SIGN_MOD` over every
 * valid k-mer of DNA samples -- Sketch::get_signs_no_densify (src/sketch/mod.rs:156-176) over
 * NtHashIterator (src/hashing/nthash_iterator.rs:325-523), all samples and k-mer lengths of a
 * batch in one launch.  `codes`: 2-bit base codes ((byte >> 1) & 3, hashing/mod.rs:82-85), one
 * byte per valid base, samples concatenated; sample s owns codes[code_begin[s] .. code_begin[s+1]).
 * `offsets`: for each sample the ascending positions (in its own code coordinates) of every
 * invalid base and record end (NtHashIterator::add_dna_seq, nthash_iterator.rs:205-251); a
 * window [p, p+k) is hashed iff no offset o has p < o < p+k.  out_signs: [n_samples][nk][num_bins]
 * u64, u64::MAX for an empty bin; densify_bin and the 14-plane transpose are the caller's
 * (they touch num_bins words, not the genome).  Host pointers. */
int skl_sketch_signs(skl_ctx *ctx, const uint8_t *codes, const uint64_t *code_begin,
                     const uint64_t *offsets, const uint64_t *offset_begin, size_t n_samples,
                     const size_t *kmers, size_t nk, uint64_t num_bins, int rc, uint64_t *out_signs);
/* The same with the bases already at 2 bits each -- what crosses PCIe either way (the one-byte form above is packed by the
 * library on host threads): `packed` holds, sample after sample, ceil(len / 16) little-endian u32 words per sample, code c of
 * the sample at bits 2 (c % 16) of its word c / 16, a sample's last word zero-padded; code_begin still counts CODES
 * (sample s has code_begin[s + 1] - code_begin[s] of them).  A caller that parses sequence files packs as it goes
 * (csrc/host/sketch_gpu.cpp).  Either form uploads batch i + 1 of the samples under the kernel of batch i. */
int skl_sketch_signs_packed(skl_ctx *ctx, const uint32_t *packed, const uint64_t *code_begin,
                            const uint64_t *offsets, const uint64_t *offset_begin, size_t n_samples,
                            const size_t *kmers, size_t nk, uint64_t num_bins, int rc, uint64_t *out_signs);

/* GPU sketching of amino-acid sequences: bin minima of `aaHash % SIGN_MOD` over every window of k valid
 * residues -- Sketch::get_signs_no_densify (src/sketch/mod.rs:156-176) over AaHashIterator
 * (src/hashing/aahash_iterator.rs:138-210), forward hash only, all samples and k-mer lengths of the call.
 * `residues`: one byte per STORED residue, a class code: 0 = separator (an invalid residue or a record end, the
 * reference's SEQSEP), 1..20 = the letters ACDEFGHIKLMNPQRSTVWY in this order (either case); anything above 20 is
 * refused.  Sample s owns residues[res_begin[s] .. res_begin[s+1]) (res_begin: n_samples + 1 entries, not decreasing).
 * There is no offsets array: a window [p, p+k) is hashed iff none of its k codes is 0.  `level` 1 / 2 / 3 chooses the
 * seed table (level 2 groups ST, DE, KQR, ILMV, FWY; level 3 also A with ST and N with DE).
 * concat_end_rule != 0 reproduces the reference's iterator at the end of a sample: it seeds a window only where
 * start < len - k, so the window at exactly len - k is hashed only when it is reached by rolling, i.e. when
 * len - k >= 1 and the residue at len - k - 1 is valid too.  A sample that ends in a separator (every sample sketched
 * without --concat-fasta) never shows the difference; concat_end_rule = 0 hashes every window of k valid residues.
 * out_signs: [n_samples][nk][num_bins] u64, u64::MAX for an empty bin -- a sample without a hashed window (empty,
 * shorter than k, all separators) comes back all-max and the error is the caller's to raise; densify_bin and the
 * 14-plane transpose are the caller's too.  Any k from 1 to 65 535 works (k above skl_sketch_aa_shape(3, 0) takes the
 * unstaged kernel for every sample).  The samples go in batches of whole samples of at most 256 MiB of signs
 * (SKL_AA_BATCH_SIGN_BYTES) and 256 Mi residues; short samples share workgroups (csrc/aa_plan.hpp).  Host pointers. */
int skl_sketch_signs_aa(skl_ctx *ctx, const uint8_t *residues, const uint64_t *res_begin, size_t n_samples,
                        const size_t *kmers, size_t nk, uint64_t num_bins, int level, int concat_end_rule,
                        uint64_t *out_signs);
/* Finishing (sample, k) streams of bin minima on the device: Sketch::densify_bin (src/sketch/mod.rs:237-258)
 * and the 14-plane transpose of fill_usigs (mod.rs:215-223), a workgroup per stream -- what a sketch file stores of a stream,
 * num_bins / 64 * 14 u64 words instead of num_bins u64 signs.  `signs`: [n_streams][num_bins] as skl_sketch_signs* return
 * them, u64::MAX for an empty bin.  out_usigs: [n_streams][num_bins / 64 * 14], word c * 14 + p = bit p of bins 64 c ..
 * 64 c + 63 after densification, byte for byte what the host loops give.  out_first_sign: [n_streams] the densified
 * signs[0] with all 64 bits (a read set's length estimate needs it), or null.  out_flags: [n_streams] bytes, bit 0
 * (SKL_FINISH_DENSIFIED) at least one bin was empty and filled from another; bit 1 (SKL_FINISH_EMPTY) EVERY bin is
 * u64::MAX -- the words are zeroed, the first sign is u64::MAX and the error is the caller's to raise, as the all-max
 * convention of skl_sketch_signs* leaves it (the reference's loop does not end on such a stream; the kernel never probes
 * it); bit 2 (SKL_FINISH_UNFINISHED) a bin needed more probes than the kernel's cap (2 048, csrc/finish_plan.hpp;
 * SKL_FINISH_MAX_ATTEMPTS overrides), so the library finished that stream on the host from its raw signs: the bytes are
 * the same, the flag only reports it.  num_bins must be a multiple of 64 (SKL_ERR_INVALID_ARG otherwise); up to 8 192
 * bins a stream's targets live in LDS, above that in device scratch -- any size is finished on the device.
 * SKL_SKETCH_FINISH=host finishes every stream on host threads instead (A/B timing, escape hatch).  Host pointers. */
#define SKL_FINISH_DENSIFIED 1
#define SKL_FINISH_EMPTY 2
#define SKL_FINISH_UNFINISHED 4
int skl_sketch_finish(skl_ctx *ctx, const uint64_t *signs, size_t n_streams, uint64_t num_bins, uint64_t *out_usigs,
                      uint64_t *out_first_sign, uint8_t *out_flags);
/* skl_sketch_signs_packed with every stream finished on the device: the finish launch follows each batch's bin-minimum
 * launch on the same stream and only the finished words cross PCIe (1 792 B per stream at 1 024 bins instead of 8 192 B).
 * out_usigs: [n_samples][nk][num_bins / 64 * 14] -- the layout of a sample's words in a .skd file; out_first_sign:
 * [n_samples][nk] or null; out_flags: [n_samples][nk], as skl_sketch_finish.  A sample without a valid k-mer of some
 * length comes back SKL_FINISH_EMPTY for that stream. */
int skl_sketch_usigs_packed(skl_ctx *ctx, const uint32_t *packed, const uint64_t *code_begin,
                            const uint64_t *offsets, const uint64_t *offset_begin, size_t n_samples,
                            const size_t *kmers, size_t nk, uint64_t num_bins, int rc, uint64_t *out_usigs,
                            uint64_t *out_first_sign, uint8_t *out_flags);
/* The u16 form of skl_sketch_finish, an inverted index's rows (`.skq`): densify_bin, then `sign as u16` per bin, for ANY
 * num_bins from 1 to 2^32 - 1 (an index has exactly sketch_size bins: 10, 1 000, ...).  The same kernel with another emit:
 * emptiness is decided on all 64 bits (a valid sign whose low 16 bits are 0xFFFF is not empty) and the resolve runs on
 * indices.  out_bins: [n_streams][num_bins]; out_flags as skl_sketch_finish (an all-empty stream: a zeroed row and
 * SKL_FINISH_EMPTY; a stream past the probe cap: finished on the host, the same bytes, SKL_FINISH_UNFINISHED set).
 * Batches, SKL_SKETCH_FINISH=host and SKL_FINISH_MAX_ATTEMPTS as there.  Host pointers. */
int skl_sketch_finish_u16(skl_ctx *ctx, const uint64_t *signs, size_t n_streams, uint64_t num_bins, uint16_t *out_bins,
                          uint8_t *out_flags);
/* skl_sketch_signs_packed at ONE k-mer length with the u16 finish behind each batch's bin-minimum launch, on the same
 * stream: 2 * num_bins bytes and a flag byte come home per sample instead of 8 * num_bins.  out_bins: [n_samples][num_bins];
 * out_flags: [n_samples].  A sample without a valid k-mer comes back SKL_FINISH_EMPTY (a zeroed row); the error is the
 * caller's to raise. */
int skl_sketch_bins_u16_packed(skl_ctx *ctx, const uint32_t *packed, const uint64_t *code_begin,
                               const uint64_t *offsets, const uint64_t *offset_begin, size_t n_samples,
                               size_t kmer, uint64_t num_bins, int rc, uint16_t *out_bins, uint8_t *out_flags);
/* skl_sketch_signs_aa with every stream finished on the device, batch by batch as that call cuts them; outputs as
 * skl_sketch_usigs_packed. */
int skl_sketch_usigs_aa(skl_ctx *ctx, const uint8_t *residues, const uint64_t *res_begin, size_t n_samples,
                        const size_t *kmers, size_t nk, uint64_t num_bins, int level, int concat_end_rule,
                        uint64_t *out_usigs, uint64_t *out_first_sign, uint8_t *out_flags);
/* Shapes of that call's two kernels: what = 0 window starts per thread of the staged form, 1 its threads per workgroup,
 * 2 most bins it keeps in LDS, 3 longest k-mer it takes, 4 residues from which a sample is staged (SKL_AA_LONG_MIN
 * overrides), 5 window starts per thread of the unstaged form when the longest k-mer is kmax, 6 its threads per
 * workgroup; -1 otherwise.  Needs no device. */
int skl_sketch_aa_shape(int what, size_t kmax);

/* Read sketching with a k-mer count filter.  The reference offers a window's sign to its count
 * filter only if the sign is below the current minimum of its bin (Sketch::bin_sign, src/sketch/mod.rs:198-210;
 * the filter: src/hashing/bloom_filter.rs), and a bin's minimum only ever falls.  So under any bin state the
 * caller has already reached -- however stale -- a window whose sign is >= its bin's value is never offered and
 * can be dropped; replaying only the other windows ("survivors") in stream order through the same filter gives
 * the reference's bins bit for bit.
 *
 * skl_reads_create uploads a batch of read sets once: `packed`, code_begin, offsets, offset_begin as for
 * skl_sketch_signs_packed, in the reference's padded two-file layout (nthash_iterator.rs:205-251: each file
 * starts on a multiple of 4 positions, codes cut at the number of valid bases; csrc/host/sketch.cpp
 * load_sample).  A window [p, p+k) is valid iff p + k <= the sample's code count and no offset o has
 * p < o < p+k.  Stream (s, ki) = sample s at kmers[ki], index s * nk + ki.
 *
 * skl_reads_survivors: for every stream, the valid windows with start in [win_begin[s], win_end[s]) whose
 * sign (canonical -- rc != 0 -- ntHash % SIGN_MOD) is strictly below thresholds[stream][bin], bin = sign /
 * ceil(SIGN_MOD / num_bins).  out_survivors[stream][0 .. capacity) receives (window start, sign) pairs in
 * no particular order; out_counts[stream] is the number of survivors, which may exceed capacity: the records
 * of such a stream are incomplete and the call must be repeated with capacity >= that count (nothing else
 * changes between the two calls).  Thresholds of all u64::MAX keep every valid window.  Host pointers.
 * Without a visible device skl_reads_create returns SKL_ERR_NO_DEVICE (pass ctx = NULL): there is no CPU path. */
typedef struct skl_reads skl_reads;
int skl_reads_create(skl_ctx *ctx, const uint32_t *packed, const uint64_t *code_begin, const uint64_t *offsets,
                     const uint64_t *offset_begin, size_t n_samples, const size_t *kmers, size_t nk,
                     uint64_t num_bins, int rc, skl_reads **out);
int skl_reads_survivors(skl_reads *r, const uint64_t *win_begin, const uint64_t *win_end,
                        const uint64_t *thresholds, uint64_t capacity, uint64_t *out_survivors,
                        uint64_t *out_counts);
int skl_reads_destroy(skl_reads *r);

/* Candidate-list form of skl_self_dists_knn: the device half of self_dists_knn_precluster
 * (src/distances/mod.rs:399-553).  Row i is compared only with the samples
 * cand[row_offsets[i] .. row_offsets[i+1]) (ascending sample ids, i itself excluded) -- what
 * Inverted::any_shared_bins (src/inverted.rs:259-268) returns for it.  Single-k Jaccard / ANI
 * only (the reference's CoreAcc arm is unimplemented!(), mod.rs:549-551).  Output as
 * skl_self_dists_knn, rows of fewer than knn candidates padded with (i, 1.0) (mod.rs:535-546).
 * All pointers are host pointers. */
int skl_self_dists_knn_candidates(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p,
                                  size_t knn, const uint64_t *row_offsets, const uint32_t *cand,
                                  uint64_t *out_idx, float *out_d0);

/* Distances of an explicit LIST of sample pairs: for every entry x the value the dense calls store for that pair --
 * core_acc_dist + simple_linear_regression (src/distances/jaccard.rs:61-142) as (core, acc), or the single-k Jaccard
 * distance / ANI (src/distances/mod.rs:83-100; what skl_self_dists_all stores, not the kNN key) -- at out[x * ncols ...),
 * ncols = 2 (core, acc interleaved) or 1.  Output position equals input position: the list is neither sorted nor
 * deduplicated, and any order, orientation and repeats are allowed.  Self form: both indices are samples of `s`, and an
 * entry with pair_a[x] == pair_b[x] gets the distance of a sample to itself ((0, 0); 0; ANI 1).  Cross form: pair_ref[x]
 * is a sample of `ref`, pair_query[x] one of `query`; a completeness correction applies when BOTH slabs carry a vector
 * (jaccard.rs:36).  Consecutive entries with the same first sample are evaluated together (its sketch is read once per 64
 * of them), so a list grouped by first sample -- the output of a kNN call -- is the cheap order; a shuffled list costs one
 * more record read per entry.  The lists are host pointers; they are uploaded and processed in bands of 64 Mi entries
 * (SKL_PAIRS_BAND).  An index >= the side's sample count is SKL_ERR_INVALID_ARG (the message names the entry) before
 * anything is launched or written; n_pairs == 0 is SKL_OK and touches nothing.  With out_on_device != 0 the results are in
 * place, and the stream idle, when the call returns.  Every k-mer count and sketch size the dense calls take. */
int skl_self_dists_pairs(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p,
                         const uint32_t *pair_a, const uint32_t *pair_b, size_t n_pairs,
                         float *out, int out_on_device);
int skl_cross_dists_pairs(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query, const skl_dist_params *p,
                          const uint32_t *pair_ref, const uint32_t *pair_query, size_t n_pairs,
                          float *out, int out_on_device);

/* cross_dists_knn (src/distances/mod.rs:306-395): rows = queries, neighbours
 * index refs; knn must already be clamped to <= n_ref (mod.rs:325).
 * Against 131 072 references or more (single-k keys, no completeness correction) the references reach a query in ascending
 * panels of columns and the tiles of the later panels are pruned against the queries' running lists, as in the self kNN
 * (skl_ctx_knn_prune_stats reports them): same lists in either tie rule, 16 384 x 1 M top-50 in 0.16 s instead of 0.36 s. */
int skl_cross_dists_knn(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query,
                        const skl_dist_params *p, size_t knn, uint64_t *out_idx, float *out_d0,
                        float *out_d1, int out_on_device);
int skl_cross_dists_knn_rows(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query,
                             const skl_dist_params *p, size_t knn, size_t query_begin,
                             size_t query_end, uint64_t *out_idx, float *out_d0, float *out_d1,
                             int out_on_device);

/* ---- raw bin-match counts (`samebits`, src/distances/jaccard.rs:15-25) ----
 * self: out[cond(i,j)*nk + k]; cross: out[(i_ref*n_query + j_query)*nk + k]. */
int skl_self_binmatch(skl_ctx *ctx, const skl_sketches *s, uint32_t *out, int out_on_device);
int skl_cross_binmatch(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query,
                       uint32_t *out, int out_on_device);

/* ---- one-shot forms: host pointers in, host pointers out; the argument lists
 *      of distances::self_dists_all / cross_dists_all flattened ---- */
int skl_self_dists_all_host(const uint64_t *bins, size_t n_samples, size_t nk,
                            const size_t *kmers, size_t sketchsize64,
                            const skl_dist_params *p, const double *completeness, float *out);
int skl_cross_dists_all_host(const uint64_t *ref_bins, size_t n_ref, const uint64_t *query_bins,
                             size_t n_query, size_t nk, const size_t *kmers, size_t sketchsize64,
                             const skl_dist_params *p, const double *ref_completeness,
                             const double *query_completeness, float *out);

#ifdef __cplusplus
}
#endif
#endif /* SKETCHLIB_DIST_H */
