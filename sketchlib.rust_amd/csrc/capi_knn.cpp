// capi_knn.cpp -- the sparse (k nearest neighbours) entry points of include/sketchlib_dist.h:
// row-by-row bands, the one-evaluation self kNN, its multi-GPU split and the merge of partial
// states.  Kernels: pair_kslice.hip (pair distances, turned second store), kernels.hip
// (topk_merge_kernel, merge_states_kernel).  Band heights, panels, the band driver's geometry and merges: knn_plan.hpp (pure).
#include "capi_internal.hpp"

#include <algorithm>
#include <cstring>

using namespace skl;

// ---------------------------------------------------------------------------
// sparse kNN: dense row bands into scratch, then a row-wise top-k kernel
// ---------------------------------------------------------------------------

// Running top-k states of a kNN call: (sortable key, sample id[, second value]) x knn per row.
namespace {
struct KnnState {
    uint32_t *key = nullptr, *idx = nullptr;
    float *d1 = nullptr;
    // Reference tie order (skl_ctx_set_knn_ties): the state of a row is the reference's BinaryHeap itself -- heap-ordered
    // (key, id[, second value]) arrays of h_len items -- and thr its maximum once full, in sortable bits
    // (refheap_merge_kernel, topk.hip).  Null in the canonical mode.
    float *h_key = nullptr, *h_d1 = nullptr;
    uint32_t *h_id = nullptr, *h_len = nullptr, *thr = nullptr;
    bool borrowed = false;   // the arrays belong to the caller (skl_self_dists_knn_window)
    // accept log of the heap replays (skl_self_dists_knn_window_logged; RefHeapMergeArgs::log_*), the caller's arrays
    float *log_rec = nullptr;
    uint32_t *log_id = nullptr, *log_len = nullptr;
    uint32_t log_cap = 0;
    ~KnnState()
    {
        if (borrowed) return;
        for (void *p : {(void *)key, (void *)idx, (void *)d1, (void *)h_key, (void *)h_d1, (void *)h_id, (void *)h_len, (void *)thr}) {
            if (p) (void)hipFree(p);
        }
    }
};
}  // namespace

// TILE-PRUNING COUNTERS (diagnostic): 1 024 slots of 4 words on the device (scratch slot SCRATCH_PRUNE_COUNTERS), added to by the pair kernels of
// every band of a call, read back LAZILY by skl_ctx_knn_prune_stats -- never on the launch path: the drivers that feed bands one
// call at a time (column windows, column panels) must not stall the host once per call.
static int prune_stats_reset(skl_ctx *ctx)
{
    ctx->knn_tiles = ctx->knn_tiles_sparse = ctx->knn_tiles_pruned = ctx->knn_tiles_probe_pruned = ctx->knn_pruned_stages = ctx->knn_tile_stages = 0;
    if (ctx->scratch[SCRATCH_PRUNE_COUNTERS] != nullptr) HIP_TRY(hipMemsetAsync(ctx->scratch[SCRATCH_PRUNE_COUNTERS], 0, 4096 * sizeof(uint32_t), ctx->stream));
    return SKL_OK;
}

static int prune_stats_collect(skl_ctx *ctx)
{
    if (ctx->scratch[SCRATCH_PRUNE_COUNTERS] == nullptr || !ctx->knn_prune_pending) return SKL_OK;
    std::vector<uint32_t> counted(4096, 0u);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->aux_stream) HIP_TRY(hipStreamSynchronize(ctx->aux_stream));
    HIP_TRY(hipMemcpy(counted.data(), ctx->scratch[SCRATCH_PRUNE_COUNTERS], counted.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    ctx->knn_tiles_pruned = ctx->knn_tiles_probe_pruned = ctx->knn_pruned_stages = ctx->knn_tiles_sparse = 0;
    for (size_t x = 0; x < 1024; ++x) {
        ctx->knn_tiles_pruned += (uint64_t)counted[4 * x] + counted[4 * x + 1];
        ctx->knn_tiles_probe_pruned += counted[4 * x];
        ctx->knn_pruned_stages += counted[4 * x + 2];
        ctx->knn_tiles_sparse += counted[4 * x + 3];
    }
    return SKL_OK;
}

static int knn_state_init(KnnState &st, size_t rows, size_t knn, bool coreacc, hipStream_t stream, bool ref_heap = false)
{
    const size_t items = rows * knn;
    if (ref_heap) {
        HIP_TRY(hipMalloc((void **)&st.h_key, items * sizeof(float)));
        HIP_TRY(hipMalloc((void **)&st.h_id, items * sizeof(uint32_t)));
        if (coreacc) HIP_TRY(hipMalloc((void **)&st.h_d1, items * sizeof(float)));
        HIP_TRY(hipMalloc((void **)&st.h_len, rows * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void **)&st.thr, rows * sizeof(uint32_t)));
        HIP_TRY(hipMemsetAsync(st.h_len, 0, rows * sizeof(uint32_t), stream));     // empty heaps
        HIP_TRY(hipMemsetAsync(st.thr, 0xFF, rows * sizeof(uint32_t), stream));    // not full: everything may enter
        return SKL_OK;
    }
    HIP_TRY(hipMalloc((void **)&st.key, items * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void **)&st.idx, items * sizeof(uint32_t)));
    if (coreacc) HIP_TRY(hipMalloc((void **)&st.d1, items * sizeof(float)));
    HIP_TRY(hipMemsetAsync(st.key, 0xFF, items * sizeof(uint32_t), stream));   // empty
    HIP_TRY(hipMemsetAsync(st.idx, 0xFF, items * sizeof(uint32_t), stream));
    return SKL_OK;
}

static_assert(PLAN_TOPK_LDS_MAX == TOPK_LDS_MAX && PLAN_REFHEAP_LDS_MAX == REFHEAP_LDS_MAX, "knn_plan.hpp restates these constants of kernels.h");

static bool knn_symmetric_ok(const skl_sketches *s, const skl_dist_params *p)
{
    return skl::knn_symmetric_ok(p->dist_type == SKL_DIST_COREACC, fused_coreacc_ok(s), forced_kernel(s->ctx));
}

static int knn_ani_undo(const skl_dist_params *p) { return (p->dist_type != SKL_DIST_COREACC && p->ani) ? 1 : 0; }

// The states of rows [r0, r1) -> the public output form (into_sorted_vec of the heaps / the sorted running lists as they are).
static int knn_finalize(const KnnState &st, size_t r0, size_t r1, size_t knn, const skl_dist_params *p, uint64_t *d_idx, float *d_d0,
                        float *d_d1, hipStream_t stream)
{
    const size_t o = r0 * knn;
    if (st.h_key != nullptr) {
        HIP_TRY(launch_refheap_finalize(st.h_key + o, st.h_id + o, st.h_d1 ? st.h_d1 + o : nullptr, st.h_len + r0, (uint32_t)(r1 - r0), (uint32_t)knn,
                                        knn_ani_undo(p), d_idx, d_d0, d_d1, stream));
    } else {
        HIP_TRY(launch_topk_finalize(st.key + o, st.idx + o, st.d1 ? st.d1 + o : nullptr, (r1 - r0) * knn, knn_ani_undo(p), d_idx, d_d0, d_d1, stream));
    }
    return SKL_OK;
}

// ---------------------------------------------------------------------------
// The band driver: knn_plan.hpp decides the geometry, the buffers' sizes, what a band is eligible for and its two merges;
// here the decision is executed.
// ---------------------------------------------------------------------------

// What the plan reads about one call of the band driver: rows of `s` against columns of `cs` (the same slab but for a cross
// panel), all columns and all rows -- a column window or a cross panel narrows win_* / row_* afterwards.
static KnnCall knn_call(const skl_ctx *ctx, const skl_sketches *s, const skl_sketches *cs, const skl_dist_params *p, KnnForm form,
                        size_t knn, size_t band_rows, size_t n_bands, bool overlap, const KnnState &st)
{
    KnnCall c;
    c.form = form;
    c.n_rows = s->n;
    c.n_cols = cs->n;
    c.band_rows = band_rows;
    c.knn = knn;
    c.win_hi = cs->n;
    c.row_hi = s->n;
    c.coreacc = p->dist_type == SKL_DIST_COREACC;
    c.ref = st.h_key != nullptr;
    c.overlap = overlap;
    c.nk = s->nk;
    c.ss64 = s->ss64;
    c.has_comp = s->d_comp != nullptr;
    c.fused_coreacc_ok = fused_coreacc_ok(s);
    c.forced_kernel = forced_kernel(ctx);
    c.n_bands = n_bands;
    c.knobs = ctx->knobs;
    return c;
}

// The scratch of a call: [2] = one per band buffer (the same one twice when bands do not overlap).
struct KnnBuffers {
    void *kband[2] = {nullptr, nullptr}, *tband[2] = {nullptr, nullptr};
    uint32_t *flags[2] = {nullptr, nullptr}, *row_bits[2] = {nullptr, nullptr}, *tbits[2] = {nullptr, nullptr};
    uint32_t *prune_q = nullptr, *prune_stats = nullptr;
    void *eb_counts[2] = {nullptr, nullptr};
};

static int knn_band_buffers(skl_ctx *ctx, const KnnCall &c, const KnnCallPlan &P, KnnBuffers &m)
{
    SKL_TRY(ctx_scratch(ctx, P.key_band_bytes, &m.kband[0], SCRATCH_KEY_BAND));
    if (P.turned) SKL_TRY(ctx_scratch(ctx, P.turned_band_bytes, &m.tband[0], SCRATCH_TURNED_BAND));
    m.kband[1] = m.kband[0];
    m.tband[1] = m.tband[0];
    if (c.overlap) {
        SKL_TRY(ctx_scratch(ctx, P.key_band_bytes, &m.kband[1], SCRATCH_KEY_BAND_2));
        if (P.turned) SKL_TRY(ctx_scratch(ctx, P.turned_band_bytes, &m.tband[1], SCRATCH_TURNED_BAND_2));
    }
    void *flag_mem = nullptr, *bits_mem = nullptr;
    SKL_TRY(ctx_scratch(ctx, P.flags_bytes, &flag_mem, SCRATCH_KNN_FLAGS));
    m.flags[0] = (uint32_t *)flag_mem;
    m.flags[1] = m.flags[0] + P.flags_half;
    HIP_TRY(hipMemsetAsync(flag_mem, 0, P.flags_bytes, ctx->stream));
    SKL_TRY(ctx_scratch(ctx, P.row_bits_bytes, &bits_mem, SCRATCH_KNN_ROW_BITS));
    m.row_bits[0] = (uint32_t *)bits_mem;
    m.row_bits[1] = m.row_bits[0] + P.row_bits_half;
    if (P.turned_bits_bytes) {
        void *tb = nullptr;
        SKL_TRY(ctx_scratch(ctx, P.turned_bits_bytes, &tb, SCRATCH_KNN_TURNED_BITS));
        m.tbits[0] = (uint32_t *)tb;
        m.tbits[1] = m.tbits[0] + P.turned_bits_half;
    }
    if (P.prune) {
        void *pq = nullptr, *ps = nullptr;
        SKL_TRY(ctx_scratch(ctx, P.prune_bounds_bytes, &pq, SCRATCH_PRUNE_BOUNDS));
        const bool fresh = ctx->scratch[SCRATCH_PRUNE_COUNTERS] == nullptr;
        SKL_TRY(ctx_scratch(ctx, 4096 * sizeof(uint32_t), &ps, SCRATCH_PRUNE_COUNTERS));
        m.prune_q = (uint32_t *)pq;
        m.prune_stats = (uint32_t *)ps;
        if (fresh) HIP_TRY(hipMemsetAsync(m.prune_stats, 0, 4096 * sizeof(uint32_t), ctx->stream));   // (afterwards: prune_stats_reset, at the start of a call)
        ctx->knn_prune_pending = true;
        if (c.cross()) HIP_TRY(hipMemsetAsync(m.prune_q + P.prune_cols_at, 0, (c.n_cols + 64) * sizeof(uint32_t), ctx->stream));   // the columns have no lists: bound 0
    }
    return SKL_OK;
}

// The early break's decision for the call and its counts buffers: *eb_lengths k-mer lengths counted (0: no early break).
// The counts kernel stays on the context's stream; the band's epilogue goes with the merges (the other stream when bands
// overlap): it is bound by memory and by the latency of the one-by-one completions, the counts kernel by the VALUs.
static int knn_early_break_buffers(skl_ctx *ctx, const skl_sketches *s, const skl_sketches *cs, const KnnCall &c, const KnnCallPlan &P,
                                   KnnBuffers &m, int *eb_lengths)
{
    *eb_lengths = 0;
    if (!P.eb_may_ask) return SKL_OK;
    SKL_TRY(early_break_lengths(ctx, s, cs, 1, eb_lengths));
    if (*eb_lengths <= 0) return SKL_OK;
    // (the band heights count these buffers in -- coreacc_rec_with_counts() -- but a band height the CALLER chose, or a
    // device short of memory, must not fail the call: without the counts the bands take the fused kernel as before)
    const size_t bytes = knn_eb_counts_bytes(c, *eb_lengths);
    int rc = ctx_scratch(ctx, bytes, &m.eb_counts[0], SCRATCH_COUNTS);
    ctx->clean_plane1 = nullptr;   // (the counts scratch holds another layout now)
    m.eb_counts[1] = m.eb_counts[0];
    if (rc == SKL_OK && c.overlap) rc = ctx_scratch(ctx, bytes, &m.eb_counts[1], SCRATCH_COUNTS_2);
    if (rc == SKL_ERR_OOM) {
        (void)hipGetLastError();   // (cleared: the call goes on)
        *eb_lengths = 0;
        return SKL_OK;
    }
    return rc;
}

// uint4 words of the lane slab before the 64-column block that starts at column col0
static size_t knn_lane_offset(const skl_sketches *s, size_t col0) { return (col0 / 64) * (s->nk * s->ss64 * 7 * 64); }

// The pair launch of band B into buffer `buf`: the view, the marks it leaves for the merges (cleared here) and, with tile
// pruning, every sample's bound as of now.
static int knn_pair_args(skl_ctx *ctx, const skl_sketches *s, const skl_sketches *cs, const skl_dist_params *p, const KnnCall &c,
                         const KnnCallPlan &P, const KnnBand &B, const KnnBuffers &m, int buf, const KnnState &st, PairArgs *out)
{
    PairArgs &g = *out;
    const size_t knn = c.knn;
    SKL_TRY(fill_args(s, cs, p, c.coreacc ? MODE_COREACC : MODE_JACCARD, c.coreacc ? 0 : (p->ani ? JOUT_ANI_KEY : JOUT_DIST), &g));
    g.B += knn_lane_offset(s, B.col0);
    g.nB = B.nB;
    if (g.compB) g.compB += B.col0;
    g.row_begin = (uint32_t)B.b0;
    g.row_end = (uint32_t)B.b1;
    g.self_mode = 0;
    g.out_base = (uint64_t)B.b0 * g.nB;
    g.out = m.kband[buf];
    g.out_t = B.has_turned ? (float *)m.tband[buf] : nullptr;
    g.t_col_begin = (uint32_t)(B.t_first - B.col0);
    g.t_stride = (uint32_t)P.t_stride;
    if (ctx->knobs.knn_row_flags) {
        HIP_TRY(hipMemsetAsync(m.row_bits[buf], 0, c.band_rows * P.bit_words * sizeof(uint32_t), ctx->stream));
        g.r_bits = m.row_bits[buf];
        g.r_bits_stride = (uint32_t)P.bit_words;
        g.r_thr = c.ref ? st.thr + B.b0 : st.key + B.b0 * knn + (knn - 1);        // knn-th best of sample b0 + r
        g.r_thr_stride = c.ref ? 1u : (uint32_t)knn;
    }
    if (g.out_t && ctx->knobs.knn_row_flags) {
        g.t_flag = m.flags[buf] + B.col0;                   // indexed by the view's column number, like t_col_begin
        g.t_flag_value = B.flag_value;
        g.t_thr = c.ref ? st.thr + B.col0 : st.key + B.col0 * knn + (knn - 1);      // knn-th best of sample col0 + c
        g.t_thr_stride = c.ref ? 1u : (uint32_t)knn;
        HIP_TRY(hipMemsetAsync(m.tbits[buf] + B.t_first * P.tbit_words, 0, (c.win_hi - B.t_first) * P.tbit_words * sizeof(uint32_t), ctx->stream));
        g.t_bits = m.tbits[buf] + B.col0 * P.tbit_words;
        g.t_bits_stride = (uint32_t)P.tbit_words;
    }
    if (P.prune) {
        // every sample's bound as of now (the merges of earlier bands may still be lowering thresholds: stale = too high = safe)
        HIP_TRY(launch_prune_thresholds(c.ref ? st.thr : st.key + (knn - 1), c.ref ? 1u : (uint32_t)knn, (uint32_t)c.n_rows, g.dtab,
                                        (uint32_t)(64 * s->ss64), m.prune_q, ctx->stream));
        g.prune_q_rows = m.prune_q;
        g.prune_q_cols = m.prune_q + P.prune_cols_at + B.col0;
        g.prune_stats = m.prune_stats;
        g.prune_flags = ctx->knobs.knn_sparse ? 0u : 1u;

        if (!g.t_bits) {   // (the last band has no turned copy; the kernel takes "both bit sets given" as the sign that the merges mask)
            g.t_bits = m.tbits[buf] + B.col0 * P.tbit_words;
            g.t_bits_stride = (uint32_t)P.tbit_words;
        }
        ctx->knn_tiles += B.tiles;
    }
    return SKL_OK;
}

// EARLY-BREAK band: the counts launch `cnt` over the view of the band's pair launch `g` (first eb_lengths k-mer lengths, u16
// records, k-major) and the epilogue `e` that turns them into g's records, marks and turned copy.
static int knn_early_break_args(skl_ctx *ctx, const skl_sketches *s, const skl_sketches *cs, const skl_dist_params *p, const PairArgs &g,
                                const KnnBand &B, int eb_lengths, void *counts, PairArgs *cnt, EpilogueKnnArgs *epi)
{
    const size_t pairs_view = (B.b1 - B.b0) * (size_t)g.nB;
    PairArgs &c = *cnt;
    SKL_TRY(fill_args(s, cs, p, MODE_COUNTS, 0, &c));
    c.B += knn_lane_offset(s, B.col0);
    c.nB = g.nB;
    c.row_begin = g.row_begin;
    c.row_end = g.row_end;
    c.self_mode = 0;
    c.out_base = g.out_base;
    c.k_count = (uint32_t)eb_lengths;
    c.cnt_pair_stride = 1;
    c.cnt_k_stride = pairs_view;
    c.k_sliced = 1;
    c.k_slices = 1;
    c.cnt_u16 = 1;
    c.out = counts;
    EpilogueKnnArgs &e = *epi;
    memset(&e, 0, sizeof e);
    e.counts = (const uint32_t *)counts;
    e.n_pairs = pairs_view;
    e.rows = (uint32_t)(B.b1 - B.b0);
    e.nB = g.nB;
    e.nk = (uint32_t)eb_lengths;
    e.nk_total = (uint32_t)s->nk;
    e.ss64 = (uint32_t)s->ss64;
    e.row_sample0 = (uint32_t)B.b0;
    e.col_sample0 = (uint32_t)B.col0;
    e.ytab = s->d_ytab;
    e.kf = s->d_kf;
    e.tolerance = g.tolerance;
    e.rows_ref = s->d_rows;
    e.cols_ref = cs->d_rows;
    e.out = (float *)g.out;
    e.r_thr = g.r_thr;
    e.r_thr_stride = g.r_thr_stride;
    e.r_bits = g.r_bits;
    e.r_bits_stride = g.r_bits_stride;
    e.out_t = g.out_t;
    e.t_col_begin = g.t_col_begin;
    e.t_stride = g.t_stride;
    e.t_thr = g.t_thr;
    e.t_thr_stride = g.t_thr_stride;
    e.t_flag = g.t_flag;
    e.t_flag_value = g.t_flag_value;
    e.t_bits = g.t_bits;
    e.t_bits_stride = g.t_bits_stride;
    e.alive_count = ctx->eb_counter;
    e.min_alive = s->min_alive;
    e.xcd_blocked = (uint32_t)ctx->knobs.knn_epi_blocked;
    e.cnt_u16 = 1;
    e.plain_marks_nothing = B.plain_marks_nothing ? 1u : 0u;
    return SKL_OK;
}

// Where a planned merge reads: the band buffer, the rows' flags and the marks of its records.
struct KnnMergeSource {
    const float *keys = nullptr;
    const uint32_t *flag = nullptr, *seg_bits = nullptr;
    uint32_t seg_bits_stride = 0;
};
static KnnMergeSource knn_merge_source(const skl_ctx *ctx, const KnnCallPlan &P, const KnnMerge &mg, const KnnBuffers &m, int buf)
{
    KnnMergeSource src;
    const bool marks = ctx->knobs.knn_row_flags;
    const size_t first = mg.state_row_base;   // (turned: row r of the launch = sample t_first + r)
    src.keys = (const float *)(mg.turned ? m.tband[buf] : m.kband[buf]);
    src.flag = mg.row_flags && marks ? m.flags[buf] + first : nullptr;
    src.seg_bits = !marks ? nullptr : (mg.turned ? m.tbits[buf] + first * P.tbit_words : m.row_bits[buf]);
    src.seg_bits_stride = (uint32_t)(mg.turned ? P.tbit_words : P.bit_words);
    return src;
}

// canonical ties: the sorted running lists
static int knn_merge_topk(const skl_ctx *ctx, const KnnCall &c, const KnnBand &B, const KnnMerge &mg, const KnnMergeSource &src,
                          const KnnState &st, hipStream_t stream)
{
    TopkMergeArgs m;
    memset(&m, 0, sizeof m);
    m.knn = (uint32_t)c.knn;
    m.stride2 = c.coreacc ? 2 : 1;
    m.run_key = st.key;
    m.run_idx = st.idx;
    m.run_d1 = st.d1;
    m.streaming = ctx->knobs.topk_stream;
    m.keys = src.keys;
    m.key_stride = mg.stride * m.stride2;
    m.rows = mg.rows;
    m.cols = mg.cols;
    m.id_base = mg.id_base;
    m.skip_below = mg.skip_below;
    m.state_row_base = mg.state_row_base;
    m.self_id_base = mg.self_id_base;
    m.flag = src.flag;
    m.flag_value = mg.row_flags ? B.flag_value : 0u;
    m.seg_bits = src.seg_bits;
    m.seg_bits_stride = src.seg_bits_stride;
    m.seg_shift = mg.seg_shift;
    HIP_TRY(launch_topk_merge(m, stream));
    return SKL_OK;
}

// reference ties: the heaps replayed
static int knn_merge_refheap(const skl_ctx *ctx, const KnnCall &c, const KnnBand &B, const KnnMerge &mg, const KnnMergeSource &src,
                             const KnnState &st, hipStream_t stream)
{
    RefHeapMergeArgs m;
    memset(&m, 0, sizeof m);
    m.knn = (uint32_t)c.knn;
    m.stride2 = c.coreacc ? 2 : 1;
    m.h_key = st.h_key;
    m.h_id = st.h_id;
    m.h_d1 = st.h_d1;
    m.h_len = st.h_len;
    m.thr = st.thr;
    m.log_rec = st.log_rec;
    m.log_id = st.log_id;
    m.log_len = st.log_len;
    m.log_cap = st.log_cap;
    m.force_workgroup_form = ctx->knobs.refheap_wave ? 0u : 1u;
    m.keys = src.keys;
    m.key_stride = mg.stride * m.stride2;
    m.rows = mg.rows;
    m.cols = mg.cols;
    m.id_base = mg.id_base;
    m.skip_below = mg.skip_below;
    m.state_row_base = mg.state_row_base;
    m.self_id_base = mg.self_id_base;
    m.flag = src.flag;
    m.flag_value = B.flag_value;
    m.seg_bits = src.seg_bits;
    m.seg_bits_stride = src.seg_bits_stride;
    m.seg_shift = mg.seg_shift;
    HIP_TRY(launch_refheap_merge(m, stream));
    return SKL_OK;
}

// The bands `bands` of call `c` (ascending indices) merged into the running states `st`: rows of `s` against columns of `cs`.
static int knn_run_bands(skl_ctx *ctx, const skl_sketches *s, const skl_sketches *cs, const skl_dist_params *p, const KnnCall &c,
                         const std::vector<uint32_t> &bands, KnnState &st)
{
    const KnnCallPlan P = plan_knn_call(c);
    const int mode = c.coreacc ? MODE_COREACC : MODE_JACCARD;
    KnnBuffers m;
    SKL_TRY(knn_band_buffers(ctx, c, P, m));
    hipStream_t topk_stream = c.overlap ? ctx->aux_stream : ctx->stream;
    if (c.overlap) {   // the states were cleared on the context's stream, the merges run on the other one
        HIP_TRY(hipEventRecord(ctx->knn_pair_done[0], ctx->stream));
        HIP_TRY(hipStreamWaitEvent(topk_stream, ctx->knn_pair_done[0], 0));
    }
    int eb_lengths = 0;
    SKL_TRY(knn_early_break_buffers(ctx, s, cs, c, P, m, &eb_lengths));
    size_t it = 0;
    for (const uint32_t band : bands) {
        const KnnBand B = plan_knn_band(c, P, band, it, eb_lengths);
        if (B.skip) continue;
        const RoctxRange range_("skl:knn_band pair kernel + merges (every pair once)");
        const int buf = c.overlap ? (int)(it & 1) : 0;
        if (c.overlap && it >= 2) HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->knn_topk_done[buf], 0));
        PairArgs g;
        SKL_TRY(knn_pair_args(ctx, s, cs, p, c, P, B, m, buf, st, &g));
        EpilogueKnnArgs e;
        if (B.eb_band) {
            PairArgs cnt;
            SKL_TRY(knn_early_break_args(ctx, s, cs, p, g, B, eb_lengths, m.eb_counts[buf], &cnt, &e));
            SKL_TRY(timed_pair_launch(ctx, cnt, MODE_COUNTS));
            ctx->eb_pairs += e.n_pairs;
            ctx->last_kernel += " + early break: " + std::to_string(eb_lengths) + " of " + std::to_string(s->nk) + " k-mer lengths counted, the pairs still in the running completed by the band's epilogue";
        } else {
            SKL_TRY(timed_pair_launch(ctx, g, mode));
        }
        if (c.overlap) {
            HIP_TRY(hipEventRecord(ctx->knn_pair_done[buf], ctx->stream));
            HIP_TRY(hipStreamWaitEvent(topk_stream, ctx->knn_pair_done[buf], 0));
        }
        if (B.eb_band) {   // counts -> records, marks, turned copy: with the merges, behind the counts kernel
            if (g.out_t != nullptr) {   // (1, 1): every pair that left the loop before its third length
                HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)m.tband[buf], 0x3F800000, (c.win_hi - B.t_first) * P.t_stride * 2, topk_stream));
            }
            HIP_TRY(launch_coreacc_epilogue_knn(e, topk_stream));
        }
        for (const KnnMerge &mg : B.merge) {
            const KnnMergeSource src = knn_merge_source(ctx, P, mg, m, buf);
            SKL_TRY(c.ref ? knn_merge_refheap(ctx, c, B, mg, src, st, topk_stream) : knn_merge_topk(ctx, c, B, mg, src, st, topk_stream));
        }
        if (c.overlap) HIP_TRY(hipEventRecord(ctx->knn_topk_done[buf], topk_stream));
        ++it;
    }
    if (P.prune) ctx->knn_tile_stages = (s->ss64 + 3) / 4;   // stages of a whole 32 x 128 tile: 4 waves, one chunk each per stage
    if (c.overlap && it) {   // the states (and the band buffers) belong to the context's stream again
        HIP_TRY(hipEventRecord(ctx->knn_topk_done[0], topk_stream));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->knn_topk_done[0], 0));
    }
    return SKL_OK;
}

static int knn_self_symmetric(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t knn,
                              size_t band_rows, bool overlap, uint64_t *d_idx, float *d_d0, float *d_d1)
{
    const size_t n = s->n;
    const bool ref = ctx->knn_ties == SKL_KNN_TIES_REFERENCE;
    KnnState st;
    SKL_TRY(knn_state_init(st, n, knn, p->dist_type == SKL_DIST_COREACC, ctx->stream, ref));
    std::vector<uint32_t> bands((n + band_rows - 1) / band_rows);
    for (size_t b = 0; b < bands.size(); ++b) bands[b] = (uint32_t)b;
    SKL_TRY(knn_run_bands(ctx, s, s, p, knn_call(ctx, s, s, p, KNN_SYMMETRIC, knn, band_rows, bands.size(), overlap, st), bands, st));
    SKL_TRY(knn_finalize(st, 0, n, knn, p, d_idx, d_d0, d_d1, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // the running states are freed on return
    return SKL_OK;
}

// Row-by-row kNN: dense bands of records into scratch, then a per-row top-k.  With two bands
// the top-k of band i (memory / LDS bound, on the auxiliary stream) runs while the pair kernel
// of band i + 1 (VALU bound) fills the other one.  The top-k is the streaming one of the
// symmetric driver (topk_merge_kernel), fed a whole row at once.
static int knn_rows_banded(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cands,
                           const skl_dist_params *p, const KnnRowsCall &rc, size_t band_rows, bool overlap,
                           uint64_t *d_idx, float *d_d0, float *d_d1)
{
    const size_t knn = rc.knn, r0 = rc.r0, r1 = rc.r1;
    const int self_mode = rc.self_mode ? 1 : 0;
    const bool coreacc = rc.coreacc;
    const int mode = coreacc ? MODE_COREACC : MODE_JACCARD;
    const int jout = coreacc ? 0 : (p->ani ? JOUT_ANI_KEY : JOUT_DIST);
    const size_t rec = coreacc ? 2 * sizeof(float) : sizeof(float);
    const size_t n_cand = cands->n;
    void *band[2] = {nullptr, nullptr};
    SKL_TRY(ctx_scratch(ctx, band_rows * n_cand * rec, &band[0], SCRATCH_KEY_BAND));
    band[1] = band[0];
    if (overlap) SKL_TRY(ctx_scratch(ctx, band_rows * n_cand * rec, &band[1], SCRATCH_KEY_BAND_2));
    hipStream_t topk_stream = overlap ? ctx->aux_stream : ctx->stream;
    // Three ways from a band of records to neighbour lists:
    //   * the streaming running top-k (topk_merge_kernel) + finalize: canonical ties, knn <= TOPK_LDS_MAX;
    //   * the radix select with its items in global memory (topk_kernel, dense form): canonical ties, any knn;
    //   * the BinaryHeap replay (topk_refheap_kernel): the reference binary's tie order, any knn.
    const bool ref_ties = ctx->knn_ties == SKL_KNN_TIES_REFERENCE;
    const bool big = knn > (size_t)TOPK_LDS_MAX;
    const bool streaming_state = !ref_ties && !big;
    // COLUMN PANELS (knn_plan.hpp plan_knn_panels): the candidates in ascending panels of columns, each a call of the band driver
    const KnnPanels panels = plan_knn_panels(rc, band_rows);
    if (panels.eligible) {
        KnnState pst;
        SKL_TRY(knn_state_init(pst, rows->n, knn, false, ctx->stream, ref_ties));
        std::vector<uint32_t> bands;
        for (size_t b = r0 / panels.rows_per; b * panels.rows_per < r1; ++b) bands.push_back((uint32_t)b);
        KnnCall call = knn_call(ctx, rows, cands, p, KNN_CROSS_PANEL, knn, panels.rows_per, bands.size(), overlap && bands.size() > 1, pst);
        call.self_rows = self_mode != 0;
        call.row_lo = r0;
        call.row_hi = r1;
        SKL_TRY(prune_stats_reset(ctx));
        for (size_t c0 = 0; c0 < n_cand; c0 += panels.panel) {
            call.win_lo = c0;
            call.win_hi = std::min(n_cand, c0 + panels.panel);
            SKL_TRY(knn_run_bands(ctx, rows, cands, p, call, bands, pst));
        }
        SKL_TRY(knn_finalize(pst, r0, r1, knn, p, d_idx, d_d0, d_d1, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));   // the running states are freed on return
        return SKL_OK;
    }
    KnnState st;
    DevBuf big_scratch;
    if (streaming_state) {
        SKL_TRY(knn_state_init(st, r1 - r0, knn, coreacc, ctx->stream));
    } else if (ref_ties && knn > (size_t)REFHEAP_LDS_MAX) {
        HIP_TRY(hipMalloc(&big_scratch.p, band_rows * 3 * (knn + 1) * sizeof(float)));
    } else if (!ref_ties && big) {
        HIP_TRY(hipMalloc(&big_scratch.p, band_rows * topk_items_pitch(knn) * sizeof(uint64_t)));
    }
    if (overlap) {   // the states are cleared on the context's stream, the merges run on the other one
        HIP_TRY(hipEventRecord(ctx->knn_pair_done[0], ctx->stream));
        HIP_TRY(hipStreamWaitEvent(topk_stream, ctx->knn_pair_done[0], 0));
    }

    size_t it = 0;
    for (size_t b0 = r0; b0 < r1; b0 += band_rows, ++it) {
        const size_t b1 = std::min(r1, b0 + band_rows);
        const RoctxRange range_("skl:knn_band pair kernel + top-k (row by row)");
        const int buf = overlap ? (int)(it & 1) : 0;
        // the top-k that read this buffer two bands ago must be done before it is overwritten
        if (overlap && it >= 2) HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->knn_topk_done[buf], 0));
        SKL_TRY(dense_band(ctx, rows, cands, p, mode, jout, 0, b0, b1, band[buf]));
        if (overlap) {
            HIP_TRY(hipEventRecord(ctx->knn_pair_done[buf], ctx->stream));
            HIP_TRY(hipStreamWaitEvent(topk_stream, ctx->knn_pair_done[buf], 0));
        }
        const size_t o = (b0 - r0) * knn;   // first output item of the band
        const int ani_undo = knn_ani_undo(p);
        if (streaming_state) {
            TopkMergeArgs m;
            memset(&m, 0, sizeof m);
            m.knn = (uint32_t)knn;
            m.stride2 = coreacc ? 2 : 1;
            m.run_key = st.key;
            m.run_idx = st.idx;
            m.run_d1 = st.d1;
            m.streaming = ctx->knobs.topk_stream;
            m.key_stride = (uint64_t)n_cand * m.stride2;
            m.rows = (uint32_t)(b1 - b0);
            m.self_id_base = self_mode ? (uint32_t)b0 : 0xFFFFFFFFu;
            m.state_row_base = (uint32_t)(b0 - r0);
            m.keys = (const float *)band[buf];
            m.cols = (uint32_t)n_cand;
            m.id_base = 0;
            HIP_TRY(launch_topk_merge(m, topk_stream));
        } else if (ref_ties) {
            RefHeapArgs h;
            memset(&h, 0, sizeof h);
            h.keys = (const float *)band[buf];
            h.stride2 = coreacc ? 2 : 1;
            h.key_stride = (uint64_t)n_cand * h.stride2;
            h.rows = (uint32_t)(b1 - b0);
            h.cols = (uint32_t)n_cand;
            h.self_id_base = self_mode ? (uint32_t)b0 : 0xFFFFFFFFu;
            h.knn = (uint32_t)knn;
            h.ani_undo = ani_undo;
            h.out_idx = d_idx + o;
            h.out_d0 = d_d0 + o;
            h.out_d1 = coreacc ? d_d1 + o : nullptr;
            h.heap_scratch = (float *)big_scratch.p;
            h.force_workgroup_form = ctx->knobs.refheap_wave ? 0u : 1u;
            HIP_TRY(launch_topk_refheap(h, topk_stream));
        } else {
            TopkArgs t;
            memset(&t, 0, sizeof t);
            t.keys = (const float *)band[buf];
            t.rows = (uint32_t)(b1 - b0);
            t.cols = (uint32_t)n_cand;
            t.stride2 = coreacc ? 2 : 1;
            t.knn = (uint32_t)knn;
            t.self_mode = self_mode;
            t.row_begin = (uint32_t)b0;
            t.ani_undo = ani_undo;
            t.out_idx = d_idx + o;
            t.out_d0 = d_d0 + o;
            t.out_d1 = coreacc ? d_d1 + o : nullptr;
            t.items_scratch = (uint64_t *)big_scratch.p;
            t.items_pitch = topk_items_pitch(knn);
            HIP_TRY(launch_topk(t, topk_stream));
        }
        if (overlap) HIP_TRY(hipEventRecord(ctx->knn_topk_done[buf], topk_stream));
    }
    if (streaming_state) SKL_TRY(knn_finalize(st, 0, r1 - r0, knn, p, d_idx, d_d0, d_d1, topk_stream));
    if (overlap) {   // results (and the band buffers) belong to the context's stream again
        HIP_TRY(hipEventRecord(ctx->knn_topk_done[0], topk_stream));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->knn_topk_done[0], 0));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // the running states are freed on return
    return SKL_OK;
}

static int knn_rows(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cands,
                    const skl_dist_params *p, size_t knn, int self_mode, size_t r0, size_t r1,
                    uint64_t *out_idx, float *out_d0, float *out_d1, int out_on_device)
{
    SKL_TRY(ctx_bind(ctx));
    if (!out_idx || !out_d0) return fail(SKL_ERR_INVALID_ARG, "output pointers are null");
    const bool coreacc = p->dist_type == SKL_DIST_COREACC;
    if (coreacc && !out_d1) return fail(SKL_ERR_INVALID_ARG, "out_d1 is required for core/accessory");
    if (r0 > r1 || r1 > rows->n) return fail(SKL_ERR_INVALID_ARG, "row range out of bounds");
    const size_t n_cand = cands->n;
    const size_t max_knn = n_cand > (size_t)(self_mode ? 1 : 0) ? n_cand - (self_mode ? 1 : 0) : 0;
    if (knn == 0 || knn > max_knn) {
        return fail(SKL_ERR_INVALID_ARG, "knn=%zu must be in [1, %zu]", knn, max_knn);
    }
    if (r1 == r0) return SKL_OK;
    // band heights, every pair once or row by row, overlap: knn_plan.hpp plan_knn_rows
    KnnRowsCall rc;
    rc.n_cand = n_cand;
    rc.r0 = r0;
    rc.r1 = r1;
    rc.knn = knn;
    rc.self_mode = self_mode != 0;
    rc.coreacc = coreacc;
    rc.ref_ties = ctx->knn_ties == SKL_KNN_TIES_REFERENCE;
    rc.nk = rows->nk;
    rc.ss64 = rows->ss64;
    rc.both_comp = rows->d_comp && cands->d_comp;
    rc.fused_coreacc_ok = fused_coreacc_ok(rows);
    rc.forced_kernel = forced_kernel(ctx);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) rc.free_bytes = free_b;
    rc.knobs = ctx->knobs;
    const KnnRowsPlan plan = plan_knn_rows(rc);

    // device staging for host-destined results
    uint64_t *d_idx = out_idx;
    float *d_d0 = out_d0, *d_d1 = out_d1;
    const size_t items = (r1 - r0) * knn;
    if (!out_on_device) {
        void *stage = nullptr;
        SKL_TRY(ctx_scratch(ctx, items * (sizeof(uint64_t) + 2 * sizeof(float)), &stage, SCRATCH_KNN_STAGING));
        d_idx = (uint64_t *)stage;
        d_d0 = (float *)(d_idx + items);
        d_d1 = d_d0 + items;
    }
    SKL_TRY(prune_stats_reset(ctx));
    if (plan.symmetric) {
        SKL_TRY(knn_self_symmetric(ctx, rows, p, knn, plan.band_rows, plan.overlap, d_idx, d_d0, d_d1));
    } else {
        SKL_TRY(knn_rows_banded(ctx, rows, cands, p, rc, plan.band_rows, plan.overlap, d_idx, d_d0, d_d1));
    }
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(out_idx, d_idx, items * sizeof(uint64_t), hipMemcpyDeviceToHost,
                               ctx->stream));
        HIP_TRY(hipMemcpyAsync(out_d0, d_d0, items * sizeof(float), hipMemcpyDeviceToHost,
                               ctx->stream));
        if (coreacc) {
            HIP_TRY(hipMemcpyAsync(out_d1, d_d1, items * sizeof(float), hipMemcpyDeviceToHost,
                                   ctx->stream));
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return SKL_OK;
}

extern "C" int skl_ctx_knn_prune_stats(skl_ctx *ctx, uint64_t *tiles, uint64_t *tiles_pruned, uint64_t *stages_per_tile,
                                       uint64_t *stages_walked_in_pruned_tiles, uint64_t *tiles_sparse)
{
    SKL_TRY(ctx_bind(ctx));
    SKL_TRY(prune_stats_collect(ctx));
    if (tiles_sparse) *tiles_sparse = ctx->knn_tiles_sparse;
    if (tiles) *tiles = ctx->knn_tiles;
    if (tiles_pruned) *tiles_pruned = ctx->knn_tiles_pruned;
    if (stages_per_tile) *stages_per_tile = ctx->knn_tile_stages;
    if (stages_walked_in_pruned_tiles) *stages_walked_in_pruned_tiles = ctx->knn_pruned_stages;
    return SKL_OK;
}

extern "C" int skl_ctx_set_knn_ties(skl_ctx *ctx, int mode)
{
    SKL_TRY(ctx_bind(ctx));
    if (mode != SKL_KNN_TIES_CANONICAL && mode != SKL_KNN_TIES_REFERENCE) return fail(SKL_ERR_INVALID_ARG, "unknown kNN tie mode %d", mode);
    ctx->knn_ties = mode;
    return SKL_OK;
}

extern "C" int skl_self_dists_knn_rows(skl_ctx *ctx, const skl_sketches *s,
                                       const skl_dist_params *p, size_t knn, size_t row_begin,
                                       size_t row_end, uint64_t *out_idx, float *out_d0,
                                       float *out_d1, int out_on_device)
{
    SKL_TRY(check_params(s, s, p));
    return knn_rows(ctx, s, s, p, knn, 1, row_begin, row_end, out_idx, out_d0, out_d1,
                    out_on_device);
}

extern "C" int skl_self_dists_knn(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p,
                                  size_t knn, uint64_t *out_idx, float *out_d0, float *out_d1,
                                  int out_on_device)
{
    if (!s) return fail(SKL_ERR_INVALID_ARG, "null sketches");
    return skl_self_dists_knn_rows(ctx, s, p, knn, 0, s->n, out_idx, out_d0, out_d1, out_on_device);
}

extern "C" size_t skl_knn_band_rows(const skl_sketches *s, const skl_dist_params *p, size_t n_participants)
{
    if (!s || !p || s->n == 0) return 0;
    const size_t rec = coreacc_rec_with_counts(p->dist_type == SKL_DIST_COREACC, s->nk, fused_coreacc_ok(s));
    return knn_shared_band_rows(s->n, rec, s->ctx->knobs, n_participants);
}

extern "C" int skl_self_dists_knn_partial(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t knn,
                                          size_t band_rows, const uint32_t *bands, size_t n_bands,
                                          uint32_t *state_key, uint32_t *state_idx, float *state_d1,
                                          int out_on_device)
{
    SKL_TRY(check_params(s, s, p));
    SKL_TRY(ctx_bind(ctx));
    const bool coreacc = p->dist_type == SKL_DIST_COREACC;
    if (!state_key || !state_idx || (coreacc && !state_d1)) return fail(SKL_ERR_INVALID_ARG, "state pointers are null");
    const size_t n = s->n;
    if (n < 2 || knn == 0 || knn > n - 1) return fail(SKL_ERR_INVALID_ARG, "knn=%zu must be in [1, %zu]", knn, n ? n - 1 : 0);
    if (knn > (size_t)TOPK_LDS_MAX) return fail(SKL_ERR_INVALID_ARG, "the one-evaluation kNN keeps its running lists in LDS: knn=%zu exceeds %u; shard rows with skl_self_dists_knn_rows", knn, TOPK_LDS_MAX);
    if (ctx->knn_ties == SKL_KNN_TIES_REFERENCE) {
        return fail(SKL_ERR_INVALID_ARG, "the reference's tie order follows from the order candidates arrive in: no one-evaluation form; "
                                         "shard rows with skl_self_dists_knn_rows");
    }
    if (band_rows == 0) return fail(SKL_ERR_INVALID_ARG, "band_rows is zero");
    if (n_bands && !bands) return fail(SKL_ERR_INVALID_ARG, "bands is null");
    if (!knn_symmetric_ok(s, p)) {
        return fail(SKL_ERR_INVALID_ARG, "no one-evaluation kNN for this configuration; shard rows with skl_self_dists_knn_rows");
    }
    const size_t total_bands = (n + band_rows - 1) / band_rows;
    std::vector<uint32_t> list(bands, bands + n_bands);
    for (size_t x = 0; x < list.size(); ++x) {
        if (list[x] >= total_bands || (x && list[x] <= list[x - 1])) {
            return fail(SKL_ERR_INVALID_ARG, "bands must be ascending and below %zu", total_bands);
        }
    }
    KnnState st;
    SKL_TRY(knn_state_init(st, n, knn, coreacc, ctx->stream));
    SKL_TRY(prune_stats_reset(ctx));
    const bool overlap = ctx->knobs.knn_overlap && list.size() > 1;
    SKL_TRY(knn_run_bands(ctx, s, s, p, knn_call(ctx, s, s, p, KNN_SYMMETRIC, knn, band_rows, list.size(), overlap, st), list, st));
    const hipMemcpyKind kind = out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const size_t items = n * knn;
    HIP_TRY(hipMemcpyAsync(state_key, st.key, items * sizeof(uint32_t), kind, ctx->stream));
    HIP_TRY(hipMemcpyAsync(state_idx, st.idx, items * sizeof(uint32_t), kind, ctx->stream));
    if (coreacc) HIP_TRY(hipMemcpyAsync(state_d1, st.d1, items * sizeof(float), kind, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // the running states are freed on return
    return SKL_OK;
}

// ---------------------------------------------------------------------------
// The reference's tie order over several devices, every pair evaluated once: the column-window pipeline.
// ---------------------------------------------------------------------------
// A row's BinaryHeap must meet its candidates in ascending id (mod.rs:156-181), so partial heaps cannot be merged; but a heap
// can TRAVEL.  Participant r owns the column window [lo_r, hi_r) (windows ascending with r, cut where the pair counts
// balance) and evaluates exactly the pairs (i, j) with i < j and j in its window: for each row band [b0, b1) with b0 < hi_r,
// ascending, the band's rows against the columns [max(b0, lo_r), hi_r) -- the band's own rows take them as candidates, and the
// window's rows below the band take the band's samples turned.  A row of the window therefore meets, on its owner, every id
// below its own (turned from the bands above it, ascending) and then its window's ids above; its heap then moves to
// participant r + 1 -- which feeds it the columns of ITS window when it reaches that row's band -- and so on to the last one,
// where every heap ends.  The heaps of rows [b0, b1) are handed on as soon as the band is done, so the participants work one
// band behind each other.  This call is one band on one participant; the caller owns the heap arrays (device memory, the
// RefHeap layout of skl_knn_heaps_*: h_key / h_id / h_d1 [n][knn], h_len [n], thr [n]) and moves row slices between devices.
static int knn_window_impl(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t knn,
                           size_t band_rows, size_t band, size_t col_lo, size_t col_hi,
                           float *h_key, uint32_t *h_id, float *h_d1, uint32_t *h_len, uint32_t *thr,
                           float *log_rec, uint32_t *log_id, uint32_t *log_len, size_t log_cap)
{
    SKL_TRY(check_params(s, s, p));
    SKL_TRY(ctx_bind(ctx));
    const bool coreacc = p->dist_type == SKL_DIST_COREACC;
    if (!h_key || !h_id || !h_len || !thr || (coreacc && !h_d1)) return fail(SKL_ERR_INVALID_ARG, "heap state pointers are null");
    const size_t n = s->n;
    if (n < 2 || knn == 0 || knn > n - 1) return fail(SKL_ERR_INVALID_ARG, "knn=%zu must be in [1, %zu]", knn, n ? n - 1 : 0);
    if (knn > (size_t)REFHEAP_LDS_MAX) return fail(SKL_ERR_INVALID_ARG, "the travelling heaps live in LDS while they are fed: knn=%zu exceeds %u", knn, REFHEAP_LDS_MAX);
    if (band_rows == 0 || band * band_rows >= n || col_lo > col_hi || col_hi > n) return fail(SKL_ERR_INVALID_ARG, "row band / column window out of range");
    // (an empty window holds no pair: nothing to evaluate and nothing to refuse -- a caller that cuts its own windows may hand one
    // to a participant past the last band boundary below n -- so no launch, heaps and logs untouched)
    if (col_lo == col_hi) return SKL_OK;
    // (a window that starts inside a band would give that band's rows turned candidates on this window's owner which the heaps
    // arriving from the upstream participant then overwrite: candidates silently lost)
    if (col_lo % band_rows != 0 || (col_hi % band_rows != 0 && col_hi != n)) {
        return fail(SKL_ERR_INVALID_ARG, "column window [%zu, %zu) must be cut on band boundaries (multiples of band_rows = %zu; col_hi may equal n)", col_lo, col_hi, band_rows);
    }
    if (!knn_symmetric_ok(s, p)) return fail(SKL_ERR_INVALID_ARG, "no one-evaluation kNN for this configuration; shard rows with skl_self_dists_knn_rows");
    KnnState st;
    st.borrowed = true;
    st.h_key = h_key;
    st.h_id = h_id;
    st.h_d1 = h_d1;
    st.h_len = h_len;
    st.thr = thr;
    st.log_rec = log_rec;
    st.log_id = log_id;
    st.log_len = log_len;
    st.log_cap = (uint32_t)log_cap;
    const std::vector<uint32_t> one{(uint32_t)band};
    // (the counters run on over the bands of a window: skl_ctx_knn_prune_stats reports everything since the last kNN
    // call of another kind -- no read-back, no reset here: this call must not stall the hand-over of the heaps)
    KnnCall call = knn_call(ctx, s, s, p, KNN_WINDOW, knn, band_rows, one.size(), false, st);
    call.win_lo = col_lo;
    call.win_hi = col_hi;
    // Every list the band's TURNED copy reaches -- the window's rows [max(b1, col_lo), col_hi) -- holds knn candidates: bands
    // 0 .. band - 1 of this call's sequence gave each of them band_rows >= knn, on this participant, so this holds for heaps that
    // started empty on the window (the _logged form) as well.  It says nothing of the band's OWN rows: below col_lo they start
    // empty under logs.  It need not: it only feeds plain_marks_nothing, which epilogue.hip applies to the turned side, while
    // the own rows' records are stored and marked by the row-side test against the row's own threshold (thr_row: "not full"
    // lets a (1, 1) in), so a row with fewer than knn candidates still takes its plain pairs.
    call.lists_hold_knn = band >= 1 && band_rows >= knn;
    return knn_run_bands(ctx, s, s, p, call, one, st);
}

// Empty heaps (h_len = 0, thr = "not full") for rows [row_begin, row_end) of caller-owned state arrays.
extern "C" int skl_self_dists_knn_window(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t knn,
                                         size_t band_rows, size_t band, size_t col_lo, size_t col_hi,
                                         float *h_key, uint32_t *h_id, float *h_d1, uint32_t *h_len, uint32_t *thr)
{
    return knn_window_impl(ctx, s, p, knn, band_rows, band, col_lo, col_hi, h_key, h_id, h_d1, h_len, thr, nullptr, nullptr, nullptr, 0);
}

// DECOUPLED COLUMN WINDOWS (round 6).  The travelling heaps make participant r wait for r - 1.  A heap that starts EMPTY on a
// window takes a superset of what the row's true heap -- the one that has already met every earlier window -- would take
// there (its maximum is never lower, and push_heap's test is `key < maximum`, mod.rs:41-48), so every participant can run its
// window against empty heaps at once and LOG what they take, in order; the row's true list is then the replay of the logs in
// window order (skl_knn_heaps_replay): a candidate missing from a log was refused by a heap with a higher maximum, so the true
// heap refuses it too, and the logged ones reach it in the order the reference would have shown them.
extern "C" int skl_self_dists_knn_window_logged(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t knn,
                                                size_t band_rows, size_t band, size_t col_lo, size_t col_hi,
                                                float *h_key, uint32_t *h_id, float *h_d1, uint32_t *h_len, uint32_t *thr,
                                                float *log_rec, uint32_t *log_id, uint32_t *log_len, size_t log_cap)
{
    if (!log_rec || !log_id || !log_len || log_cap == 0 || log_cap >= (1ull << 31)) return fail(SKL_ERR_INVALID_ARG, "accept-log pointers / capacity");
    return knn_window_impl(ctx, s, p, knn, band_rows, band, col_lo, col_hi, h_key, h_id, h_d1, h_len, thr, log_rec, log_id, log_len, log_cap);
}

extern "C" int skl_knn_heaps_replay(skl_ctx *ctx, size_t rows, size_t knn, int coreacc, const float *log_rec, const uint32_t *log_id,
                                    const uint32_t *log_len, size_t log_cap, float *h_key, uint32_t *h_id, float *h_d1, uint32_t *h_len,
                                    uint32_t *thr)
{
    SKL_TRY(ctx_bind(ctx));
    if (rows == 0) return SKL_OK;
    if (!log_rec || !log_id || !log_len || !h_key || !h_id || !h_len || !thr || (coreacc && !h_d1)) return fail(SKL_ERR_INVALID_ARG, "null argument");
    if (knn == 0 || knn > (size_t)REFHEAP_LDS_MAX || log_cap == 0 || log_cap >= (1ull << 31) || rows >= (1ull << 31)) return fail(SKL_ERR_INVALID_ARG, "knn / capacity / rows out of range");
    RefHeapMergeArgs m;
    memset(&m, 0, sizeof m);
    m.keys = log_rec;
    m.stride2 = coreacc ? 2u : 1u;
    m.key_stride = (uint64_t)log_cap * m.stride2;
    m.rows = (uint32_t)rows;
    m.cols = (uint32_t)log_cap;
    m.self_id_base = 0xFFFFFFFFu;   // (a log never holds the row itself)
    m.knn = (uint32_t)knn;
    m.h_key = h_key;
    m.h_id = h_id;
    m.h_d1 = h_d1;
    m.h_len = h_len;
    m.thr = thr;
    m.cand_ids = log_id;
    m.row_cols = log_len;
    m.force_workgroup_form = ctx->knobs.refheap_wave ? 0u : 1u;
    HIP_TRY(launch_refheap_merge(m, ctx->stream));
    return SKL_OK;
}

extern "C" int skl_knn_heaps_clear(skl_ctx *ctx, size_t row_begin, size_t row_end, uint32_t *h_len, uint32_t *thr)
{
    SKL_TRY(ctx_bind(ctx));
    if (!h_len || !thr || row_begin > row_end) return fail(SKL_ERR_INVALID_ARG, "bad heap range");
    if (row_begin == row_end) return SKL_OK;
    HIP_TRY(hipMemsetAsync(h_len + row_begin, 0, (row_end - row_begin) * sizeof(uint32_t), ctx->stream));
    HIP_TRY(hipMemsetAsync(thr + row_begin, 0xFF, (row_end - row_begin) * sizeof(uint32_t), ctx->stream));
    return SKL_OK;
}

extern "C" int skl_device_malloc(skl_ctx *ctx, size_t bytes, void **out)
{
    SKL_TRY(ctx_bind(ctx));
    if (!out) return fail(SKL_ERR_INVALID_ARG, "out is null");
    *out = nullptr;
    HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
    return SKL_OK;
}

extern "C" int skl_device_free(skl_ctx *ctx, void *ptr)
{
    SKL_TRY(ctx_bind(ctx));
    if (!ptr) return SKL_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipFree(ptr));
    return SKL_OK;
}

extern "C" int skl_device_memcpy(skl_ctx *ctx, void *dst, const void *src, size_t bytes, int to_device)
{
    SKL_TRY(ctx_bind(ctx));
    if (bytes == 0) return SKL_OK;
    if (!dst || !src) return fail(SKL_ERR_INVALID_ARG, "null pointer");
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SKL_OK;
}

extern "C" int skl_ctx_get_knn_ties(const skl_ctx *ctx) { return ctx ? ctx->knn_ties : SKL_KNN_TIES_REFERENCE; }

// into_sorted_vec of `rows` heaps (arrays pointing at the first of them) -> the public output form (device pointers).
extern "C" int skl_knn_heaps_finalize(skl_ctx *ctx, size_t rows, size_t knn, const float *h_key, const uint32_t *h_id, const float *h_d1,
                                      const uint32_t *h_len, int ani, uint64_t *out_idx, float *out_d0, float *out_d1)
{
    SKL_TRY(ctx_bind(ctx));
    if (!h_key || !h_id || !h_len || !out_idx || !out_d0 || (h_d1 && !out_d1)) return fail(SKL_ERR_INVALID_ARG, "null argument");
    if (knn == 0 || knn > (size_t)REFHEAP_LDS_MAX) return fail(SKL_ERR_INVALID_ARG, "knn out of range");
    HIP_TRY(launch_refheap_finalize(h_key, h_id, h_d1, h_len, (uint32_t)rows, (uint32_t)knn, (!h_d1 && ani) ? 1 : 0, out_idx, out_d0, out_d1, ctx->stream));
    return SKL_OK;
}

extern "C" int skl_knn_merge_states(skl_ctx *ctx, size_t n_states, size_t rows, size_t knn,
                                    const uint32_t *state_key, const uint32_t *state_idx, const float *state_d1,
                                    int states_on_device, int ani, uint64_t *out_idx, float *out_d0, float *out_d1,
                                    int out_on_device)
{
    SKL_TRY(ctx_bind(ctx));
    if (!state_key || !state_idx || !out_idx || !out_d0) return fail(SKL_ERR_INVALID_ARG, "null argument");
    if (state_d1 && !out_d1) return fail(SKL_ERR_INVALID_ARG, "out_d1 is required with second values");
    if (n_states == 0 || knn == 0 || knn > 2048) return fail(SKL_ERR_INVALID_ARG, "n_states and knn (<= 2048) must be positive");
    if (rows == 0) return SKL_OK;
    const size_t items = rows * knn;
    DevBuf in_key, in_idx, in_d1, tmp_key[2], tmp_idx[2], tmp_d1[2], o_idx, o_d0, o_d1;
    const uint32_t *d_key = state_key, *d_idx = state_idx;
    const float *d_d1 = state_d1;
    if (!states_on_device) {
        HIP_TRY(hipMalloc(&in_key.p, n_states * items * sizeof(uint32_t)));
        HIP_TRY(hipMalloc(&in_idx.p, n_states * items * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(in_key.p, state_key, n_states * items * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(in_idx.p, state_idx, n_states * items * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        d_key = (const uint32_t *)in_key.p;
        d_idx = (const uint32_t *)in_idx.p;
        if (state_d1) {
            HIP_TRY(hipMalloc(&in_d1.p, n_states * items * sizeof(float)));
            HIP_TRY(hipMemcpyAsync(in_d1.p, state_d1, n_states * items * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            d_d1 = (const float *)in_d1.p;
        }
    }
    // fold the states, as many per launch as fit the LDS sort
    std::vector<const uint32_t *> keys, idxs;
    std::vector<const float *> d1s;
    for (size_t x = 0; x < n_states; ++x) {
        keys.push_back(d_key + x * items);
        idxs.push_back(d_idx + x * items);
        d1s.push_back(d_d1 ? d_d1 + x * items : nullptr);
    }
    const size_t group = std::max<size_t>(2, std::min<size_t>(MERGE_STATES_MAX, MERGE_STATES_ITEMS / knn));
    int flip = 0;
    for (;;) {   // (one state: a pass through the kernel is a copy)
        const size_t take = std::min(group, keys.size());
        if (!tmp_key[flip].p) {
            HIP_TRY(hipMalloc(&tmp_key[flip].p, items * sizeof(uint32_t)));
            HIP_TRY(hipMalloc(&tmp_idx[flip].p, items * sizeof(uint32_t)));
            if (d_d1) HIP_TRY(hipMalloc(&tmp_d1[flip].p, items * sizeof(float)));
        }
        MergeStatesArgs m;
        memset(&m, 0, sizeof m);
        for (size_t x = 0; x < take; ++x) {
            m.key[x] = keys[x];
            m.idx[x] = idxs[x];
            m.d1[x] = d1s[x];
        }
        m.n_in = (uint32_t)take;
        m.rows = (uint32_t)rows;
        m.knn = (uint32_t)knn;
        m.out_key = (uint32_t *)tmp_key[flip].p;
        m.out_idx = (uint32_t *)tmp_idx[flip].p;
        m.out_d1 = d_d1 ? (float *)tmp_d1[flip].p : nullptr;
        HIP_TRY(launch_merge_states(m, ctx->stream));
        keys.erase(keys.begin(), keys.begin() + take);
        idxs.erase(idxs.begin(), idxs.begin() + take);
        d1s.erase(d1s.begin(), d1s.begin() + take);
        keys.insert(keys.begin(), m.out_key);
        idxs.insert(idxs.begin(), m.out_idx);
        d1s.insert(d1s.begin(), m.out_d1);
        flip ^= 1;
        if (keys.size() == 1) break;
    }
    uint64_t *r_idx = out_idx;
    float *r_d0 = out_d0, *r_d1 = out_d1;
    if (!out_on_device) {
        HIP_TRY(hipMalloc(&o_idx.p, items * sizeof(uint64_t)));
        HIP_TRY(hipMalloc(&o_d0.p, items * sizeof(float)));
        r_idx = (uint64_t *)o_idx.p;
        r_d0 = (float *)o_d0.p;
        if (d_d1) {
            HIP_TRY(hipMalloc(&o_d1.p, items * sizeof(float)));
            r_d1 = (float *)o_d1.p;
        }
    }
    HIP_TRY(launch_topk_finalize(keys[0], idxs[0], d1s[0], items, (!d_d1 && ani) ? 1 : 0, r_idx, r_d0, r_d1, ctx->stream));
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(out_idx, r_idx, items * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(out_d0, r_d0, items * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (d_d1) HIP_TRY(hipMemcpyAsync(out_d1, r_d1, items * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // temporaries are freed on return
    return SKL_OK;
}

extern "C" int skl_cross_dists_knn_rows(skl_ctx *ctx, const skl_sketches *ref,
                                        const skl_sketches *query, const skl_dist_params *p,
                                        size_t knn, size_t query_begin, size_t query_end,
                                        uint64_t *out_idx, float *out_d0, float *out_d1,
                                        int out_on_device)
{
    SKL_TRY(check_params(ref, query, p));
    if (ref->n == 0) return fail(SKL_ERR_EMPTY_DB, "Reference database has no loaded samples");
    if (query->n == 0) return fail(SKL_ERR_EMPTY_DB, "Query database has no loaded samples");
    // rows = queries (scalar operand), candidates = refs (lane operand); samebits and the
    // completeness factor are symmetric in the pair, so core_acc_dist(ref, query, ri, qi)
    // (mod.rs:377-385) is computed with the roles swapped.
    return knn_rows(ctx, query, ref, p, knn, 0, query_begin, query_end, out_idx, out_d0, out_d1,
                    out_on_device);
}

extern "C" int skl_cross_dists_knn(skl_ctx *ctx, const skl_sketches *ref,
                                   const skl_sketches *query, const skl_dist_params *p, size_t knn,
                                   uint64_t *out_idx, float *out_d0, float *out_d1,
                                   int out_on_device)
{
    if (!ref || !query) return fail(SKL_ERR_INVALID_ARG, "null sketches");
    return skl_cross_dists_knn_rows(ctx, ref, query, p, knn, 0, query->n, out_idx, out_d0, out_d1,
                                    out_on_device);
}
