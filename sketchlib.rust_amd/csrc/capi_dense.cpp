// capi_dense.cpp -- the dense calls of include/sketchlib_dist.h: one launch of the pair kernel, the executors of a dense call's
// three forms, banding of large pair spaces through bounded scratch, and the entry points.  HOW a call is launched is decided in
// dense_plan.hpp (pure); here the decision's input is gathered and its answer executed.
#include "capi_internal.hpp"

#include <algorithm>
#include <cstring>
#include <optional>
#include <string>

using namespace skl;

static_assert(PLAN_MODE_COUNTS == MODE_COUNTS && PLAN_MODE_JACCARD == MODE_JACCARD && PLAN_MODE_COREACC == MODE_COREACC &&
              PLAN_MAX_U16_CHUNKS == (uint32_t)KSLICE_MAX_U16_CHUNKS && PLAN_SEG_CHUNKS == (uint32_t)KSLICE_SEG_CHUNKS,
              "dense_plan.hpp restates these constants of kernels.h");

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
    const PairShape s = plan_pair_shape(a);
    args.no_half_tiles = s.no_half_tiles ? 1u : 0u;
    args.round_size = s.round_size;
    if (args.tail_slices > 1u) args.tail_resident = s.tail_resident;
    const bool kslice = s.try_kslice && kslice_supported(args, mode, s.sliced_launch);
    ctx->last_kernel = pair_kernel_name(s, kslice);
    args.tile_cost_order = args_in.tile_cost_order != 0u && s.tile_cost_order && kslice ? 1u : 0u;   // (asked for by the dense calls' counts launches alone)
    if (args.tile_cost_order) ctx->last_kernel += " [tiles dealt by cost, half tiles last]";
    // the unit table: asked for by the dense calls (skl_ctx_set_unit_table 0: by nobody, 1: by every launch); the launcher gives one
    // to the forms that read it, within its cap.  Which path ran is skl_ctx_unit_table()'s answer, not part of the kernel's description.
    if (ctx->unit_table_mode >= 0) args.unit_table_ok = (uint32_t)ctx->unit_table_mode;
    ctx->last_unit_table = false;
    if (!kslice) return launch_pair_kernel_ksplit(args, mode, s.ksplit_rows, ctx->tile_scratch, stream);
    const hipError_t e = launch_pair_kernel_kslice(args, mode, s.shape, s.sliced_launch, s.ablate, ctx->tile_scratch, stream);
    ctx->last_unit_table = e == hipSuccess && ctx->tile_scratch.unit_table_used;
    return e;
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
        g.block_ke_host = plan->decision.block_ke.data();   // (the same table on the host: the unit table's builder reads it)
        g.block_ke_bytes = plan->decision.block_ke.size();
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
    g.unit_table_ok = 1;     // (a request: the launcher decides; unit_table.hpp)
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
        g.fuse_variant = ctx->knobs.fuse_variant;
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
    g.unit_table_ok = 1;
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
    g.unit_table_ok = 1;     // (k-sliced counts and single-k launches within the table's cap)
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
