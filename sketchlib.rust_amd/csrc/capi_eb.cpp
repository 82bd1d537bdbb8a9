// capi_eb.cpp -- the early break of the core/accessory calls, host side: the sample taken on the device, and the decisions the
// context keeps per slab pair.  The rules are eb_plan.hpp's (pure).
#include "capi_internal.hpp"
#include "dist_tables.hpp"
#include "glibc_log.hpp"

#include <cstring>
#include <memory>
#include <vector>

using namespace skl;

static void free_plan(EbPlan *p)
{
    if (!p) return;
    if (p->d_block_ke) (void)hipFree(p->d_block_ke);
    delete p;
}
struct EbPlanFree {
    void operator()(EbPlan *p) const { free_plan(p); }
};

void free_plans(skl_ctx *ctx)
{
    for (EbPlan *p : ctx->eb_plans) free_plan(p);
    ctx->eb_plans.clear();
    ctx->eb_last_plan = nullptr;
}

// The early break's sample: `g.samples` pairs of every block run the reference's loop on the device; *hist = [block][EB_HIST]
// pairs that pass the test at exactly their first m lengths.
static int eb_sample(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, double cutoff, const EbGeometry &g, std::vector<uint32_t> *hist)
{
    const bool has_comp = rows->d_comp != nullptr && cols->d_comp != nullptr;
    SKL_TRY(ensure_ytab(rows));
    DevBuf d_hist;
    hist->assign((size_t)g.n_blocks() * EB_HIST, 0u);
    HIP_TRY(hipMalloc(&d_hist.p, hist->size() * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(d_hist.p, 0, hist->size() * sizeof(uint32_t), ctx->stream));
    EbSampleArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.rows_ref = rows->d_rows;
    sa.cols_ref = cols->d_rows;
    sa.n_rows = (uint32_t)rows->n;
    sa.n_cols = (uint32_t)cols->n;
    sa.nk = (uint32_t)rows->nk;
    sa.ss64 = (uint32_t)rows->ss64;
    sa.self_mode = g.self_mode ? 1u : 0u;
    sa.samples = g.samples;
    sa.blk_shift_r = g.shift_r;
    sa.blk_shift_c = g.shift_c;
    sa.blk_rows = g.blk_rows;
    sa.blk_cols = g.blk_cols;
    sa.min_alive = rows->min_alive;
    sa.has_comp = has_comp ? 1 : 0;
    if (has_comp) {
        const int v = host_log_variant();
        sa.log_variant = v < 0 ? (int)SKL_LOG_FMA : v;
    }
    sa.ytab = rows->d_ytab;
    sa.compA = rows->d_comp;
    sa.compB = cols->d_comp;
    sa.cutoff = cutoff;
    sa.tolerance = break_tolerance(rows->ss64);
    sa.hist = (uint32_t *)d_hist.p;
    HIP_TRY(launch_early_break_sample(sa, ctx->stream));
    HIP_TRY(hipMemcpyAsync(hist->data(), d_hist.p, hist->size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SKL_OK;
}

// The decision for a slab pair (eb_plan.hpp): applicable? -> kept from an earlier call? -> forced, or sampled and decided -> kept.
int early_break_plan(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, int self_mode, double cutoff, const EbPlan **out)
{
    *out = nullptr;
    const int knob = ctx->knobs.early_break;
    if (!eb_applicable(knob, rows->nk, rows->n, cols->n)) return SKL_OK;
    if (!ctx->eb_counter) {
        HIP_TRY(hipMalloc((void **)&ctx->eb_counter, 1024 * sizeof(uint32_t)));   // 1 024 counter slots (diagnostic)
        HIP_TRY(hipMemsetAsync(ctx->eb_counter, 0, 1024 * sizeof(uint32_t), ctx->stream));
    }
    const bool has_comp = rows->d_comp != nullptr && cols->d_comp != nullptr;
    for (const EbPlan *p : ctx->eb_plans) {
        if (p->rows_gen == rows->gen && p->cols_gen == cols->gen && p->self_mode == self_mode && p->knob == knob && (!has_comp || p->cutoff == cutoff)) {
            *out = p;
            return SKL_OK;
        }
    }
    EbGeometry geo;
    EbDecision decision;
    if (knob >= 2) {
        decision = eb_forced(knob, rows->nk);
    } else {
        geo = eb_geometry(rows->n, cols->n, self_mode != 0);
        std::vector<uint32_t> hist;
        SKL_TRY(eb_sample(ctx, rows, cols, cutoff, geo, &hist));
        decision = eb_decide(geo, rows->nk, eb_cost((uint32_t)rows->ss64, rows->n, cols->n, self_mode != 0), hist.data());
    }
    // (owned here until it is kept: an upload that fails takes the plan and its table with it)
    std::unique_ptr<EbPlan, EbPlanFree> plan(new EbPlan());
    plan->rows_gen = rows->gen;
    plan->cols_gen = cols->gen;
    plan->self_mode = self_mode;
    plan->cutoff = cutoff;
    plan->knob = knob;
    plan->geo = geo;
    plan->decision = std::move(decision);
    if (plan->decision.mixed) {
        const std::vector<uint8_t> &ke = plan->decision.block_ke;
        HIP_TRY(hipMalloc((void **)&plan->d_block_ke, ke.size()));
        HIP_TRY(hipMemcpy(plan->d_block_ke, ke.data(), ke.size(), hipMemcpyHostToDevice));
    }
    if (ctx->eb_plans.size() >= EB_PLANS_KEPT) {
        // (nothing in flight may still read the oldest plan's table: the streams are drained before it goes)
        if (ctx->eb_plans.front()->d_block_ke != nullptr) {
            (void)hipStreamSynchronize(ctx->stream);
            if (ctx->epi_stream) (void)hipStreamSynchronize(ctx->epi_stream);
        }
        if (ctx->eb_last_plan == ctx->eb_plans.front()) ctx->eb_last_plan = nullptr;
        free_plan(ctx->eb_plans.front());
        ctx->eb_plans.erase(ctx->eb_plans.begin());
    }
    ctx->eb_plans.push_back(plan.get());
    *out = plan.release();
    return SKL_OK;
}

int early_break_lengths(skl_ctx *ctx, const skl_sketches *rows, const skl_sketches *cols, int self_mode, int *lengths)
{
    *lengths = 0;
    // (the kNN bands' epilogue has no completeness branch and no segmented counts: capi_knn.cpp)
    if (rows->d_comp != nullptr || cols->d_comp != nullptr || rows->ss64 > (size_t)KSLICE_MAX_U16_CHUNKS) return SKL_OK;
    const EbPlan *plan = nullptr;
    SKL_TRY(early_break_plan(ctx, rows, cols, self_mode, 0.0, &plan));
    if (plan) *lengths = plan->decision.lengths;
    return SKL_OK;
}

extern "C" int skl_ctx_early_break_blocks(skl_ctx *ctx, uint32_t *blk_rows, uint32_t *blk_cols, uint32_t *shift_rows, uint32_t *shift_cols,
                                          int *pooled_lengths, int *mixed, uint8_t *block_lengths, size_t capacity)
{
    SKL_TRY(ctx_bind(ctx));
    const EbPlan *p = ctx->eb_last_plan;
    if (blk_rows) *blk_rows = p ? p->geo.blk_rows : 0u;
    if (blk_cols) *blk_cols = p ? p->geo.blk_cols : 0u;
    if (shift_rows) *shift_rows = p ? p->geo.shift_r : 0u;
    if (shift_cols) *shift_cols = p ? p->geo.shift_c : 0u;
    if (pooled_lengths) *pooled_lengths = p ? p->decision.lengths : 0;
    if (mixed) *mixed = p && p->decision.mixed ? 1 : 0;
    if (p && p->decision.mixed && block_lengths) {
        const std::vector<uint8_t> &ke = p->decision.block_ke;
        if (capacity < ke.size()) return fail(SKL_ERR_INVALID_ARG, "skl_ctx_early_break_blocks: %zu blocks, room for %zu", ke.size(), capacity);
        memcpy(block_lengths, ke.data(), ke.size());
    }
    return SKL_OK;
}

