// capi_cand.cpp -- the candidate-list kNN of the precluster mode: skl_self_dists_knn_candidates,
// skl_self_dists_knn_shared_bins.  Kernels: cand_gen.hip, pair_cand.hip, topk.hip.
#include "capi_internal.hpp"

#include <algorithm>
#include <cstring>

using namespace skl;

// The last step of a candidate-list call: the per-row selection of rows [r, r + rows) -- `launch(first_row, rows)` --
// and the results' way back to the host.  A copy into pageable memory blocks its caller, so large results go in four row
// batches, batch b's copy issued on the auxiliary stream behind batch b + 1's selection.
template <class Launch>
static int select_and_copy_back(skl_ctx *ctx, size_t n, size_t knn, const Launch &launch, const void *d_idx, const void *d_d0,
                                uint64_t *out_idx, float *out_d0)
{
    const size_t n_batches = n * knn * (sizeof(uint64_t) + sizeof(float)) >= (32u << 20) ? 4 : 1;
    size_t prev0 = 0, prev_rows = 0;
    auto copy_back = [&](size_t r0, size_t rows, int ev) -> int {
        HIP_TRY(hipStreamWaitEvent(ctx->aux_stream, ctx->knn_pair_done[ev], 0));
        HIP_TRY(hipMemcpyAsync(out_idx + r0 * knn, (const uint64_t *)d_idx + r0 * knn, rows * knn * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->aux_stream));
        HIP_TRY(hipMemcpyAsync(out_d0 + r0 * knn, (const float *)d_d0 + r0 * knn, rows * knn * sizeof(float), hipMemcpyDeviceToHost, ctx->aux_stream));
        return SKL_OK;
    };
    for (size_t b = 0; b < n_batches; ++b) {
        const size_t r0 = n * b / n_batches, r1 = n * (b + 1) / n_batches;
        if (r1 == r0) continue;
        SKL_TRY(launch(r0, r1 - r0));
        HIP_TRY(hipEventRecord(ctx->knn_pair_done[b & 1], ctx->stream));
        if (prev_rows) SKL_TRY(copy_back(prev0, prev_rows, (int)((b - 1) & 1)));
        prev0 = r0;
        prev_rows = r1 - r0;
    }
    if (prev_rows) SKL_TRY(copy_back(prev0, prev_rows, (int)((n_batches - 1) & 1)));
    HIP_TRY(hipStreamSynchronize(ctx->aux_stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SKL_OK;
}

// Candidate-list kNN: the device half of the reference's self_dists_knn_precluster
// (src/distances/mod.rs:399-553).  Host pointers in, host pointers out.
// Distances + ragged top-k for candidate lists that are already on the device.  host_offsets is
// the host copy of the CSR offsets (the 64-candidate work items are cut on the host).
static int knn_from_device_csr(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t knn,
                               const uint64_t *host_offsets, const uint64_t *d_off, const uint32_t *d_cand,
                               bool symmetric_lists, uint64_t *out_idx, float *out_d0)
{
    const size_t n = s->n;
    const uint64_t total = host_offsets[n];
    const bool symmetric = symmetric_lists && ctx->knobs.cand_symmetric;
    // symmetric lists: only the candidates with a larger id than the row are evaluated (the
    // kernel stores each key for both rows), so a row's work items start at its first such candidate
    std::vector<uint64_t> first;
    DevBuf d_first;
    if (symmetric && n) {
        HIP_TRY(hipMalloc(&d_first.p, n * sizeof(uint64_t)));
        HIP_TRY(launch_first_greater(d_off, d_cand, (uint32_t)n, (uint64_t *)d_first.p, ctx->stream));
        first.resize(n);
        HIP_TRY(hipMemcpyAsync(first.data(), d_first.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    // Launch order of the rows (round 4).  pair_cand_kernel is bound by the gather of the candidates' sketches, and the rows
    // of one cluster gather nearly the SAME candidates: dispatched next to each other they find them in the L2 of their XCD;
    // in sample order -- cluster members scattered over the database -- every pair goes to HBM.  Rows are therefore taken
    // in the order of their first candidate (the lowest member of the cluster, as a rule): a counting sort, no list is
    // looked at.  (SKL_CAND_ROW_ORDER=0: sample order, A/B.)
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    if (ctx->knobs.cand_row_order && n > 1) {
        DevBuf d_key;
        HIP_TRY(hipMalloc(&d_key.p, n * sizeof(uint32_t)));
        HIP_TRY(launch_first_candidate(d_off, d_cand, (uint32_t)n, (uint32_t *)d_key.p, ctx->stream));
        std::vector<uint32_t> key(n);
        HIP_TRY(hipMemcpyAsync(key.data(), d_key.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        std::vector<uint32_t> begin(n + 2, 0);   // bucket n: empty rows
        for (size_t i = 0; i < n; ++i) ++begin[(key[i] < n ? key[i] : n) + 1];
        for (size_t b = 0; b <= n; ++b) begin[b + 1] += begin[b];
        for (size_t i = 0; i < n; ++i) order[begin[key[i] < n ? key[i] : n]++] = (uint32_t)i;
    }
    // The work items (a row and up to 64 of its candidates each; millions at a few hundred thousand rows): the host only
    // counts them per row, in launch order; a kernel writes them out.
    std::vector<uint64_t> item_begin(n + 1, 0);
    for (size_t x = 0; x < n; ++x) {
        const size_t i = order[x];
        item_begin[x + 1] = item_begin[x] + (host_offsets[i + 1] - (symmetric ? first[i] : host_offsets[i]) + 63) / 64;
    }
    const uint64_t n_items = item_begin[n];
    DevBuf d_wrow, d_wstart, d_order, d_ibegin, d_keys, d_idx, d_d0;
    HIP_TRY(hipMalloc(&d_wrow.p, std::max<size_t>(n_items * sizeof(uint32_t), 16)));
    HIP_TRY(hipMalloc(&d_wstart.p, std::max<size_t>(n_items * sizeof(uint64_t), 16)));
    HIP_TRY(hipMalloc(&d_order.p, std::max<size_t>(n * sizeof(uint32_t), 16)));
    HIP_TRY(hipMalloc(&d_ibegin.p, (n + 1) * sizeof(uint64_t)));
    if (n) HIP_TRY(hipMemcpyAsync(d_order.p, order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_ibegin.p, item_begin.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_cand_work_items((const uint32_t *)d_order.p, (const uint64_t *)d_ibegin.p, d_off, (const uint64_t *)d_first.p,
                                   (uint32_t)n, (uint32_t *)d_wrow.p, (uint64_t *)d_wstart.p, ctx->stream));
    HIP_TRY(hipMalloc(&d_keys.p, std::max<size_t>(total * sizeof(float), 16)));
    HIP_TRY(hipMalloc(&d_idx.p, n * knn * sizeof(uint64_t)));
    HIP_TRY(hipMalloc(&d_d0.p, n * knn * sizeof(float)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // pageable uploads done before the vectors die

    PairArgs g;
    SKL_TRY(fill_args(s, s, p, MODE_JACCARD, p->ani ? JOUT_ANI_KEY : JOUT_DIST, &g));
    g.xcd_shift = ctx->knobs.cand_row_order ? ctx_xcd_shift(ctx) : 0u;
    CandArgs c;
    memset(&c, 0, sizeof c);
    c.row_offsets = d_off;
    c.cand = d_cand;
    c.work_row = (const uint32_t *)d_wrow.p;
    c.work_start = (const uint64_t *)d_wstart.p;
    c.n_work = n_items;
    c.keys = (float *)d_keys.p;
    c.symmetric = symmetric ? 1u : 0u;
    c.lanes_over_candidates = ctx->knobs.cand_lanes ? 1u : 0u;
    {   // bracketed like the pair kernels, so skl_ctx_kernel_ms() reports it
        std::pair<hipEvent_t, hipEvent_t> *ev = timing_slot(ctx);
        if (ev) HIP_TRY(hipEventRecord(ev->first, ctx->stream));
        HIP_TRY(launch_pair_cand(c, g, ctx->stream));
        if (ev) HIP_TRY(hipEventRecord(ev->second, ctx->stream));
    }
    ctx->last_kernel = "skl::pair_cand_rows_kernel (row x 64 candidates per wave, one after the other, each read as one contiguous run)";
#ifdef SKL_AB
    if (ctx->knobs.cand_lanes) ctx->last_kernel = "skl::pair_cand_kernel (row x 64 candidates per wave, candidate gather from the reference layout)";
#endif
    if (ctx->knn_ties == SKL_KNN_TIES_REFERENCE) {
        // The reference's tie order: its BinaryHeap replayed over each row's candidates IN THE ORDER THEY ARE LISTED
        // (mod.rs:459-487 pushes in the order Inverted::any_shared_bins returns them: ascending .ski index -- the
        // caller lists them that way; lists built on the device are ascending in the slab's sample order).
        RefHeapArgs h;
        memset(&h, 0, sizeof h);
        h.keys = (const float *)d_keys.p;
        h.stride2 = 1;
        h.rows = (uint32_t)n;
        h.self_id_base = 0xFFFFFFFFu;
        h.knn = (uint32_t)knn;
        h.ani_undo = p->ani ? 1 : 0;
        h.out_idx = (uint64_t *)d_idx.p;
        h.out_d0 = (float *)d_d0.p;
        h.row_offsets = d_off;
        h.col_ids = d_cand;
        h.force_workgroup_form = ctx->knobs.refheap_wave ? 0u : 1u;
        if (knn <= (size_t)REFHEAP_LDS_MAX) {
            return select_and_copy_back(
                ctx, n, knn,
                [&](size_t r0, size_t rows) -> int {
                    h.first_row = (uint32_t)r0;
                    h.rows = (uint32_t)rows;
                    HIP_TRY(launch_topk_refheap(h, ctx->stream));
                    return SKL_OK;
                },
                d_idx.p, d_d0.p, out_idx, out_d0);
        } else {   // heaps in global memory, rows in batches of at most 1 GiB of it
            DevBuf heaps;
            const size_t per_row = 3 * (knn + 1) * sizeof(float);
            const size_t batch = std::max<size_t>(1, std::min<size_t>(n, (1ull << 30) / per_row));
            HIP_TRY(hipMalloc(&heaps.p, batch * per_row));
            h.heap_scratch = (float *)heaps.p;
            for (size_t r = 0; r < n; r += batch) {
                h.first_row = (uint32_t)r;
                h.rows = (uint32_t)std::min(batch, n - r);
                HIP_TRY(launch_topk_refheap(h, ctx->stream));
            }
            HIP_TRY(hipStreamSynchronize(ctx->stream));   // `heaps` is freed on scope exit
        }
        HIP_TRY(hipMemcpyAsync(out_idx, d_idx.p, n * knn * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(out_d0, d_d0.p, n * knn * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return SKL_OK;
    }
    TopkArgs t;
    memset(&t, 0, sizeof t);
    t.keys = (const float *)d_keys.p;
    t.rows = (uint32_t)n;
    t.cols = 0;
    t.stride2 = 1;
    t.knn = (uint32_t)knn;
    t.self_mode = 0;
    t.row_begin = 0;
    t.ani_undo = p->ani ? 1 : 0;
    t.out_idx = (uint64_t *)d_idx.p;
    t.out_d0 = (float *)d_d0.p;
    t.out_d1 = nullptr;
    t.row_offsets = d_off;
    t.col_ids = d_cand;
    if (knn <= (size_t)TOPK_LDS_MAX) {
        return select_and_copy_back(
            ctx, n, knn,
            [&](size_t r0, size_t rows) -> int {
                t.first_row = (uint32_t)r0;
                t.rows = (uint32_t)rows;
                HIP_TRY(launch_topk(t, ctx->stream));
                return SKL_OK;
            },
            d_idx.p, d_d0.p, out_idx, out_d0);
    } else {
        // more neighbours than the LDS array holds: the selected items of a row are collected and sorted in
        // global memory, rows in batches of at most 1 GiB of it
        DevBuf items;
        t.items_pitch = topk_items_pitch(knn);
        const size_t batch = std::max<size_t>(1, std::min<size_t>(n, (1ull << 30) / (t.items_pitch * sizeof(uint64_t))));
        HIP_TRY(hipMalloc(&items.p, batch * t.items_pitch * sizeof(uint64_t)));
        t.items_scratch = (uint64_t *)items.p;
        for (size_t r = 0; r < n; r += batch) {
            t.first_row = (uint32_t)r;
            t.rows = (uint32_t)std::min(batch, n - r);
            HIP_TRY(launch_topk(t, ctx->stream));
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));   // `items` is freed on scope exit
    }
    HIP_TRY(hipMemcpyAsync(out_idx, d_idx.p, n * knn * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out_d0, d_d0.p, n * knn * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return SKL_OK;
}

static int check_candidate_call(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t knn)
{
    SKL_TRY(check_params(s, s, p));
    SKL_TRY(ctx_bind(ctx));
    if (p->dist_type != SKL_DIST_JACCARD) {
        return fail(SKL_ERR_INVALID_ARG, "Prefilter only available for single k-mer distances");  // mod.rs:549-551
    }
    if (knn == 0) return fail(SKL_ERR_INVALID_ARG, "knn must be positive");
    return SKL_OK;
}

extern "C" int skl_self_dists_knn_candidates(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p,
                                             size_t knn, const uint64_t *row_offsets, const uint32_t *cand,
                                             uint64_t *out_idx, float *out_d0)
{
    const RoctxRange range_("skl:candidate-list kNN (precluster)");
    SKL_TRY(check_candidate_call(ctx, s, p, knn));
    if (!row_offsets || !out_idx || !out_d0) return fail(SKL_ERR_INVALID_ARG, "null argument");
    const size_t n = s->n;
    if (n == 0) return SKL_OK;
    const uint64_t total = row_offsets[n];
    if (total && !cand) return fail(SKL_ERR_INVALID_ARG, "cand is null");
    for (size_t i = 0; i < n; ++i) {
        if (row_offsets[i + 1] < row_offsets[i]) return fail(SKL_ERR_INVALID_ARG, "row_offsets must not decrease");
    }
    for (uint64_t x = 0; x < total; ++x) {
        if (cand[x] >= n) return fail(SKL_ERR_INVALID_ARG, "candidate id %u out of range", cand[x]);
    }
    DevBuf d_off, d_cand;
    HIP_TRY(hipMalloc(&d_off.p, (n + 1) * sizeof(uint64_t)));
    HIP_TRY(hipMalloc(&d_cand.p, std::max<size_t>(total * sizeof(uint32_t), 16)));
    HIP_TRY(hipMemcpyAsync(d_off.p, row_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    if (total) HIP_TRY(hipMemcpyAsync(d_cand.p, cand, total * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    // caller-supplied lists: no symmetry assumed, every listed pair is evaluated
    return knn_from_device_csr(ctx, s, p, knn, row_offsets, (const uint64_t *)d_off.p, (const uint32_t *)d_cand.p,
                               false, out_idx, out_d0);
}

extern "C" size_t skl_shared_bins_max_samples(void) { return MAX_DEVICE_CANDGEN_SAMPLES; }

// The whole precluster kNN on the device: candidate lists from the index sketches (cand_gen.hip),
// then distances and ragged top-k.
extern "C" int skl_self_dists_knn_shared_bins(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p,
                                              size_t knn, const uint16_t *skq, size_t sketch_size,
                                              uint64_t *out_idx, float *out_d0, uint64_t *out_n_candidates)
{
    const RoctxRange range_("skl:shared-bins candidates + kNN (precluster)");
    SKL_TRY(check_candidate_call(ctx, s, p, knn));
    if (!skq || !out_idx || !out_d0) return fail(SKL_ERR_INVALID_ARG, "null argument");
    const size_t n = s->n;
    if (out_n_candidates) *out_n_candidates = 0;
    if (n == 0) return SKL_OK;
    if (sketch_size == 0) return fail(SKL_ERR_INVALID_ARG, "sketch_size is zero");
    if (n > MAX_DEVICE_CANDGEN_SAMPLES) {
        return fail(SKL_ERR_INVALID_ARG, "%zu samples exceed the %zu the on-device candidate search handles per call",
                    n, (size_t)MAX_DEVICE_CANDGEN_SAMPLES);
    }
    DevBuf d_skq, d_starts, d_cursor, d_members, d_counts, d_off, d_cand;
    const size_t table = sketch_size * 65536 * sizeof(uint32_t);
    HIP_TRY(hipMalloc(&d_skq.p, n * sketch_size * sizeof(uint16_t)));
    HIP_TRY(hipMalloc(&d_starts.p, table));
    HIP_TRY(hipMalloc(&d_cursor.p, table));
    HIP_TRY(hipMalloc(&d_members.p, n * sketch_size * sizeof(uint32_t) + 16));   // (+16: cand_rows_kernel reads whole 16-byte blocks)
    HIP_TRY(hipMalloc(&d_counts.p, n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&d_off.p, (n + 1) * sizeof(uint64_t)));
    HIP_TRY(hipMemcpyAsync(d_skq.p, skq, n * sketch_size * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_starts.p, 0, table, ctx->stream));
    CandGenArgs cg;
    memset(&cg, 0, sizeof cg);
    cg.skq = (const uint16_t *)d_skq.p;
    cg.n = (uint32_t)n;
    cg.sketch_size = (uint32_t)sketch_size;
    cg.starts = (uint32_t *)d_starts.p;
    cg.cursor = (uint32_t *)d_cursor.p;
    cg.members = (uint32_t *)d_members.p;
    cg.counts = (uint32_t *)d_counts.p;
    HIP_TRY(launch_cand_groups(cg, ctx->stream));
    HIP_TRY(launch_cand_rows(cg, false, ctx->stream));
    std::vector<uint32_t> counts(n);
    HIP_TRY(hipMemcpyAsync(counts.data(), d_counts.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> offsets(n + 1, 0);
    for (size_t i = 0; i < n; ++i) offsets[i + 1] = offsets[i] + counts[i];
    const uint64_t total = offsets[n];
    if (out_n_candidates) *out_n_candidates = total;
    HIP_TRY(hipMalloc(&d_cand.p, std::max<size_t>(total * sizeof(uint32_t), 16)));
    HIP_TRY(hipMemcpyAsync(d_off.p, offsets.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    cg.row_offsets = (const uint64_t *)d_off.p;
    cg.cand = (uint32_t *)d_cand.p;
    HIP_TRY(launch_cand_rows(cg, true, ctx->stream));
    // the group tables are no longer needed: release them before the distance buffers are allocated
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    (void)hipFree(d_members.p); d_members.p = nullptr;
    (void)hipFree(d_starts.p); d_starts.p = nullptr;
    (void)hipFree(d_cursor.p); d_cursor.p = nullptr;
    // "any shared bin" is a symmetric relation: each candidate pair is evaluated once
    return knn_from_device_csr(ctx, s, p, knn, offsets.data(), (const uint64_t *)d_off.p, (const uint32_t *)d_cand.p,
                               true, out_idx, out_d0);
}
