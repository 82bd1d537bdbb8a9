// pair_kslice_finish.inc -- the end of a k-mer length (all-k forms), of a segment (BIG) or of the walk (k-sliced) in
// pair_kslice_walk.inc, included there inside the loop over those: the 4 waves' partial counts of every pair are summed
// through LDS, and each wave finishes its share of the pairs in the way of the kernel's mode.  Text like the walk itself:
// wrapped in a function or a lambda, the forms with segments pick up scratch and the 32-row counts form a register.
//
// (PRUNE: the lane id of the epilogue is made afresh -- two instructions -- instead of kept from the top of the kernel: with
// the probe and the sparse walk in between, the register allocator parked that one value in scratch and fetched it
// back before every use below, some thirty dependent scratch loads per tile)
if constexpr (PRUNE) asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
if (kl + 1 == n_outer) SKL_TRACE_MARK(2);
// The buffer this wave consumed last is dead (the next stage was prefetched into the
// other one), so every wave publishes into its own: [wave][buf][PX][LANES] words.
const uint32_t dead = (t - 1u) & 1u;
// word x of wave w: red_at(w, x)
uint32_t *red_rows = reinterpret_cast<uint32_t *>(&lds_all[0]);
uint32_t *red_over = reinterpret_cast<uint32_t *>(&lds_all[ROWS_U4]);
auto red_at = [&](uint32_t w, uint32_t x) -> uint32_t & {
    return x < (uint32_t)XIN ? red_rows[(w * 2u + ((KSL && !BIG) ? 0u : dead)) * (BUF_U4 * 4u) + x * LANES + lane_e]
                             : red_over[(w * (uint32_t)XOV + (x - (uint32_t)XIN)) * LANES + lane_e];
};
// wave w finishes the words (rows) r = w (mod 4); fields stay below 2^16 (ss64 <= 1023)
float tval[(MODE == MODE_JACCARD && KSL) ? SLOTS * 2 : 1];   // this wave's keys, for out_t
// (RED_PHASES = 2: words [0, XIN) first, then words [XIN, PX) through the same buffer)
#pragma unroll
for (int ph = 0; ph < RED_PHASES; ++ph) {
constexpr int XPH = PX / RED_PHASES;
if (ph > 0) __syncthreads();   // the previous phase's words have been summed
#pragma unroll
for (int x = ph * XPH; x < (ph + 1) * XPH; ++x) red_at(wave, (uint32_t)(x - ph * XPH)) = cnt[x];
if (ph == RED_PHASES - 1) {
#pragma unroll
    for (int x = 0; x < R; ++x) cnt[x] = 0;
}
__syncthreads();
#pragma unroll
for (int i = ph * (SLOTS / RED_PHASES); i < (ph + 1) * (SLOTS / RED_PHASES); ++i) {
    const uint32_t r = (uint32_t)i * W + wave;   // (word r = row r of the tile)
    uint32_t total = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) total += red_at((uint32_t)w, r - (uint32_t)(ph * XPH));
    if constexpr (MODE == MODE_COREACC) {
        // (ABL & 16, A/B build, timing only: only the last k-mer length's totals are parked -- what the kernel
        // would cost if the per-k totals needed no memory at all; outputs wrong by construction)
        if (!(ABL & 16) || kl + 1 == nkk) hist[i * MAX_FUSED_K + kl] = total;
    } else if (BIG && kl + 1 < n_outer) {   // (uniform) not the last segment: add up
        seg_acc[2 * i] = seg_acc[2 * i] + (total & 0xFFFFu);
        seg_acc[2 * i + 1] = seg_acc[2 * i + 1] + (total >> 16);
    } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t j = (uint32_t)h;   // (field h = column block h)
            uint32_t mism = h ? (total >> 16) : (total & 0xFFFFu);
            if constexpr (BIG) mism += seg_acc[2 * i + h];
            if constexpr (MODE == MODE_COUNTS) {
                if (in_tail && slice != 0u) {   // tail slices 1.. add into plane 1
                    const uint32_t i_ = a0 + r, jc_ = (jb0 + j) * 64u + lane_e;
                    if (pair_valid(g, i_, jc_)) {
                        atomicAdd(&((uint32_t *)g.out)[pair_out_index(g, i_, jc_) * g.cnt_pair_stride +
                                                       (uint64_t)(g.k_count + kk) * g.cnt_k_stride],
                                  (c_end - c_begin) * 64u - mism);
                    }
                } else if constexpr (FUSE) {   // (counts another workgroup reads back: write-through)
                    if (g.fuse_variant & 1u) store_count(g, a0 + r, (jb0 + j) * 64u + lane_e, kk, (c_end - c_begin) * 64u, mism);   // EXPERIMENT: plain stores
                    else store_count_agent(g, a0 + r, (jb0 + j) * 64u + lane_e, kk, (c_end - c_begin) * 64u, mism);
                } else {
                    store_count<KSL && !BIG>(g, a0 + r, (jb0 + j) * 64u + lane_e, (tail_mode ? 0u : slice * g.k_count) + kk, (c_end - c_begin) * 64u, mism);
                }
            } else if constexpr (KSL) {
                // (finish_key<float> as text: wrapped in ANY function -- even valid -> value -> store alone -- hipcc
                // allocates the single-k forms differently, profiles/kslice_split.md)
                const uint32_t i_ = a0 + r, jc_ = (jb0 + j) * 64u + lane_e;
                float v = __builtin_inff();
                const bool valid_ = pair_valid(g, i_, jc_);
                if (valid_) {
                    v = jaccard_out_value(g, i_, jc_, mism);
                    ((float *)g.out)[pair_out_index(g, i_, jc_)] = v;
                }
                mark_row_block(g, i_, jb0 + j, valid_, v, lane_e);
                tval[i * 2 + h] = v;
            } else {
                store_jaccard(g, a0 + r, (jb0 + j) * 64u + lane_e, mism);
            }
        }
    }
}
}
if constexpr (MODE == MODE_JACCARD && KSL) if (!BIG || kl + 1 == n_outer) {
    // Symmetric self kNN: the keys of columns >= t_col_begin are also candidates of the
    // ROW with that sample id.  The tile is turned through LDS so that a column's R keys
    // leave as R/4 16-byte stores (one 64-byte run per column at R = 16).
    if (g.out_t != nullptr && min((jb0 + (uint32_t)JL) * 64u, g.nB) > g.t_col_begin) {   // workgroup-uniform
        constexpr uint32_t TP = turned_pitch(R);
        static_assert(JL * 64 * TP * 4 <= (ROWS_U4 + RED_U4) * 16, "the turned tile fits the LDS of the workgroup");
        float *tt = reinterpret_cast<float *>(&lds_all[0]);
        __syncthreads();   // every wave is done with the reduction words
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
#pragma unroll
            for (int h = 0; h < 2; ++h) tt[((uint32_t)h * 64u + lane_e) * TP + (uint32_t)i * W + wave] = tval[i * 2 + h];
        }
        __syncthreads();
        store_turned_tile<float, R, JL>(g, tt, jb0, a0, tid);
    }
}
// the next stage's DMA of every wave goes into the buffer just read: fence the reads
if (kl + 1 < n_outer) __syncthreads();
