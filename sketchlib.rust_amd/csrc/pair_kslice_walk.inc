// pair_kslice_walk.inc -- the tile walk of pair_kernel_kslice (pair_kslice.hip), included once per
// case of column blocks [J0, J1) = SKL_WALK_BLOCKS the workgroup walks: both blocks of the tile, or one of
// them (half tiles: a block without a pair of the launch is neither loaded nor computed).  It keeps what
// depends on that case -- column prefetch, streaming loop, stage-boundary prune check, count accumulation --
// and includes the rest: pair_kslice_probe.inc, pair_kslice_finish.inc, pair_kslice_coreacc.inc.
// Everything the texts refer to -- template parameters, g, wave, lane, a0, jb0, kk0, c_begin, c_end,
// lds_all, ... -- is in scope at the point of inclusion.
{
    constexpr int WALK_BLOCKS[2] = {SKL_WALK_BLOCKS}, J0 = WALK_BLOCKS[0], J1 = WALK_BLOCKS[1];

    const size_t kmer_stride = (size_t)g.ss64 * BBITS;
    const size_t sample_stride = kmer_stride * g.nk;
    // wave w owns chunks w*CH + i + ts*(W*CH), i < CH, of every k-mer length
    // BIG (sketches beyond 65 535 bins: the u16 count fields would overflow): the one k-mer length of a k-sliced
    // workgroup is walked in SEGMENTS of g.seg_chunks chunks (a multiple of W*CH, at most 1 016: 65 024 bins).  A
    // segment is to the walk what a k-mer length is to the all-k form -- the flat stage counter runs on, the next
    // segment's first stage is prefetched under the last stage of this one, and at the end of a segment the 4 partial
    // counts per pair are summed through the row buffer just consumed -- except that the totals are ADDED UP (32-bit,
    // in private memory: touched once per segment) and the pair is finished after the last one.
    const uint32_t stages_per_k = BIG ? g.seg_chunks / (W * CH) : (c_end - c_begin + W * CH - 1) / (W * CH);
    const uint32_t n_stages = BIG ? (c_end - c_begin + W * CH - 1) / (W * CH) : stages_per_k * nkk;
    const uint32_t n_outer = BIG ? (n_stages + stages_per_k - 1) / stages_per_k : nkk;   // k-mer lengths (all-k), segments (BIG), else 1
    static_assert(!BIG || (KSL && MODE != MODE_COREACC), "segments exist for the k-sliced counts / single-k forms");
    volatile uint32_t seg_acc[BIG ? SLOTS * 2 : 1];
    if constexpr (BIG) {
#pragma unroll
        for (int x = 0; x < SLOTS * 2; ++x) seg_acc[x] = 0u;
    }

    // This wave's partial mismatch counts of the current k (its chunks only): the two columns of a row share one
    // register as u16 fields (a wave's share of one k-mer length is at most 64 * 256 mismatches per pair:
    // kslice_supported) -- R registers instead of 2 R, for one v_lshl_add_u32 more per (row, chunk).
    // Word r: row r of the tile against the lane's column of block 0 (low field) and of block 1 (high field).
    uint32_t cnt[R];
#pragma unroll
    for (int x = 0; x < R; ++x) cnt[x] = 0;
    // MODE_COREACC: totals of this wave's packed slots, one word per k-mer length (two u16
    // fields per word: the slot's two pairs).  Private (scratch) memory on purpose: written
    // once per k-mer length, read once at the end, and 24 registers cheaper.
    volatile uint32_t hist[(MODE == MODE_COREACC) ? SLOTS * MAX_FUSED_K : 1];

    // TILE PRUNING (pair_prune.hpp): the probe and the sparse walk before anything of the walk is requested, then checks at
    // stage boundaries
    uint32_t prune_next = 0xFFFFFFFFu;   // stage count (t + 1) of the next stage-boundary check of the walk
    uint32_t prune_checks = 0u;          // checks so far
    uint32_t *prune_lds = reinterpret_cast<uint32_t *>(&lds_all[ROWS_U4 + RED_U4]);
    if constexpr (PRUNE) {
        static_assert(!PRUNE || CH == 1, "the probe takes one chunk per wave and step");
#include "pair_kslice_probe.inc"
    }

    // Row staging: global -> LDS DMA (SKL_STAGE_DMA, device_common.hpp), with the per-lane byte offsets of its source kept
    uint32_t dma_lane_off[SADDR_DMA ? PPL : 1];
    if constexpr (SADDR_DMA) {
#pragma unroll
        for (int u = 0; u < PPL; ++u) {
            const uint32_t pp_ = lane + u * 64u;
            const uint32_t p_ = pp_ < (uint32_t)PIECES ? pp_ : pp_ - (uint32_t)PIECES;
            const uint32_t rc_ = p_ / 7u;
            dma_lane_off[u] = (uint32_t)(((size_t)(rc_ % R) * sample_stride + (size_t)(rc_ / R) * BBITS + 2u * (p_ % 7u)) * sizeof(uint64_t));
        }
    }
    const uint32_t lds_base = __builtin_amdgcn_readfirstlane(skl_lds_addr(&lds_all[0]));
    SKL_STAGE_DMA(0u, 0);
    SKL_TRACE_MARK(7);   // (trace build: the first row DMA is issued -- entry to here is the head's cost)

    // Next valid chunk of this wave after (kl, ts, ci) in its walk over k-mer lengths, stages
    // and chunks (wave-uniform scalar code); false when the walk is over.
    auto next_chunk = [&](uint32_t kl_, uint32_t ts_, int ci_, uint32_t &k_out, uint32_t &c_out) {
        for (;;) {
            if (++ci_ >= CH) {
                ci_ = 0;
                if (++ts_ >= stages_per_k) {
                    ts_ = 0;
                    ++kl_;
                }
            }
            if (kl_ >= n_outer) return false;
            // (BIG: segment kl_, stage ts_ of it = flat stage kl_ * stages_per_k + ts_ of the one k-mer length)
            const uint32_t c_ = c_begin + ((BIG ? kl_ * stages_per_k : 0u) + ts_) * (W * CH) + wave * CH + (uint32_t)ci_;
            if (c_ < c_end) {
                k_out = g.k_begin + kk0 + (BIG ? 0u : kl_);
                c_out = c_;
                return true;
            }
        }
    };
    auto column_ptr = [&](int j, uint32_t k_, uint32_t c_) {
        const uint32_t jb = (jb0 + j) < g.n_jblocks ? (jb0 + j) : (g.n_jblocks - 1u);   // clamped, never stored
        return g.B + (((size_t)jb * g.nk + k_) * g.ss64 + c_) * (7 * LANES) + lane;
    };

    // Column operand: 2 x 7 x 16 B per lane and chunk, always ONE CHUNK AHEAD with no extra
    // registers: during the last row of a chunk every b[j][q] is re-loaded with the next
    // chunk's data right after its last use (the first of them gets most of a row of lead,
    // the loads return in order, and the compiler's counted vmcnt before each use is exact).
    uint4 b[JL][7];
    {
        uint32_t k1 = g.k_begin + kk0, c1 = c_begin;
        next_chunk(0u, 0u, -1, k1, c1);
#pragma unroll
        for (int j = J0; j < J1; ++j) {
            const uint4 *bp = column_ptr(j, k1, c1);
#pragma unroll
            for (int q = 0; q < 7; ++q) b[j][q] = bp[q * LANES];
        }
    }
    uint32_t b_younger = 1;   // chunks' worth of column loads (JL*7 each) issued after the newest row DMA

    uint32_t t = 0;   // flat stage counter (k-mer lengths x stages)
    uint32_t lane_e = lane;   // the lane id as the epilogues use it (PRUNE: made afresh there)
    for (uint32_t kl = 0; kl < n_outer; ++kl) {
        const uint32_t kk = kk0 + (BIG ? 0u : kl);
        for (uint32_t ts = 0; ts < stages_per_k && (!BIG || t < n_stages); ++ts, ++t) {
            const uint32_t buf = t & 1u;
            const uint32_t c0 = c_begin + (BIG ? t : ts) * (W * CH) + wave * CH;
            // This wave's DMA of stage t must have landed.  VMEM returns in order, so it is
            // enough that only the younger column loads may still be in flight.
            if (b_younger == 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else if (b_younger == 1) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((J1 - J0) * 7) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (J1 - J0) * 7) : "memory");
            }
            if (t == 0) SKL_TRACE_MARK(1);
            // The next stage's rows are requested after row 0 of this stage's first chunk (all
            // column registers consumed once, so no column load is in flight then); a stage
            // in which this wave has no chunk requests them here.
            const bool want_dma = t + 1 < n_stages;
            if (want_dma && c0 >= c_end) {
                SKL_STAGE_DMA(t + 1, buf ^ 1u);
                b_younger = 0;
            }

            // (unrolled: the column loads issued in the last row of chunk 0 and their first use
            // in chunk 1 are then straight-line code, and the compiler's waits on them are counted
            // instead of the vmcnt(0) it falls back to across a loop back-edge)
#pragma unroll
            for (uint32_t ci = 0; ci < (uint32_t)CH; ++ci) {
                if (c0 + ci >= c_end) break;
                // where the columns of the next chunk are (the current ones again if none follows)
                uint32_t kn = g.k_begin + kk, cn = c0 + ci;
                next_chunk(kl, ts, (int)ci, kn, cn);
                const uint4 *bn[JL];
#pragma unroll
                for (int j = J0; j < J1; ++j) bn[j] = column_ptr(j, kn, cn);
                const uint4 *rows = &lds_rows[wave][buf][(size_t)ci * R * 7];
                // Row operand: a ring of AD plane pairs.  Step s = r * 7 + q of the chunk reads
                // rows[s]; right after its use the register is re-loaded with step s + AD (4: the 12
                // registers a whole row ahead would cost decide the occupancy).
                constexpr int AD = 4;
                uint4 a[AD];
                static_assert(R % MB == 0, "rows per tile must be a multiple of the block height");
                // step s of the chunk -> index of its plane pair in the row buffer ([row][plane pair])
                auto row_slot = [](int s) constexpr { return ((s / (7 * MB)) * MB + s % MB) * 7 + (s % (7 * MB)) / MB; };
#pragma unroll
                for (int q = 0; q < AD; ++q) a[q] = rows[row_slot(q)];
#pragma unroll
                for (int rb = 0; rb < R / MB; ++rb) {
                    uint32_t mlo[MB][JL], mhi[MB][JL];
#pragma unroll
                    for (int q = 0; q < 7; ++q) {
#pragma unroll
                        for (int m = 0; m < MB; ++m) {
                            const int s_ = (rb * 7 + q) * MB + m;      // compile-time after unrolling
                            uint4 &ar = a[s_ % AD];
#pragma unroll
                            for (int j = J0; j < J1; ++j) {
                                // b is stored (hi, lo) per plane: see device_common.hpp "VGPR banks"
                                if (q == 0) {
                                    mlo[m][j] = ar.x ^ b[j][0].y;
                                    mhi[m][j] = ar.y ^ b[j][0].x;
                                } else {
                                    mlo[m][j] = acc_mismatch_vvv(mlo[m][j], ar.x, b[j][q].y);
                                    mhi[m][j] = acc_mismatch_vvv(mhi[m][j], ar.y, b[j][q].x);
                                }
                                mlo[m][j] = acc_mismatch_vvv(mlo[m][j], ar.z, b[j][q].w);
                                mhi[m][j] = acc_mismatch_vvv(mhi[m][j], ar.w, b[j][q].z);
                            }
                            // rolling prefetch of the plane pair AD steps ahead (no extra registers)
                            __builtin_amdgcn_sched_barrier(0);
                            if (s_ + AD < R * 7) ar = rows[row_slot(s_ + AD)];
                            if (rb == R / MB - 1 && m == MB - 1) {   // last use of b[.][q] in this chunk: fetch the next chunk's
#pragma unroll
                                for (int j = J0; j < J1; ++j) b[j][q] = bn[j][q * LANES];
                            }
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
#pragma unroll
                  for (int m = 0; m < MB; ++m) {
                    const int r = rb * MB + m;
                    // popcount with the add fused (v_bcnt_u32_b32 d, m, d)
                    if constexpr (J0 == 0) {
                        asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(cnt[r]) : "v"(mlo[m][0]));
                        asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(cnt[r]) : "v"(mhi[m][0]));
                    }
                    if constexpr (J1 > 1) {
                        uint32_t t1;
                        asm("v_bcnt_u32_b32 %0, %1, 0" : "=v"(t1) : "v"(mlo[m][1]));
                        asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(t1) : "v"(mhi[m][1]));
                        cnt[r] = (t1 << 16) + cnt[r];   // v_lshl_add_u32
                    }
                  }
                    if (rb == 0 && ci == 0 && want_dma) {
                        SKL_STAGE_DMA(t + 1, buf ^ 1u);  // lands under this stage's VALU work
                        b_younger = 0;
                    }
                }
                ++b_younger;
            }
            if constexpr (PRUNE) {
                if (t + 1u == prune_next) {   // (workgroup-uniform)
                    // is every pair of the tile hopeless on THIS wave's chunks alone?  cnt[r] = (count of column block 1) << 16 |
                    // (count of column block 0) over the t + 1 stages walked
                    uint64_t alive = 0ull;
                    const uint32_t qc0 = prune_lds[lane], qc1 = prune_lds[LANES + lane];
                    const bool col0_ok = jb0 * 64u + lane < g.nB, col1_ok = (jb0 + 1u) * 64u + lane < g.nB;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (a0 + (uint32_t)r < g.row_end) {   // (uniform; rows past the band hold no pair)
                            const AliveBallots al = alive_pairs(cnt[r], prune_lds[PRUNE_ROW_BOUNDS + (uint32_t)r], qc0, qc1, col0_ok, col1_ok);
                            alive |= al.blk0 | al.blk1;
                        }
                    }
                    const uint32_t slot_ = PRUNE_VOTES + (prune_checks++ & 1u) * 4u;
                    if (lane == 0u) prune_lds[slot_ + wave] = alive != 0ull ? 1u : 0u;
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // (no vmcnt wait: the prefetches stay in flight)
                    const uint4 votes_ = *reinterpret_cast<const uint4 *>(&prune_lds[slot_]);
                    if ((votes_.x | votes_.y | votes_.z | votes_.w) == 0u) {
                        // hopeless as a whole: leave without storing.  No r_bits / t_bits bit is set for this tile, so the merges
                        // never read its records.  The prefetches in flight (row DMA into LDS!) must land first.
                        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                        if (g.prune_stats != nullptr && tid == 0u) {   // (one of 1 024 slots, as above)
                            atomicAdd(&g.prune_stats[(blockIdx.x & 1023u) * 4u + 1u], 1u);
                            atomicAdd(&g.prune_stats[(blockIdx.x & 1023u) * 4u + 2u], t + 1u);   // stages walked before leaving
                        }
                        return;
                    }
                    prune_next += max(1u, prune_next >> 1);
                    if (prune_next >= n_stages) prune_next = 0xFFFFFFFFu;
                }
            }
        }

#include "pair_kslice_finish.inc"
    }

#include "pair_kslice_coreacc.inc"
}
#undef SKL_WALK_BLOCKS
