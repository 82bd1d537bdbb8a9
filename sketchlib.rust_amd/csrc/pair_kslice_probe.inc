// pair_kslice_probe.inc -- tile pruning BEFORE the walk of pair_kslice_walk.inc (PRUNE launches, included there): the
// plane-pair probe, run by the whole workgroup before anything of the walk is requested, and the sparse walk with its finish
// for a tile that survives the probe for a few rows only.  A tile that is done with here (hopeless and left unwritten, or
// finished by the sparse walk) returns from the kernel; otherwise prune_next holds the stage count of the walk's first
// stage-boundary check.  Text, not a function: as a __forceinline__ function template hipcc schedules two blocks of the
// walk that FOLLOWS differently (profiles/kslice_split.md).
        if (g.prune_q_rows != nullptr) {
            // Everything the probe needs is requested AT ONCE, before any of it is looked at: the bounds of the tile's columns
            // (2 per lane) and rows (lane r: row r), and -- speculatively, the plan is not known yet -- the plane pairs of the
            // probe's first PRE steps (rows: one 16-byte load per lane and two steps; columns: two per step).
            constexpr uint32_t PRE = 4;                  // probe steps fetched before the plan is known
            static_assert(64 % R == 0 && R <= 64, "a trip of the row fetch covers whole probe steps");
            const uint32_t per_wave = (c_end - c_begin) / (uint32_t)W;   // chunks every wave has
            const uint32_t k_ = g.k_begin + kk0;
            uint32_t qcol[JL];
        #pragma unroll
            for (int j = 0; j < JL; ++j) {
                const uint32_t jc = (jb0 + (uint32_t)j) * 64u + lane;
                qcol[j] = jc < g.nB ? g.prune_q_cols[jc] : 0u;   // (columns past the end hold no pair)
            }
            const uint32_t qrow = (lane < (uint32_t)R && a0 + lane < g.row_end) ? g.prune_q_rows[a0 + lane] : 0u;   // (rows past the band hold no pair)
            auto row_pair = [&](uint32_t item) -> uint4 {   // plane pair 0 of row item % R at probe step item / R: (lo0, hi0, lo1, hi1)
                const uint32_t step = item / (uint32_t)R, r = item % (uint32_t)R;
                const uint32_t c_ = min(c_begin + wave + step * (uint32_t)W, g.ss64 - 1u);
                return a0 + r < g.row_end
                           ? *reinterpret_cast<const uint4 *>(g.A + (size_t)(a0 + r) * sample_stride + (size_t)k_ * kmer_stride + (size_t)c_ * BBITS)
                           : make_uint4(0u, 0u, 0u, 0u);
            };
            auto col_pair = [&](int j, uint32_t step) -> uint4 {   // plane pair 0 of this lane's column in block j: (hi0, lo0, hi1, lo1)
                const uint32_t jb = (jb0 + j) < g.n_jblocks ? (jb0 + j) : (g.n_jblocks - 1u);   // clamped, masked in the vote
                const uint32_t c_ = min(c_begin + wave + step * (uint32_t)W, g.ss64 - 1u);
                return g.B[(((size_t)jb * g.nk + k_) * g.ss64 + c_) * (7 * LANES) + lane];
            };
            constexpr uint32_t PRE_TRIPS = (PRE * (uint32_t)R + 63u) / 64u;
            uint4 pre_rows[PRE_TRIPS], pre_cols[PRE][JL];
        #pragma unroll
            for (uint32_t u = 0; u < PRE_TRIPS; ++u) pre_rows[u] = row_pair(u * 64u + lane);
        #pragma unroll
            for (uint32_t st = 0; st < PRE; ++st) {
        #pragma unroll
                for (int j = 0; j < JL; ++j) pre_cols[st][j] = col_pair(j, st);
            }
            // the bounds: column bounds and row bounds to LDS (every wave writes the same values), the largest of all of them
            uint32_t qmax = max(qrow, max(qcol[0], qcol[JL - 1]));
        #pragma unroll
            for (int j = 0; j < JL; ++j) prune_lds[j * LANES + lane] = qcol[j];
            if (lane < (uint32_t)R) prune_lds[PRUNE_ROW_BOUNDS + lane] = qrow;
        #pragma unroll
            for (int sh = 32; sh >= 1; sh >>= 1) qmax = max(qmax, (uint32_t)__shfl_xor((int)qmax, sh));
            qmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)qmax);
            // (1) PLANE-PAIR PROBE, before anything of the walk is requested.  A bin that differs in ANY plane mismatches, so the
            // mismatches seen in planes 0 and 1 alone are a lower bound of a pair's count -- and an unrelated pair shows 3/4 of
            // its bins there (48 per chunk) for 1/7 of the loads and 1/5 of the instructions of the full comparison.  Each wave
            // takes `need` of its own chunks (the first ones; chosen so that an unrelated pair reaches the tile's largest bound
            // with a margin), rows staged through the wave's own (still idle) row buffer and read back by broadcast, columns as
            // one coalesced 16-byte load per lane, chunk and column block; then the same vote as at a stage boundary.  A tile that
            // is hopeless leaves here; one that is not starts its walk as if nothing had happened.
            const uint32_t need = (qmax + 16u) / 44u + 1u;
            if (need <= per_wave && need <= 16u) {   // (workgroup-uniform)
                uint4 *prows = &lds_rows[wave][0][0];   // (this wave's own row buffers: dead until the walk's first DMA, issued after the probe)
        #pragma unroll
                for (uint32_t u = 0; u < PRE_TRIPS; ++u) prows[u * 64u + lane] = pre_rows[u];
                for (uint32_t item = PRE_TRIPS * 64u + lane; item < need * (uint32_t)R; item += 64u) prows[item] = row_pair(item);
                uint32_t pc[R];
        #pragma unroll
                for (int r = 0; r < R; ++r) pc[r] = 0u;
                auto probe_step = [&](uint32_t step, const uint4 &b0_, const uint4 &b1_) {
        #pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const uint4 ar = prows[step * (uint32_t)R + (uint32_t)r];   // (uniform address: one broadcast read)
                        const uint32_t l0 = (ar.x ^ b0_.y) | (ar.z ^ b0_.w), h0 = (ar.y ^ b0_.x) | (ar.w ^ b0_.z);
                        const uint32_t l1 = (ar.x ^ b1_.y) | (ar.z ^ b1_.w), h1 = (ar.y ^ b1_.x) | (ar.w ^ b1_.z);
                        pc[r] += (uint32_t)(__popc(l0) + __popc(h0)) + ((uint32_t)(__popc(l1) + __popc(h1)) << 16);
                    }
                };
        #pragma unroll
                for (uint32_t st = 0; st < PRE; ++st) {
                    if (st < need) probe_step(st, pre_cols[st][0], pre_cols[st][JL - 1]);
                }
                if (need > PRE) {   // (bounds beyond what 4 steps show: the next step's columns are requested a step ahead)
                    uint4 nb0 = col_pair(0, PRE), nb1 = col_pair(JL - 1, PRE);
                    for (uint32_t step = PRE; step < need; ++step) {
                        const uint4 b0_ = nb0, b1_ = nb1;
                        if (step + 1u < need) {
                            nb0 = col_pair(0, step + 1u);
                            nb1 = col_pair(JL - 1, step + 1u);
                        }
                        probe_step(step, b0_, b1_);
                    }
                }
                uint64_t alive = 0ull;
                const bool col0_ok = jb0 * 64u + lane < g.nB, col1_ok = (jb0 + 1u) * 64u + lane < g.nB;
        #pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (a0 + (uint32_t)r < g.row_end) {
                        const AliveBallots al = alive_pairs(pc[r], prune_lds[PRUNE_ROW_BOUNDS + (uint32_t)r], qcol[0], qcol[1], col0_ok, col1_ok);
                        alive |= al.blk0 | al.blk1;
                    }
                }
                const uint32_t slot_ = PRUNE_VOTES + (prune_checks++ & 1u) * 4u;
                if (lane == 0u) prune_lds[slot_ + wave] = alive != 0ull ? 1u : 0u;
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                const uint4 votes_ = *reinterpret_cast<const uint4 *>(&prune_lds[slot_]);
                if ((votes_.x | votes_.y | votes_.z | votes_.w) == 0u) {
                    // (counted in one of 1 024 slots: sixty million adds to ONE address queue up behind each other, and a wave
                    // does not end before its add has been taken -- that queue was most of a pruned tile's time)
                    if (g.prune_stats != nullptr && tid == 0u) atomicAdd(&g.prune_stats[(blockIdx.x & 1023u) * 4u], 1u);
                    return;
                }
                // The tile survives.  WHICH rows of it, and which of its two column blocks, still hold a pair that is not hopeless
                // on some wave's chunks?  (a second vote, paid by the survivors only: the tiles that leave above pay what they did)
                uint32_t rows_alive = 0xFFFFFFFFu, blks_alive = 3u;
                if ((g.prune_flags & 1u) == 0u) {
                    uint32_t rowmask = 0u, blkmask = 0u;
        #pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (a0 + (uint32_t)r < g.row_end) {
                            const AliveBallots al = alive_pairs(pc[r], prune_lds[PRUNE_ROW_BOUNDS + (uint32_t)r], qcol[0], qcol[1], col0_ok, col1_ok);
                            if ((al.blk0 | al.blk1) != 0ull) rowmask |= 1u << r;
                            if (al.blk0 != 0ull) blkmask |= 1u;
                            if (al.blk1 != 0ull) blkmask |= 2u;
                        }
                    }
                    constexpr uint32_t PROBE_VOTES = PRUNE_ROW_BOUNDS + (uint32_t)R;   // 4 row masks, 4 block masks (the probe's own words:
                                                                                 // the rotating vote rows belong to the checks)
                    if (lane == 0u) {
                        prune_lds[PROBE_VOTES + wave] = rowmask;
                        prune_lds[PROBE_VOTES + 4u + wave] = blkmask;
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                    const uint4 rv_ = *reinterpret_cast<const uint4 *>(&prune_lds[PROBE_VOTES]);
                    const uint4 bv_ = *reinterpret_cast<const uint4 *>(&prune_lds[PROBE_VOTES + 4u]);
                    rows_alive = (uint32_t)__builtin_amdgcn_readfirstlane((int)(rv_.x | rv_.y | rv_.z | rv_.w));
                    blks_alive = (uint32_t)__builtin_amdgcn_readfirstlane((int)(bv_.x | bv_.y | bv_.z | bv_.w));
                }
                // (1b) SPARSE WALK.  A tile that survives the probe usually does so for ONE pair (a relative among 4 096 pairs): every
                // pair outside the alive rows -- and outside the alive column block -- is as hopeless as a pruned tile's.  With at
                // most SPARSE_ROWS alive rows the wave walks its chunks for those rows only: their plane pairs staged through the
                // wave's row buffers a batch of chunks at a time (one 16-byte load per lane and 64 pieces) and read back by
                // broadcast, the alive blocks' columns as in the dense walk, ~60 VALU instructions per (row, block, chunk)
                // instead of 2 000 per chunk -- the walk turns from VALU bound to bound by the column loads.  The hopeless pairs get
                // the count "every bin differs" (the worst key there is: no mark, rejected by both lists like their true value,
                // which lies beyond both bounds), and the tile goes through the ordinary reduction and stores.
                constexpr uint32_t SPARSE_ROWS = 4u, SPARSE_BATCH = 16u;
                static_assert(SPARSE_BATCH * SPARSE_ROWS * 7u <= 2u * BUF_U4, "a batch of row pieces fits the wave's two row buffers");
                const uint32_t n_alive = (uint32_t)__popc(rows_alive);
                if (n_alive <= SPARSE_ROWS) {   // (workgroup-uniform)
                    uint32_t rl[SPARSE_ROWS], cs[SPARSE_ROWS];
                    {
                        uint32_t m_ = rows_alive;
        #pragma unroll
                        for (uint32_t x = 0; x < SPARSE_ROWS; ++x) {
                            rl[x] = m_ != 0u ? (uint32_t)__builtin_ctz(m_) : 0u;
                            m_ &= m_ - 1u;
                            cs[x] = 0u;
                        }
                    }
                    const uint32_t first_c = c_begin + wave;
                    const uint32_t n_w = first_c < c_end ? (c_end - first_c + (uint32_t)W - 1u) / (uint32_t)W : 0u;   // this wave's chunks
                    for (uint32_t s0_ = 0; s0_ < n_w; s0_ += SPARSE_BATCH) {
                        const uint32_t nb = min(SPARSE_BATCH, n_w - s0_);
                        // piece ((step * n_alive + x) * 7 + q): plane pair q of alive row x at the batch's chunk `step`
                        for (uint32_t item = lane; item < nb * n_alive * 7u; item += 64u) {
                            const uint32_t q_ = item % 7u, sx_ = item / 7u, x_ = sx_ % n_alive, st_ = sx_ / n_alive;
                            const uint32_t r_ = x_ == 0u ? rl[0] : (x_ == 1u ? rl[1] : (x_ == 2u ? rl[2] : rl[3]));
                            const uint32_t c_ = first_c + (s0_ + st_) * (uint32_t)W;
                            prows[item] = *reinterpret_cast<const uint4 *>(g.A + (size_t)(a0 + r_) * sample_stride + (size_t)k_ * kmer_stride +
                                                                           (size_t)c_ * BBITS + 2u * q_);
                        }
                        for (uint32_t st_ = 0; st_ < nb; ++st_) {
                            const uint32_t c_ = first_c + (s0_ + st_) * (uint32_t)W;
                            uint4 bb[JL][7];
        #pragma unroll
                            for (int j = 0; j < JL; ++j) {
                                if ((blks_alive >> j) & 1u) {
                                    const uint32_t jb = (jb0 + j) < g.n_jblocks ? (jb0 + j) : (g.n_jblocks - 1u);
                                    const uint4 *bp = g.B + (((size_t)jb * g.nk + k_) * g.ss64 + c_) * (7 * LANES) + lane;
        #pragma unroll
                                    for (int q = 0; q < 7; ++q) bb[j][q] = bp[q * LANES];
                                }
                            }
        #pragma unroll
                            for (uint32_t x = 0; x < SPARSE_ROWS; ++x) {
                                if (x < n_alive) {
                                    uint4 ar[7];
        #pragma unroll
                                    for (int q = 0; q < 7; ++q) ar[q] = prows[(st_ * n_alive + x) * 7u + (uint32_t)q];   // (uniform address: broadcast)
        #pragma unroll
                                    for (int j = 0; j < JL; ++j) {
                                        if ((blks_alive >> j) & 1u) {
                                            uint32_t mlo = ar[0].x ^ bb[j][0].y, mhi = ar[0].y ^ bb[j][0].x;
                                            mlo = acc_mismatch_vvv(mlo, ar[0].z, bb[j][0].w);
                                            mhi = acc_mismatch_vvv(mhi, ar[0].w, bb[j][0].z);
        #pragma unroll
                                            for (int q = 1; q < 7; ++q) {
                                                mlo = acc_mismatch_vvv(mlo, ar[q].x, bb[j][q].y);
                                                mhi = acc_mismatch_vvv(mhi, ar[q].y, bb[j][q].x);
                                                mlo = acc_mismatch_vvv(mlo, ar[q].z, bb[j][q].w);
                                                mhi = acc_mismatch_vvv(mhi, ar[q].w, bb[j][q].z);
                                            }
                                            cs[x] += (uint32_t)(__popc(mlo) + __popc(mhi)) << (16 * j);
                                        }
                                    }
                                }
                            }
                        }
                    }
                    // The alive rows' partial counts meet in LDS (each wave's first row buffer, which its staging is done with),
                    // and ONE wave finishes the tile: at most 4 rows x 2 blocks of keys per lane instead of the 32 x 2 of the
                    // ordinary reduction.  Only what can be read is written: an alive row's alive blocks to the band (a block
                    // of a row is read by the merge only if a key in it marks it -- and a hopeless pair cannot), and for the
                    // turned copy the 32-row stretch of the columns an alive key marks (the other rows of such a stretch hold
                    // the worst key there is, like their true value rejected by the column's list).
                    static_assert(R == 32, "the sparse finish is written for the 32-row single-k form");
                    const uint32_t all_ = n_w * 64u;   // this wave's share of "every bin differs", for the fields of a block that is not alive
                    const uint32_t dead_fields = ((blks_alive & 1u) ? 0u : all_) | ((blks_alive & 2u) ? 0u : all_ << 16);
                    uint32_t *spw = reinterpret_cast<uint32_t *>(&lds_all[0]);
        #pragma unroll
                    for (uint32_t x = 0; x < SPARSE_ROWS; ++x) spw[((wave * 2u) * (BUF_U4 * 4u)) + x * LANES + lane] = cs[x] | dead_fields;
                    __syncthreads();
                    if (wave != 0u) return;
                    if (g.prune_stats != nullptr && lane == 0u) atomicAdd(&g.prune_stats[(blockIdx.x & 1023u) * 4u + 3u], 1u);
                    const float v_dead = g.dtab[0];   // no bin in common
                    float val[SPARSE_ROWS][JL];
        #pragma unroll
                    for (uint32_t x = 0; x < SPARSE_ROWS; ++x) {
        #pragma unroll
                        for (int h = 0; h < JL; ++h) val[x][h] = v_dead;
                        if (x < n_alive) {
                            uint32_t total = 0u;
        #pragma unroll
                            for (uint32_t w = 0; w < (uint32_t)W; ++w) total += spw[((w * 2u) * (BUF_U4 * 4u)) + x * LANES + lane];
        #pragma unroll
                            for (int h = 0; h < JL; ++h) {
                                if ((blks_alive >> h) & 1u) val[x][h] = finish_key<float, false>(g, a0 + rl[x], jb0 + (uint32_t)h, lane, h ? (total >> 16) : (total & 0xFFFFu));
                            }
                        }
                    }
                    if (g.out_t != nullptr && min((jb0 + (uint32_t)JL) * 64u, g.nB) > g.t_col_begin) {
        #pragma unroll
                        for (int h = 0; h < JL; ++h) {
                            const uint32_t jc = (jb0 + (uint32_t)h) * 64u + lane;
                            if (((blks_alive >> h) & 1u) && jc >= g.t_col_begin && jc < g.nB) {
                                float best = val[0][h];
        #pragma unroll
                                for (uint32_t x = 1; x < SPARSE_ROWS; ++x) best = fminf(best, val[x][h]);
                                if (g.t_flag == nullptr || mark_turned(g, jc, a0 - g.row_begin, best)) {   // (a 32-row tile is one stretch)
                                    float *dst = &g.out_t[(size_t)(jc - g.t_col_begin) * g.t_stride + (a0 - g.row_begin)];
        #pragma unroll
                                    for (uint32_t q = 0; q < (uint32_t)R / 4u; ++q) {
                                        float4 f = make_float4(v_dead, v_dead, v_dead, v_dead);
        #pragma unroll
                                        for (uint32_t x = 0; x < SPARSE_ROWS; ++x) {
                                            if (x < n_alive && (rl[x] >> 2) == q) {   // (uniform)
                                                const uint32_t e_ = rl[x] & 3u;
                                                if (e_ == 0u) f.x = val[x][h];
                                                else if (e_ == 1u) f.y = val[x][h];
                                                else if (e_ == 2u) f.z = val[x][h];
                                                else f.w = val[x][h];
                                            }
                                        }
                                        *reinterpret_cast<float4 *>(dst + 4u * q) = f;
                                    }
                                }
                            }
                        }
                    }
                    return;
                }
            }
            // (2) ... and checks at stage boundaries of the walk, for the tiles the probe could not settle (bounds beyond what its
            // chunks can show: after s stages an unrelated pair has 64 s mismatches on every wave, 63 s with a chance match or two).
            // The first check sits where the tile's largest bound is reached, the next ones 1.5 x later each.
            const uint32_t s0 = max(1u, (qmax + 63u * CH - 1u) / (63u * CH));
            if (s0 < n_stages) prune_next = s0;
        }
