// pair_kslice_coreacc.inc -- MODE_COREACC, after the last k-mer length of the walk (pair_kslice_walk.inc, included there): every
// wave finishes its SLOTS rows of the tile from the per-k totals it parked in hist[].  Text: as a function template over
// hist the all-k core/accessory forms compile to different vector code (profiles/kslice_split.md).
    if constexpr (MODE == MODE_COREACC) {
        // symmetric self kNN: (core, acc) of columns >= t_col_begin also leave turned, see MODE_JACCARD
        constexpr uint32_t TP = turned_pitch(R);
        static_assert(JL * 64 * TP * 8 <= (ROWS_U4 + RED_U4) * 16, "the turned tile fits the LDS of the workgroup");
        const bool turned = g.out_t != nullptr && min((jb0 + (uint32_t)JL) * 64u, g.nB) > g.t_col_begin;   // workgroup-uniform
        float2 *tt = reinterpret_cast<float2 *>(&lds_all[0]);
        if (turned) __syncthreads();   // every wave is done with the reduction words
        // store_coreacc() takes u16 fields, newest k lowest, as s2:s1:s0
#pragma clang loop unroll(disable)
        for (int i = 0; i < SLOTS; ++i) {
            const uint32_t r = (uint32_t)i * W + wave;   // (word x = row x of the tile)
            uint32_t word[MAX_FUSED_K];   // word[f]: totals of the k-mer length f steps from the newest
            if constexpr ((ABL & 16) != 0) {
                const uint32_t last_ = hist[i * MAX_FUSED_K + (nkk - 1u)];
#pragma unroll
                for (int f = 0; f < MAX_FUSED_K; ++f) word[f] = (uint32_t)f < nkk ? last_ : 0u;
            } else {
#pragma unroll
                for (int f = 0; f < MAX_FUSED_K; ++f) {
                    word[f] = (uint32_t)f < nkk ? hist[i * MAX_FUSED_K + (nkk - 1u - f)] : 0u;
                }
            }
#pragma clang loop unroll(disable)
            for (int h = 0; h < 2; ++h) {
                const uint32_t sh = h * 16u;
                const uint32_t s0 = ((word[0] >> sh) & 0xFFFFu) | (((word[1] >> sh) & 0xFFFFu) << 16);
                const uint32_t s1 = ((word[2] >> sh) & 0xFFFFu) | (((word[3] >> sh) & 0xFFFFu) << 16);
                const uint32_t s2 = ((word[4] >> sh) & 0xFFFFu) | (((word[5] >> sh) & 0xFFFFu) << 16);
                const float2 v = finish_key<float2>(g, a0 + r, jb0 + (uint32_t)h, lane_e, s0, s1, s2);
                if (turned) tt[((uint32_t)h * 64u + lane_e) * TP + r] = v;
            }
        }
        if (turned) {
            __syncthreads();
            store_turned_tile<float2, R, JL>(g, tt, jb0, a0, tid);
        }
    }
