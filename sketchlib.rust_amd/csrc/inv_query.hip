// inv_query.hip -- `inverted query` (src/inverted.rs:229-269) on the GPU (gfx950): for every query
// q and every indexed sample s, count(q, s) = #{ b : R[s][b] == q[b] } over the S u16 bins of the
// index sketches, then either the counts (match-count) or the predicate count > 0 (any-bins) /
// count == S (all-bins) as a bitmap.  The reference walks a HashMap<u16, RoaringBitmap> per bin and
// query on host threads; here it is a dense Q x N x S equality count.
//
//   1. inv_planes_kernel: u16 bins -> bit planes.  Word w of a row holds bins 32 w .. 32 w + 31;
//      plane p of that word has bit j = bit p of bin 32 w + j (16 planes: index bins are full u16
//      values, not the 14 planes of the pair kernels).  Bins past S are 0 on both sides and are
//      MASKED in the count, never compared.  The index is laid out [w][p][s] (adjacent lanes read
//      adjacent dwords); queries [w][q][p] (one query word = 64 contiguous bytes, one s_load_dwordx16).
//   2. inv_query_kernel: one lane per indexed sample, IQ_QTILE queries per workgroup.  Per (sample,
//      query, word): acc = ~(r_0 ^ q_0), then acc = acc & ~(r_p ^ q_p) for the other 15 planes, each
//      ONE v_bitop3_b32 (the query plane is wave-uniform and comes in an SGPR), then one v_bcnt_u32_b32
//      that adds the matching bins to the running count: 17 VALU per (pair, 32 bins), one AND more on
//      the last word, whose bins past S are masked off.  The 16 index planes of a word are loaded once
//      per lane and reused across the whole query tile; the next word's planes are in flight meanwhile.
//
// Query tile: 64.  The index planes are 64 B per (sample, word) and every query tile re-reads all of
// them: at 17 VALU lane-ops per (pair, word), a tile of T queries needs 17 T lane-ops per 64 B, i.e.
// 78.6 T lane-op/s / 6.3 TB/s = 12.5 lane-ops per byte balance -> T >= 47 to be VALU-bound from HBM
// alone.  64 is the next power of two; the tiles of one sample block are adjacent in dispatch order, so
// a block's planes mostly come from the caches after the first tile has read them.  The 64 counters live
// in VGPRs (104 VGPRs, 4 waves per SIMD).  Measured at N = 1 M, S = 1 000, Q = 1 024 (one kernel, every
// query tile): tiles of 32, 48 and 64 queries all take 15 ms (46-48 % of the VALU peak), 128 takes 27 ms
// (2 waves per SIMD).  What does matter is how the query planes arrive: one s_load_dwordx16 and one
// wait per query left 38 ms (18 %), the latency of each scalar load exposed; loading IQ_QGROUP = 4
// queries' planes at once and interleaving their four chains gives the 15 ms (2 per group: 23 ms; 8:
// no better than 4; the planes staged in LDS and read as broadcasts: the same 15 ms).
#include "kernels.h"

#include <type_traits>

namespace skl {

constexpr int IQ_THREADS = 256;
constexpr int IQ_QGROUP = 4;   // queries whose planes are loaded together (both tile sizes are multiples of it)
static_assert(IQ_QTILE % IQ_QGROUP == 0 && IQ_QTAIL % IQ_QGROUP == 0, "query tiles are whole groups");

__global__ __launch_bounds__(IQ_THREADS) void inv_planes_kernel(const InvPlanesArgs a)
{
    const uint64_t total = (uint64_t)a.rows * a.words;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(x % a.rows);   // adjacent threads: adjacent rows (coalesced index stores)
        const uint32_t w = (uint32_t)(x / a.rows);
        const uint16_t *src = a.bins + (uint64_t)row * a.sketch_size + (uint64_t)w * 32u;
        const uint32_t nb = min(32u, a.sketch_size - w * 32u);
        uint32_t pl[16];
#pragma unroll
        for (int p = 0; p < 16; ++p) pl[p] = 0u;
        for (uint32_t j = 0; j < nb; ++j) {
            const uint32_t v = src[j];
#pragma unroll
            for (int p = 0; p < 16; ++p) pl[p] |= ((v >> p) & 1u) << j;
        }
        uint32_t *dst = a.planes + (uint64_t)(a.row0 + row) * a.stride_row + (uint64_t)w * a.stride_word;
#pragma unroll
        for (int p = 0; p < 16; ++p) dst[(uint64_t)p * a.stride_plane] = pl[p];
    }
}

// QT queries per workgroup (IQ_QTILE for the full tiles of a launch, IQ_QTAIL for what is left): the query loop is
// unrolled whole so the counters stay in VGPRs.  The query planes are padded to whole tiles (zeros: counted, never stored)
// and laid out [w][q][p], so the planes of query j of the tile sit at a constant offset (64 j bytes) from the tile's word.
template <int QT>
__global__ __launch_bounds__(IQ_THREADS) void inv_query_kernel(const InvQueryArgs a)
{
    const uint32_t qt = blockIdx.x % a.n_qtiles;      // query tiles of one sample block are neighbours in dispatch order
    const uint32_t sb = blockIdx.x / a.n_qtiles;
    const uint32_t s = sb * IQ_THREADS + threadIdx.x;
    const bool live = s < a.n;
    const uint32_t s_ld = live ? s : a.n - 1u;        // dead lanes of the last block read a valid sample and store nothing
    const uint32_t q0 = a.q_first + qt * QT;
    const uint32_t nq = min((uint32_t)QT, a.nq - q0);
    const uint32_t W = a.words;
    const uint32_t *__restrict__ ref = a.ref_planes + s_ld;
    const uint32_t *__restrict__ qtile = a.q_planes + (uint64_t)q0 * 16u;
    const uint64_t q_word = (uint64_t)a.nq_pad * 16u;

    uint32_t cnt[QT];
#pragma unroll
    for (int j = 0; j < QT; ++j) cnt[j] = 0u;

    // one word of the tile: acc = ~(r_0 ^ q_0) & ~(r_1 ^ q_1) & ..., 1 + 15 VALU, then one v_bcnt_u32_b32 into the count;
    // the last word masks the bins past S first.  Queries go IQ_QGROUP at a time: their planes arrive in one batch of
    // scalar loads (one wait instead of one per query) and their chains interleave.
    uint32_t r[16];
    auto word = [&](const uint32_t *__restrict__ qw, auto masked) {
#pragma unroll
        for (int j0 = 0; j0 < QT; j0 += IQ_QGROUP) {
            uint32_t acc[IQ_QGROUP];
#pragma unroll
            for (int g = 0; g < IQ_QGROUP; ++g) acc[g] = ~(r[0] ^ qw[(j0 + g) * 16]);
#pragma unroll
            for (int p = 1; p < 16; ++p) {
#pragma unroll
                for (int g = 0; g < IQ_QGROUP; ++g) {
                    acc[g] = __builtin_amdgcn_bitop3_b32(acc[g], r[p], qw[(j0 + g) * 16 + p], 0x90);   // acc & ~(r ^ q)
                }
            }
#pragma unroll
            for (int g = 0; g < IQ_QGROUP; ++g) {
                if constexpr (decltype(masked)::value) acc[g] &= a.tail_mask;
                cnt[j0 + g] += __popc(acc[g]);
            }
        }
    };
#pragma unroll
    for (int p = 0; p < 16; ++p) r[p] = ref[(uint64_t)p * a.n];
    for (uint32_t w = 0; w + 1 < W; ++w) {
        uint32_t nxt[16];                             // the next word's planes load under this word's queries
#pragma unroll
        for (int p = 0; p < 16; ++p) nxt[p] = ref[((uint64_t)(w + 1) * 16u + p) * a.n];
        word(qtile + (uint64_t)w * q_word, std::false_type());
#pragma unroll
        for (int p = 0; p < 16; ++p) r[p] = nxt[p];
    }
    word(qtile + (uint64_t)(W - 1) * q_word, std::true_type());

    if (a.mode == INVQ_COUNTS) {
        if (live) {
#pragma unroll
            for (int j = 0; j < QT; ++j) {
                if ((uint32_t)j < nq) a.counts[(uint64_t)(q0 + j) * a.n + s] = cnt[j];
            }
        }
        return;
    }
    // predicate bitmap: one ballot per (wave, query); a wave covers the 64 samples from a multiple of 64
    const uint32_t wave_s0 = s - (threadIdx.x & 63u);
    const bool store = (threadIdx.x & 63u) == 0u && wave_s0 < a.n;
#pragma unroll
    for (int j = 0; j < QT; ++j) {
        const bool pred = live && (a.mode == INVQ_ANY ? cnt[j] > 0u : cnt[j] == a.sketch_size);
        const uint64_t bits = __ballot(pred);
        if (store && (uint32_t)j < nq) a.bits[(uint64_t)(q0 + j) * a.n_words64 + (wave_s0 >> 6)] = bits;
    }
}

hipError_t launch_inv_planes(const InvPlanesArgs &a, hipStream_t stream)
{
    const uint64_t total = (uint64_t)a.rows * a.words;
    if (total == 0) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((total + IQ_THREADS - 1) / IQ_THREADS, 1u << 16);
    hipLaunchKernelGGL(inv_planes_kernel, dim3((uint32_t)blocks), dim3(IQ_THREADS), 0, stream, a);
    return hipGetLastError();
}

// queries [0, nq) of the band: the full tiles of IQ_QTILE, then the rest in tiles of IQ_QTAIL
hipError_t launch_inv_query(const InvQueryArgs &args, hipStream_t stream)
{
    if (args.n == 0 || args.nq == 0) return hipSuccess;
    const uint64_t s_blocks = (args.n + IQ_THREADS - 1) / IQ_THREADS;
    InvQueryArgs a = args;
    const uint32_t full = args.nq / IQ_QTILE;
    if (full) {
        a.q_first = 0;
        a.n_qtiles = full;
        a.nq = full * IQ_QTILE;
        hipLaunchKernelGGL(inv_query_kernel<IQ_QTILE>, dim3((uint32_t)(s_blocks * a.n_qtiles)), dim3(IQ_THREADS), 0, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (args.nq > full * IQ_QTILE) {
        a.q_first = full * IQ_QTILE;
        a.nq = args.nq;
        a.n_qtiles = (args.nq - a.q_first + IQ_QTAIL - 1) / IQ_QTAIL;
        hipLaunchKernelGGL(inv_query_kernel<IQ_QTAIL>, dim3((uint32_t)(s_blocks * a.n_qtiles)), dim3(IQ_THREADS), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace skl
