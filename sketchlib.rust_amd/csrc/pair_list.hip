// pair_list.hip -- distances of an explicit list of sample pairs (gfx950).
//
// Every other distance call fills a whole shape (triangle, row band, rectangle, kNN lists); this one answers "the core and
// accessory distance of THESE pairs": core_acc_dist + simple_linear_regression (src/distances/jaccard.rs:61-142) or the
// single-k Jaccard / ANI value (src/distances/mod.rs:83-100) of list entry x = (a[x], b[x]), stored at out[x].  A pure
// gather: no compaction, no atomics, no LDS.
//
// The wave form is pair_cand.hip's pair_cand_rows_kernel: a work item is a run of consecutive entries with the same `a`
// (cut at 64; a shuffled list gives runs of one), the lanes go ACROSS THE SKETCH (lane l takes the l-th half chunk of a
// trip: 7 planes, 56 bytes), the run's partners are taken one after the other and each partner's record -- all its k-mer
// lengths, nk x ss64 x 112 bytes, contiguous in the reference layout -- is walked in order.  The counts are wave-uniform
// after wave_sum (device_common.hpp); partner p's are kept by lane p, and once the run is counted every lane fits ITS
// partner (coreacc_value_counts / jaccard_out_value): up to 64 fits side by side, one float2 / float store per lane.
//
// A partner's record is read as ONE flat run of half chunks -- length after length, as it lies in memory -- and all the
// loads a step needs are issued unconditionally (a lane past the end reads the last half chunk again and only its COUNT is
// masked), so nothing but the data itself stands between a load and the next one:
// pair_list_kernel<FT, COUNTS_OUT>:
//   FT = 1, 2, 3   the walked part of a record (lengths x 2 x ss64 half chunks) fits FT trips of 64 lanes -- 4 lengths x 16
//             chunks are 2 trips with every lane busy.  The ROW's planes are read once per work item and stay in registers
//             (14 per trip); a partner's loads are independent and no branch stands between them (as compiled: issued back
//             to back under counted waits, as many ahead of the folds as registers allow, one full wait per partner); a
//             lane's share goes to the length its half chunk belongs to and one wave_sum per length follows;
//   FT = 0    any sketch size: steps of 64 half chunks, length by length and partner by partner in ONE loop, the row's planes
//             re-read (L1) beside the partner's, and the NEXT step's planes -- the next trip, the next length or the next
//             partner's first -- requested before the current step is folded;
//   COUNTS_OUT (FT = 0 only)  more than MAX_FUSED_K lengths: the counts go to memory and pair_list_fit_kernel fits them
//             with the lengths read from a device array.
// The reference's `break` (jaccard.rs:89-91) is NOT used to cut a partner's walk short: every length is counted, the fit
// ignores what follows the break as the reference does.
#include "device_common.hpp"

namespace skl {

template <int FT, bool COUNTS_OUT>
__global__ __launch_bounds__(LANES *WAVES_PER_WG) void pair_list_kernel(const PairListArgs c, const PairArgs g)
{
    constexpr bool KEEP = FT > 0;
    static_assert(!(KEEP && COUNTS_OUT), "the counts-to-memory form is the stepped one");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (grid = blocks_per_xcd << xcd_shift exactly: every workgroup has a block number; the items past n_work leave below)
    const uint32_t blk = (blockIdx.x & ((1u << c.xcd_shift) - 1u)) * c.blocks_per_xcd + (blockIdx.x >> c.xcd_shift);
    const uint64_t w = c.work_base + (uint64_t)blk * WAVES_PER_WG + wave;
    if (w >= c.work_end) return;
    const uint32_t start = c.work_start[w];
    const uint32_t cnt = c.work_start[w + 1] - start;        // 1 ... 64
    const uint32_t row = (uint32_t)__builtin_amdgcn_readfirstlane((int)c.pair_a[start]);
    const uint32_t j_mine = lane < cnt ? c.pair_b[start + lane] : 0u;
    const size_t kmer_stride = (size_t)g.ss64 * BBITS;
    const size_t sample_stride = kmer_stride * g.nk;
    const uint32_t halves = g.ss64 * 2u;                     // half chunks of 7 planes (56 bytes) per (sample, length)
    const uint32_t maxnbits = g.ss64 * 64u;
    const uint32_t nkw = g.k_count;                          // lengths walked, from k_begin on
    const uint2 *pi = reinterpret_cast<const uint2 *>(g.A + (size_t)row * sample_stride + (size_t)g.k_begin * kmer_stride);
    auto partner = [&](uint32_t cc) -> const uint2 * {       // (cc is wave-uniform)
        const uint32_t j = (uint32_t)__builtin_amdgcn_readlane((int)j_mine, (int)cc);
        return reinterpret_cast<const uint2 *>(c.b_rows + (size_t)j * sample_stride + (size_t)g.k_begin * kmer_stride);
    };
    uint32_t same_mine[MAX_FUSED_K];
#pragma unroll
    for (int t = 0; t < MAX_FUSED_K; ++t) same_mine[t] = 0u;
    if constexpr (KEEP) {
        const uint32_t flat = nkw * halves;                  // half chunks of the walked part of a record: <= 64 FT
        uint2 a_row[FT][7];
        uint32_t at[FT], t_of[FT];
        bool counted[FT];
#pragma unroll
        for (int tr = 0; tr < FT; ++tr) {
            const uint32_t f = (uint32_t)tr * 64u + lane;
            counted[tr] = f < flat;
            const uint32_t fc = counted[tr] ? f : flat - 1u;
            at[tr] = fc * 7u;
            t_of[tr] = fc / halves;                          // the length this lane's half chunk belongs to
#pragma unroll
            for (int q = 0; q < 7; ++q) a_row[tr][q] = pi[at[tr] + q];
        }
        for (uint32_t cc = 0; cc < cnt; ++cc) {
            const uint2 *pj = partner(cc);
            uint2 b[FT][7];
#pragma unroll
            for (int tr = 0; tr < FT; ++tr) {
#pragma unroll
                for (int q = 0; q < 7; ++q) b[tr][q] = pj[at[tr] + q];   // unconditional: nothing but registers between a partner's loads
            }
            uint32_t part[MAX_FUSED_K];
#pragma unroll
            for (int t = 0; t < MAX_FUSED_K; ++t) part[t] = 0u;
#pragma unroll
            for (int tr = 0; tr < FT; ++tr) {
                uint32_t mlo = 0, mhi = 0;
                half_chunk_fold(a_row[tr], b[tr], mlo, mhi);
                const uint32_t share = half_chunk_share(mlo, mhi, lane, counted[tr]);
#pragma unroll
                for (int t = 0; t < MAX_FUSED_K; ++t) part[t] += t_of[tr] == (uint32_t)t ? share : 0u;
            }
#pragma unroll
            for (int t = 0; t < MAX_FUSED_K; ++t) {
                if ((uint32_t)t < nkw) {
                    const uint32_t total = wave_sum(part[t]);
                    if (lane == cc) same_mine[t] = maxnbits - total;
                }
            }
        }
    } else {
        const uint32_t steps_per_length = (halves + 63u) >> 6;
        const uint32_t n_steps = cnt * nkw * steps_per_length;
        // planes of step (length t, trip tr) of a record: a lane past the length's end re-reads its last half chunk
        auto offset = [&](uint32_t t, uint32_t tr) -> size_t {
            const uint32_t h = tr * 64u + lane;
            return ((size_t)t * halves + (h < halves ? h : halves - 1u)) * 7u;
        };
        uint2 a[7], b[7];
        {
            const uint2 *pj = partner(0);
            const size_t o = offset(0, 0);
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                a[q] = pi[o + q];
                b[q] = pj[o + q];
            }
        }
        uint32_t cc = 0, t = 0, tr = 0, part = 0;            // the current step (wave-uniform) and its length's share so far
        for (uint32_t s = 0; s < n_steps; ++s) {
            uint32_t ncc = cc, nt = t, ntr = tr + 1u;        // the step after it: next trip, next length, next partner
            if (ntr == steps_per_length) {
                ntr = 0;
                if (++nt == nkw) {
                    nt = 0;
                    ++ncc;
                }
            }
            if (s + 1u == n_steps) {                         // (the last step requests itself again)
                ncc = cc;
                nt = t;
                ntr = tr;
            }
            uint2 an[7], bn[7];                              // in flight under this step's count
            {
                const uint2 *pj = partner(ncc);
                const size_t o = offset(nt, ntr);
#pragma unroll
                for (int q = 0; q < 7; ++q) {
                    an[q] = pi[o + q];                       // the row's: the same addresses for every partner of the run (L1)
                    bn[q] = pj[o + q];
                }
            }
            uint32_t mlo = 0, mhi = 0;
            half_chunk_fold(a, b, mlo, mhi);
            part += half_chunk_share(mlo, mhi, lane, tr * 64u + lane < halves);
            if (tr + 1u == steps_per_length) {               // the length is counted
                const uint32_t same = maxnbits - wave_sum(part);
                part = 0;
                if constexpr (COUNTS_OUT) {
                    if (lane == cc) c.counts[(uint64_t)(start + cc) * nkw + t] = same;
                } else {
#pragma unroll
                    for (int x = 0; x < MAX_FUSED_K; ++x) {
                        if (lane == cc && t == (uint32_t)x) same_mine[x] = same;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                a[q] = an[q];
                b[q] = bn[q];
            }
            cc = ncc;
            t = nt;
            tr = ntr;
        }
    }
    if constexpr (!COUNTS_OUT) {
        if (lane < cnt) {   // every lane its own partner
            if (c.coreacc) ((float2 *)c.out)[start + lane] = coreacc_value_counts(g, row, j_mine, same_mine);
            else ((float *)c.out)[start + lane] = jaccard_out_value(g, row, j_mine, maxnbits - same_mine[0]);
        }
    }
}

// ... and the fit of counts parked in memory (more than MAX_FUSED_K lengths): one thread per entry
__global__ __launch_bounds__(256) void pair_list_fit_kernel(const PairListArgs c, const PairArgs g, uint64_t first)
{
    const uint64_t x = first + (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (x >= c.n_entries) return;
    ((float2 *)c.out)[x] = coreacc_fit_counts<0>(g, c.pair_a[x], c.pair_b[x], c.counts + x * g.k_count, c.kf);
}

namespace {
constexpr uint64_t MAX_BLOCKS_PER_LAUNCH = 1ull << 23;

// flat trips of the form that keeps the row's planes in registers (1 ... 3), or 0: the stepped form
int pair_list_flat_trips(const PairArgs &g)
{
    const uint64_t flat = (uint64_t)g.k_count * g.ss64 * 2u;
    return g.k_count <= (uint32_t)MAX_FUSED_K && flat <= 3u * 64u ? (int)((flat + 63u) / 64u) : 0;
}

template <int FT, bool COUNTS_OUT>
void launch_form(const PairListArgs &c, const PairArgs &g, unsigned grid, hipStream_t stream)
{
    hipLaunchKernelGGL((pair_list_kernel<FT, COUNTS_OUT>), dim3(grid), dim3(LANES * WAVES_PER_WG), 0, stream, c, g);
}
}  // namespace

const char *pair_list_kernel_name(const PairArgs &g)
{
    if (pair_list_flat_trips(g)) return "skl::pair_list_kernel (a run of up to 64 listed pairs per wave, partners one after the other, a partner's record as one flat run, all its planes requested at once; the row's planes in registers)";
    if (g.k_count <= (uint32_t)MAX_FUSED_K) return "skl::pair_list_kernel (a run of up to 64 listed pairs per wave, partners one after the other, every length of a partner's record in order, the next step's planes requested ahead; the row's planes re-read)";
    return "skl::pair_list_kernel (a run of up to 64 listed pairs per wave, partners one after the other, every length of a partner's record in order, the next step's planes requested ahead; counts to memory) + skl::pair_list_fit_kernel";
}

hipError_t launch_pair_list(const PairListArgs &c_in, const PairArgs &g, hipStream_t stream)
{
    PairListArgs c = c_in;
    if (c.n_work == 0) return hipSuccess;
    const bool counts_out = g.k_count > (uint32_t)MAX_FUSED_K;
    if (counts_out && (!c.coreacc || !c.counts || !c.kf)) return hipErrorInvalidValue;
    c.xcd_shift = g.xcd_shift;
    const uint64_t items_per_launch = MAX_BLOCKS_PER_LAUNCH * WAVES_PER_WG;
    for (uint64_t base = 0; base < c.n_work; base += items_per_launch) {
        const uint64_t items = std::min<uint64_t>(items_per_launch, c.n_work - base);
        const uint64_t blocks = (items + WAVES_PER_WG - 1) / WAVES_PER_WG;
        c.work_base = base;
        c.work_end = base + items;
        // rounded up to whole XCD rounds: block numbers past `blocks` hold only items >= work_end, which leave at once
        c.blocks_per_xcd = (uint32_t)((blocks + (1ull << c.xcd_shift) - 1) >> c.xcd_shift);
        const unsigned grid = (unsigned)((uint64_t)c.blocks_per_xcd << c.xcd_shift);
        switch (pair_list_flat_trips(g)) {
            case 1: launch_form<1, false>(c, g, grid, stream); break;
            case 2: launch_form<2, false>(c, g, grid, stream); break;   // (4 lengths x 16 chunks: `sketch -s 1000`)
            case 3: launch_form<3, false>(c, g, grid, stream); break;
            default:
                if (counts_out) launch_form<0, true>(c, g, grid, stream);
                else launch_form<0, false>(c, g, grid, stream);
                break;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (counts_out) {
        const uint64_t per_launch = MAX_BLOCKS_PER_LAUNCH * 256u;
        for (uint64_t first = 0; first < c.n_entries; first += per_launch) {
            const uint64_t entries = std::min<uint64_t>(per_launch, c.n_entries - first);
            hipLaunchKernelGGL(pair_list_fit_kernel, dim3((unsigned)((entries + 255u) / 256u)), dim3(256), 0, stream, c, g, first);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace skl
