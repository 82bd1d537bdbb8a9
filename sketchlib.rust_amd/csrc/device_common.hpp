// device_common.hpp -- device-side helpers shared by the pair kernels: the bin-match
// primitive and the per-pair epilogues (Jaccard / ANI / core-accessory regression),
// each a restatement of the reference function it cites.
#pragma once

#include "glibc_log.hpp"
#include "kernels.h"

namespace skl {

// m | (a ^ b) in one instruction: v_bitop3_b32 with truth table 0xDE for
// (src0 = a, src1 = m, src2 = b).
template <bool BITOP3>
__device__ __forceinline__ uint32_t acc_mismatch(uint32_t m, uint32_t a, uint32_t b)
{
    if constexpr (BITOP3) {
        return __builtin_amdgcn_bitop3_b32(a, m, b, 0xDE);
    } else {
        return m | (a ^ b);
    }
}

// Same function with the operands placed for the register file (all-VGPR form used by the
// LDS kernel): src0 = row dword, src1 = column dword, src2 = accumulator; truth table
// (F0 ^ CC) | AA = 0xBE.  Measured on MI355X (scripts/microbench/vgpr_banks.hip):
// v_bitop3_b32 issues at half rate exactly when src0 and src1 come from the same VGPR bank
// (register index mod 4); src2 and the destination are free.  The column slab stores each
// plane as (hi, lo), so the dword that pairs with the row's even-register component always
// sits in an odd register and vice versa (128-bit VGPR tuples are even-aligned on gfx950):
// the conflict cannot occur, whatever the register allocator does.
__device__ __forceinline__ uint32_t acc_mismatch_vvv(uint32_t m, uint32_t a, uint32_t b)
{
    return __builtin_amdgcn_bitop3_b32(a, b, m, 0xBE);
}

// 16 bytes per lane, global -> LDS, no VGPR destination (global_load_lds_dwordx4): lane l's
// 16 bytes land at LDS byte address m0 + 16*l.  Issued through inline asm ON PURPOSE: the
// compiler treats the builtin form as an LDS write it cannot disambiguate and puts
// `s_waitcnt vmcnt(0)` in front of every later LDS read -- which also waits for the NEXT
// stage's DMA and the column prefetch, i.e. exposes their full latency once per chunk.
// Hidden from its bookkeeping, the ordering is ours: the explicit counted vmcnt wait at the
// top of each stage (VMEM returns in order).  Hidden VMEM ops can only make the compiler's
// own counted waits stricter, never laxer, and the issue points below keep every hidden op
// OLDER than the column loads in flight, so they stay exact.
__device__ __forceinline__ void skl_dma16(const void *src, uint32_t lds_byte_addr)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
                 :
                 : "v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_byte_addr))
                 : "memory");   // m0 is reserved (cannot be listed); nothing else in these kernels uses it
#else
    (void)src;
    (void)lds_byte_addr;
#endif
}

// The same with the address split into a wave-uniform base (SGPR pair) and a 32-bit per-lane byte offset:
// the lane offsets of a wave's row pieces never change, so they are computed once (one register per DMA
// instruction) and a stage only supplies the base.
__device__ __forceinline__ void skl_dma16_saddr(const void *uniform_base, uint32_t lane_byte_offset, uint32_t lds_byte_addr)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t b = (uint64_t)uniform_base;
    // (the builtin returns int: widen as unsigned, or a low half with bit 31 set smears into the high one)
    const uint64_t sb = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32)) << 32) |
                        (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                 :
                 : "v"(lane_byte_offset), "s"(sb), "s"(__builtin_amdgcn_readfirstlane(lds_byte_addr))
                 : "memory");
#else
    (void)uniform_base;
    (void)lane_byte_offset;
    (void)lds_byte_addr;
#endif
}

// One stage of pair_kernel_kslice's row staging, for pair_kslice_walk.inc: the rows of this wave's CH chunks of flat stage T
// go into its row buffer BUF; piece p = (chunk * R + row) * 7 + q of the stage lands at slot p of the buffer.  A MACRO over
// the walk's names (g, a0, kk0, c_begin, stages_per_k, the strides, wave, lane, lds_base, dma_lane_off), not a function:
// as a __forceinline__ function template with those as parameters, hipcc computes the addresses differently inside the
// walk's hot blocks of every form (profiles/kslice_split.md).
// dma_lane_off (all forms but the A/B build's ABL & 4): the per-lane part of the source address -- which row, which of the
// stage's CH chunks, which plane pair -- is the same in every stage; it is kept as PPL 32-bit byte offsets and a stage
// supplies a scalar base.  A chunk past the end of the sketch -- sketch sizes that are not a multiple of 4 CH chunks -- is
// clamped to the last one (with lane offsets: reads the next k-mer length's or the next sample's words instead, inside the
// slab thanks to its A_PAD_ROWS zero rows) and never used.
#define SKL_STAGE_DMA(T, BUF)                                                                \
    do {                                                                                     \
        const uint32_t k_ = g.k_begin + kk0 + (BIG ? 0u : (T) / stages_per_k);               \
        const uint32_t c0_ = c_begin + (BIG ? (T) : (T) % stages_per_k) * (W * CH) + wave * CH; \
        if constexpr ((ABL & 4) == 0) {                                                      \
            const uint32_t cu_ = c0_ < g.ss64 ? c0_ : (g.ss64 - 1u);                         \
            const uint64_t *base_ = g.A + (size_t)a0 * sample_stride + (size_t)k_ * kmer_stride + (size_t)cu_ * BBITS; \
            _Pragma("unroll") for (int u = 0; u < PPL; ++u)                                  \
                skl_dma16_saddr(base_, dma_lane_off[u], lds_base + (((uint32_t)wave * 2u + (BUF)) * (PPL * LANES) + u * 64u) * 16u); \
        } else                                                                               \
        _Pragma("unroll") for (int u = 0; u < PPL; ++u)                                      \
        {   /* timing only: a tile-major row slab */                                         \
            const uint32_t pp_ = lane + u * 64u;                                             \
            const uint32_t p_ = pp_ < (uint32_t)PIECES ? pp_ : pp_ - (uint32_t)PIECES;       \
            const uint32_t q_ = p_ % 7u, rc_ = p_ / 7u;                                      \
            const uint32_t r_ = rc_ % R, c_ = rc_ / R;                                       \
            const uint32_t cc_ = (c0_ + c_) < g.ss64 ? (c0_ + c_) : (g.ss64 - 1u);           \
            skl_dma16(g.A + ((((size_t)(a0 / R) * g.nk + k_) * g.ss64 + cc_) * R + r_) * BBITS + 2u * q_, \
                      lds_base + (((uint32_t)wave * 2u + (BUF)) * (PPL * LANES) + u * 64u) * 16u); \
        }                                                                                    \
    } while (0)

__device__ __forceinline__ uint32_t skl_lds_addr(const void *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)p;
#else
    (void)p;
    return 0;
#endif
}

// jaccard.rs:14,26-44 on the device (used when a completeness correction makes the
// host-built tables inapplicable).
__device__ __forceinline__ double jaccard_from_samebits_dev(uint32_t samebits, uint32_t ss64,
                                                            bool has_c, double c1, double c2,
                                                            double cutoff)
{
    const double unionsize = (double)(64u * ss64);
    const uint32_t maxnbits = ss64 * 64u;
    const uint32_t expected = maxnbits >> BBITS;
    const uint32_t diff = samebits > expected ? samebits - expected : 0u;
    const double intersize = ((double)diff * (double)maxnbits) / (double)(maxnbits - expected);
    double j = intersize / unionsize;
    if (has_c) {
        if (c1 * c2 >= cutoff) {
            j = j / (c1 * c2 / (c1 + c2 - c1 * c2));  // jaccard.rs:55-57
            j = fmin(j, 1.0);
        }
    }
    return j;
}

// jaccard.rs:49-51; ln = the host libm's, restated (glibc_log.hpp)
__device__ __forceinline__ double ani_pois_dev(double j, double k, int log_variant)
{
    return fmax(0.0, 1.0 + 1.0 / k * glibc_log((2.0 * j) / (1.0 + j), log_variant));
}

// jaccard.rs:105-142, operation for operation.
__device__ __forceinline__ float2 simple_linear_regression_dev(double xsum, double ysum,
                                                               double xysum, double xsquaresum,
                                                               double ysquaresum, double n)
{
    if (isnan(ysum) || ysum == -INFINITY || n < 3.0) {
        return make_float2(1.0f, 1.0f);
    }
    const double xbar = xsum / n;
    const double ybar = ysum / n;
    const double x_diff = xsquaresum - xsum * xsum / n;
    const double y_diff = ysquaresum - ysum * ysum / n;
    const double xstddev = sqrt((xsquaresum - xsum * xsum / n) / n);
    const double ystddev = sqrt((ysquaresum - ysum * ysum / n) / n);
    const double r = (xysum - xsum * ysum / n) / sqrt(x_diff * y_diff);
    const double beta = r * ystddev / xstddev;
    const double alpha = -beta * xbar + ybar;
    double core = 0.0, acc = 0.0;
    if (beta < 0.0) {
        core = 1.0 - exp(beta);
    } else if (r > 0.0) {
        core = 1.0;
    }
    if (alpha < 0.0) {
        acc = 1.0 - exp(alpha);
    }
    return make_float2((float)core, (float)acc);
}

// distance_matrix.rs:11-14
__device__ __forceinline__ uint64_t square_to_condensed_dev(uint64_t i, uint64_t j, uint64_t n)
{
    return n * i - ((i * (i + 1)) >> 1) + j - 1 - i;
}


// f32 -> u32 whose unsigned order is the float order (the running top-k keeps its keys this way)
__device__ __forceinline__ uint32_t sortable_bits(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// This workgroup's tile (work_map.hpp): blockIdx % (number of XCDs) labels the XCD (MI355X_MICROARCH.md; 8 on an
// unpartitioned MI355X, PairArgs::xcd_shift), blockIdx / that number is its slot there.  False: it has none.
__device__ __forceinline__ bool lookup_tile(const PairArgs &g, uint32_t &group, uint32_t &row_tile)
{
    return lookup_tile_at(g, blockIdx.x & ((1u << g.xcd_shift) - 1u), blockIdx.x >> g.xcd_shift, group, row_tile);
}

__device__ __forceinline__ bool pair_valid(const PairArgs &g, uint32_t i, uint32_t jcol)
{
    return i < g.row_end && jcol < g.nB && (!g.self_mode || i < jcol);
}

__device__ __forceinline__ uint64_t pair_out_index(const PairArgs &g, uint32_t i, uint32_t jcol)
{
    return (g.self_mode ? square_to_condensed_dev(i, jcol, g.nB) : (uint64_t)i * g.nB + jcol) -
           g.out_base;
}

// MODE_COUNTS: samebits of k index kk (jaccard.rs:15-25) over `bins` bins (the whole sketch, or one
// chunk slice of it: pair_kslice.hip, k_slices)
// (U16_OK: the forms whose launches may park u16 records -- PairArgs::cnt_u16 -- carry the run-time choice)
template <bool U16_OK = false>
__device__ __forceinline__ void store_count(const PairArgs &g, uint32_t i, uint32_t jcol,
                                            uint32_t kk, uint32_t bins, uint32_t mismatches)
{
    if (pair_valid(g, i, jcol)) {
        const uint64_t at = pair_out_index(g, i, jcol) * g.cnt_pair_stride + kk * g.cnt_k_stride;
        if (U16_OK && g.cnt_u16) ((uint16_t *)g.out)[at] = (uint16_t)(bins - mismatches);
        else ((uint32_t *)g.out)[at] = bins - mismatches;
    }
}

// The same store write-through at agent scope (global_store_dword ... sc1): the counts a fused epilogue reads back from
// another workgroup (pair_kslice.hip, FUSE)
__device__ __forceinline__ void store_count_agent(const PairArgs &g, uint32_t i, uint32_t jcol,
                                                  uint32_t kk, uint32_t bins, uint32_t mismatches)
{
    if (pair_valid(g, i, jcol)) {
        __hip_atomic_store(&((uint32_t *)g.out)[pair_out_index(g, i, jcol) * g.cnt_pair_stride + kk * g.cnt_k_stride],
                           bins - mismatches, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// MODE_JACCARD: mod.rs:83-100 (dense) / :173-176 (kNN key)
__device__ __forceinline__ float jaccard_out_value(const PairArgs &g, uint32_t i, uint32_t jcol,
                                                   uint32_t mismatches)
{
    const uint32_t same = g.ss64 * 64u - mismatches;
    if (!g.has_comp) return g.dtab[same];
    const double jac =
        jaccard_from_samebits_dev(same, g.ss64, true, g.compA[i], g.compB[jcol], g.cutoff);
    if (g.jout == JOUT_DIST) return (float)(1.0 - jac);
    if (g.jout == JOUT_ANI) return (float)ani_pois_dev(jac, g.kf[0], g.log_variant);
    return (float)(1.0 - ani_pois_dev(jac, g.kf[0], g.log_variant));
}

__device__ __forceinline__ void store_jaccard(const PairArgs &g, uint32_t i, uint32_t jcol,
                                              uint32_t mismatches)
{
    if (!pair_valid(g, i, jcol)) return;
    ((float *)g.out)[pair_out_index(g, i, jcol)] = jaccard_out_value(g, i, jcol, mismatches);
}

// MODE_COREACC: core_acc_dist + simple_linear_regression (jaccard.rs:61-142) from the
// packed per-k mismatch counts (u16 fields, newest k lowest, s2:s1:s0).
__device__ __forceinline__ float2 coreacc_value(const PairArgs &g, uint32_t i, uint32_t jcol,
                                                uint32_t s0, uint32_t s1, uint32_t s2)
{
    const uint32_t maxnbits = g.ss64 * 64u;
    double xsum = 0.0, ysum = 0.0, xysum = 0.0, xsquaresum = 0.0, ysquaresum = 0.0, n = 0.0;
    double c1 = 0.0, c2 = 0.0;
    if (g.has_comp) {
        c1 = g.compA[i];
        c2 = g.compB[jcol];
    }
    bool alive = true;
    for (uint32_t t = 0; t < g.k_count; ++t) {
        const uint32_t f = g.k_count - 1u - t;  // field holding k index t
        const uint32_t word = (f >> 1) == 0u ? s0 : ((f >> 1) == 1u ? s1 : s2);
        const uint32_t same = maxnbits - ((word >> ((f & 1u) * 16u)) & 0xFFFFu);
        double y;
        if (!g.has_comp) {
            y = g.ytab[same];
        } else {
            y = glibc_log(jaccard_from_samebits_dev(same, g.ss64, true, c1, c2, g.cutoff), g.log_variant);
        }
        if (alive) {
            if (y < g.tolerance) {
                alive = false;  // jaccard.rs:89-91: break
            } else {
                const double k_fl = g.kf[t];
                xsum += k_fl;
                ysum += y;
                xysum += k_fl * y;
                xsquaresum += k_fl * k_fl;
                ysquaresum += y * y;
                n += 1.0;
            }
        }
    }
    return simple_linear_regression_dev(xsum, ysum, xysum, xsquaresum, ysquaresum, n);
}

// ... the same from the bin-match counts themselves, same[t] = samebits of k index t (the fused epilogue of a k-sliced
// counts launch, the pair-list kernels): core_acc_dist + simple_linear_regression, jaccard.rs:61-142, operation for operation
// as above.  The ONE loop every caller with counts runs, so that one place has to stay bit-identical: kf = the k-mer lengths
// as f64 (the kernel arguments' copy or a device array); UNROLL > 0: at most UNROLL lengths, the loop unrolled so that counts
// kept in registers are indexed statically; UNROLL = 0: any number of lengths, counts and lengths in memory.
template <int UNROLL>
__device__ __forceinline__ float2 coreacc_fit_counts(const PairArgs &g, uint32_t i, uint32_t jcol, const uint32_t *same_k, const double *kf)
{
    const uint32_t maxnbits = g.ss64 * 64u;
    double xsum = 0.0, ysum = 0.0, xysum = 0.0, xsquaresum = 0.0, ysquaresum = 0.0, n = 0.0;
    double c1 = 0.0, c2 = 0.0;
    if (g.has_comp) {
        c1 = g.compA[i];
        c2 = g.compB[jcol];
    }
    bool alive = true;
    auto one_length = [&](uint32_t t) {
        const uint32_t same = same_k[t] <= maxnbits ? same_k[t] : maxnbits;
        double y;
        if (!g.has_comp) {
            y = g.ytab[same];
        } else {
            y = glibc_log(jaccard_from_samebits_dev(same, g.ss64, true, c1, c2, g.cutoff), g.log_variant);
        }
        if (alive) {
            if (y < g.tolerance) {
                alive = false;  // jaccard.rs:89-91: break
            } else {
                const double k_fl = kf[t];
                xsum += k_fl;
                ysum += y;
                xysum += k_fl * y;
                xsquaresum += k_fl * k_fl;
                ysquaresum += y * y;
                n += 1.0;
            }
        }
    };
    if constexpr (UNROLL > 0) {
#pragma unroll
        for (uint32_t t = 0; t < (uint32_t)UNROLL; ++t) {
            if (t < g.k_count) one_length(t);
        }
    } else {
        for (uint32_t t = 0; t < g.k_count && alive; ++t) one_length(t);
    }
    return simple_linear_regression_dev(xsum, ysum, xysum, xsquaresum, ysquaresum, n);
}

__device__ __forceinline__ float2 coreacc_value_counts(const PairArgs &g, uint32_t i, uint32_t jcol, const uint32_t *same_k)
{
    return coreacc_fit_counts<MAX_FUSED_K>(g, i, jcol, same_k, g.kf);
}

__device__ __forceinline__ void store_coreacc(const PairArgs &g, uint32_t i, uint32_t jcol,
                                              uint32_t s0, uint32_t s1, uint32_t s2)
{
    if (!pair_valid(g, i, jcol)) return;
    ((float2 *)g.out)[pair_out_index(g, i, jcol)] = coreacc_value(g, i, jcol, s0, s1, s2);
}

// THE HALF-CHUNK COUNT: a wave reads a (sample, k) slice as ONE contiguous run, lane l the l-th half chunk of a trip (7 planes,
// 56 bytes; a trip is 3 584 bytes -- the form pair_cand.hip measured at 0.88 of the HBM peak), and the two halves of a chunk
// meet between neighbouring lanes.  Three steps, the loads left to the caller (who clamps the address, branches around the
// load or requests a trip ahead -- that order is what was measured):
//   half_chunk_fold   the mismatch words of this lane's seven planes, a against b;
//   half_chunk_share  the other seven planes of the chunk sit in lane l ^ 1: a bin matches iff all 14 agree.  Returns the
//                     MISMATCHES of the chunk in its even lane, 0 in the odd one and where the half chunk is not `counted`
//                     (a lane past the slice's end);
//   wave_sum          the 64 shares summed: four row shifts leave each row of 16 lanes' total in its last lane, four
//                     v_readlane add them up (wave-uniform result).
__device__ __forceinline__ void half_chunk_fold(const uint2 *a, const uint2 *b, uint32_t &mlo, uint32_t &mhi)
{
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        mlo = acc_mismatch<true>(mlo, a[q].x, b[q].x);
        mhi = acc_mismatch<true>(mhi, a[q].y, b[q].y);
    }
}

__device__ __forceinline__ uint32_t half_chunk_share(uint32_t mlo, uint32_t mhi, uint32_t lane, bool counted)
{
    mlo |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mlo, 0xB1, 0xF, 0xF, true);   // quad_perm [1, 0, 3, 2]
    mhi |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mhi, 0xB1, 0xF, 0xF, true);
    return ((lane & 1u) == 0u && counted) ? (uint32_t)__builtin_popcount(mlo) + (uint32_t)__builtin_popcount(mhi) : 0u;
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v)
{
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t part)
{
    part = dpp_add<0x111>(part);   // row_shr:1
    part = dpp_add<0x112>(part);   // row_shr:2
    part = dpp_add<0x114>(part);   // row_shr:4
    part = dpp_add<0x118>(part);   // row_shr:8
    return (uint32_t)__builtin_amdgcn_readlane((int)part, 15) + (uint32_t)__builtin_amdgcn_readlane((int)part, 31) +
           (uint32_t)__builtin_amdgcn_readlane((int)part, 47) + (uint32_t)__builtin_amdgcn_readlane((int)part, 63);
}

}  // namespace skl
