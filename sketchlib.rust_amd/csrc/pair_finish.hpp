// pair_finish.hpp -- what pair_kernel_kslice (pair_kslice.hip) does with a pair once its count is known, and the
// pruning test on counts that are not final yet: leaf helpers, scalar parameters only (hipcc's register allocation of
// that kernel does not survive wrappers around its live arrays; these it inlines without a trace).
#pragma once

#include "device_common.hpp"

namespace skl {

// Symmetric self kNN, row side: does the 64-column block jb bring row i anything below its knn-th best?  `valid` / `key`
// are this lane's pair of the block (the whole wave calls; i and jb are wave-uniform).
__device__ __forceinline__ void mark_row_block(const PairArgs &g, uint32_t i, uint32_t jb, bool valid, float key, uint32_t lane)
{
    if (g.r_bits != nullptr && i < g.row_end) {
        const uint32_t thr_ = g.r_thr[(size_t)(i - g.row_begin) * g.r_thr_stride];
        if (__ballot(valid && sortable_bits(key) < thr_) != 0ull && lane == 0u) {
            atomicOr(&g.r_bits[(size_t)(i - g.row_begin) * g.r_bits_stride + (jb >> 5)], 1u << (jb & 31u));
        }
    }
}

// ... column side: does `best`, the best key of some rows of the band from row offset row_off on (inside one 32-row
// stretch; invalid records are +inf), beat turned column jc's knn-th best?  Then the column is flagged, and the stretch
// marked.  True if it does.  For launches that keep flags (g.t_flag) only.
__device__ __forceinline__ bool mark_turned(const PairArgs &g, uint32_t jc, uint32_t row_off, float best)
{
    if (sortable_bits(best) < g.t_thr[(size_t)jc * g.t_thr_stride]) {
        g.t_flag[jc] = g.t_flag_value;
        if (g.t_bits != nullptr) {
            const uint32_t tb = row_off >> 5;
            atomicOr(&g.t_bits[(size_t)jc * g.t_bits_stride + (tb >> 5)], 1u << (tb & 31u));
        }
        return true;
    }
    return false;
}

__device__ __forceinline__ float record_key(float v) { return v; }
__device__ __forceinline__ float record_key(float2 v) { return v.x; }   // (core, acc): the key is the core distance

// Finish one key of a kNN band -- pair (i, column `lane` of block jb): valid -> value -> store -> row mark.  Returns the
// record (+inf where there is no pair), for the turned copy.  Rec = float: s0 = the mismatch count of the one k-mer
// length; float2: s2:s1:s0 = the packed counts coreacc_value() takes.  COMP = false: a launch known to have no completeness
// correction (the pruning launches), the value is the table's.
template <typename Rec, bool COMP = true>
__device__ __forceinline__ Rec finish_key(const PairArgs &g, uint32_t i, uint32_t jb, uint32_t lane, uint32_t s0, uint32_t s1 = 0u, uint32_t s2 = 0u)
{
    const uint32_t jc = jb * 64u + lane;
    Rec v;
    if constexpr (sizeof(Rec) == sizeof(float)) v = __builtin_inff();
    else v = make_float2(__builtin_inff(), __builtin_inff());
    const bool valid = pair_valid(g, i, jc);
    if (valid) {
        if constexpr (sizeof(Rec) == sizeof(float) && !COMP) v = g.dtab[g.ss64 * 64u - s0];
        else if constexpr (sizeof(Rec) == sizeof(float)) v = jaccard_out_value(g, i, jc, s0);
        else v = coreacc_value(g, i, jc, s0, s1, s2);
        ((Rec *)g.out)[pair_out_index(g, i, jc)] = v;
    }
    mark_row_block(g, i, jb, valid, record_key(v), lane);
    return v;
}

// The turned copy of a tile (symmetric self kNN: the keys of columns >= t_col_begin are also candidates of the ROW with
// that sample id).  The tile is turned through LDS -- record (column c, row r) at tt[c * turned_pitch(R) + r] -- so that
// a column's R records leave as 16-byte stores (float: one 64-byte run per column at R = 16), each with its mark.
__host__ __device__ constexpr uint32_t turned_pitch(int rows) { return (uint32_t)rows + 4u; }   // padded, keeps 16-byte alignment

template <typename Rec, int R, int JL>
__device__ __forceinline__ void store_turned_tile(const PairArgs &g, const Rec *tt, uint32_t jb0, uint32_t a0, uint32_t tid)
{
    constexpr uint32_t PER = 16u / sizeof(Rec), RUNS = (uint32_t)R / PER;   // records per store, stores per column
    for (uint32_t item = tid; item < (uint32_t)JL * 64u * RUNS; item += LANES * WAVES_PER_WG) {
        const uint32_t c = item / RUNS, q = item % RUNS;
        const uint32_t jc = jb0 * 64u + c;
        if (jc >= g.t_col_begin && jc < g.nB) {
            const float4 v = *reinterpret_cast<const float4 *>(&tt[c * turned_pitch(R) + PER * q]);
            *reinterpret_cast<float4 *>(reinterpret_cast<Rec *>(g.out_t) + (size_t)(jc - g.t_col_begin) * g.t_stride + (a0 - g.row_begin) + PER * q) = v;
            if (g.t_flag != nullptr) mark_turned(g, jc, a0 - g.row_begin + PER * q, PER == 4u ? fminf(fminf(v.x, v.y), fminf(v.z, v.w)) : fminf(v.x, v.z));
        }
    }
}

}  // namespace skl
