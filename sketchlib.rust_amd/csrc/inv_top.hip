// inv_top.hip -- the best hits of an inverted query, selected on the GPU (gfx950) behind inv_query_kernel's counts: for every
// query the `top` indexed samples with the largest key (count << 32) | index (the reference's identification query,
// src/lib.rs:1019-1109: counts -> d / (2 S - d), stable ascending sort, reverse, first nouts).  Match-count mode copies
// n u32 per query to the host; this copies `top` ids and counts.
//
// One workgroup of 256 threads per query, the three steps of inv_top_plan.hpp (which the kernel takes every number from and
// whose inv_top_select_host() restates it for the CPU test): exact, deterministic, no global atomics, no floating point.
//   1. threshold: `digits` passes over the row, 16-byte loads where the row's alignment allows (n is any number, so a row
//      starts on a 4-byte boundary: up to 3 leading and 3 trailing entries are read singly), a histogram of the current digit
//      in LDS.  Unrelated samples put nearly every lane on one bin (count 0 or 1): a wave whose active lanes all hold the first
//      active lane's digit adds its lane count once instead of 64 atomics on one address.
//   2. collect: the row again from the high end in chunks of 256 until the list is full -- with many ties at the threshold (the
//      usual case: t = 0 or 1) after a few chunks, but a query whose only good hit sits at a low index walks the whole row.
//      Ballots give the rank inside a wave, LDS the offsets between waves.  INV_TOP_WALK_BATCH chunks go together: their loads
//      are in flight at once and their per-wave totals cross one barrier (a chunk a barrier left the walk of a million
//      entries at 3 ms, each trip waiting for its own load); behind the barrier the chunks are taken one by one as the host does.
//   3. bitonic sort of at most 1 024 keys in LDS, then the ids and counts.
#include "kernels.h"

namespace skl {

namespace {

__device__ __forceinline__ uint32_t lanes_below(uint64_t m)   // set bits of m below this lane
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// one entry per lane into the histogram; every lane of the wave calls it (ballots), `digit` is 0 where !act
__device__ __forceinline__ void hist_add(uint32_t *hist, bool act, uint32_t digit)
{
    const uint64_t m = __ballot(act);
    if (m == 0) return;
    const int first = __ffsll((unsigned long long)m) - 1;
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)digit, first);   // (first comes from the ballot: wave-uniform)
    if (__ballot(act && digit == d0) == m) {
        if ((int)(threadIdx.x & 63u) == first) atomicAdd(&hist[d0], (uint32_t)__popcll(m));
    } else if (act) {
        atomicAdd(&hist[digit], 1u);
    }
}

// exclusive prefix of v over the workgroup's threads (ws: 4 u32 of LDS, free again after the next barrier)
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t *ws)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t below = __shfl_up(inc, o);
        if (lane >= (uint32_t)o) inc += below;
    }
    if (lane == 63u) ws[wave] = inc;
    __syncthreads();
    uint32_t off = 0;
    for (uint32_t k = 0; k < wave; ++k) off += ws[k];
    return off + inc - v;
}

}  // namespace

__global__ __launch_bounds__(INV_TOP_THREADS) void inv_top_kernel(const InvTopArgs a)
{
    extern __shared__ uint64_t inv_top_lds[];
    uint64_t *keys = inv_top_lds;                               // [list_len]
    uint32_t *hist = (uint32_t *)(keys + a.list_len);           // [1 << digit_bits]
    uint32_t *walk_ws = hist + (1u << a.digit_bits);            // [2][INV_TOP_WALK_BATCH][2][4]: per-wave totals of a batch's chunks (above / equal), two batches in flight
    uint32_t *scan_ws = walk_ws + 2u * INV_TOP_WALK_BATCH * 8u; // [4]
    uint32_t *pass_res = scan_ws + 4;                           // [2]: the pass's bin, the entries above it

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t q = blockIdx.x, n = a.n, w = a.digit_bits, bins = 1u << w;
    const uint32_t *__restrict__ row = a.counts + (uint64_t)q * n;

    // ---- 1. threshold ----
    const uint32_t lead = min(n, (4u - (uint32_t)(((uint64_t)q * n) & 3u)) & 3u);   // entries before the first 16-byte boundary
    const uint32_t nvec = (n - lead) / 4u;
    const uint32_t tail0 = lead + nvec * 4u;                                        // [tail0, n): at most 3 entries
    const uint4 *__restrict__ body = reinterpret_cast<const uint4 *>(row + lead);
    uint32_t prefix = 0, need = a.n_eff, g = 0;
    for (uint32_t d = 0; d < a.digits; ++d) {
        const uint32_t shift = inv_top_shift(a.digits, d, w);
        for (uint32_t b = tid; b < bins; b += INV_TOP_THREADS) hist[b] = 0u;
        __syncthreads();
        auto add = [&](bool live, uint32_t c) {
            const bool act = live && inv_top_above(c, shift, w) == prefix;
            hist_add(hist, act, act ? inv_top_digit(c, shift, w) : 0u);
        };
        {   // the unaligned ends: lanes [0, lead) the head, the next n - tail0 lanes the tail
            const bool live = tid < lead + (n - tail0);
            const uint32_t at = tid < lead ? tid : tail0 + (tid - lead);
            add(live, live ? row[at] : 0u);
        }
        for (uint32_t v0 = 0; v0 < nvec; v0 += 2u * INV_TOP_THREADS) {   // two loads in flight per lane; the trip count is wave-uniform
            const uint32_t i0 = v0 + tid, i1 = i0 + INV_TOP_THREADS;
            const bool live0 = i0 < nvec, live1 = i1 < nvec;
            const uint4 c0 = body[live0 ? i0 : 0u];   // (unconditional, so that they stay 16-byte loads; entry 0 exists: nvec >= 1 here)
            const uint4 c1 = body[live1 ? i1 : 0u];
            add(live0, c0.x);
            add(live0, c0.y);
            add(live0, c0.z);
            add(live0, c0.w);
            add(live1, c1.x);
            add(live1, c1.y);
            add(live1, c1.z);
            add(live1, c1.w);
        }
        __syncthreads();
        // the histogram from the top bin down: thread i owns `per` bins ending at bins - 1 - i * per
        const uint32_t per = bins >= INV_TOP_THREADS ? bins / INV_TOP_THREADS : 1u;
        const bool owns = tid * per < bins;
        const uint32_t hi = bins - 1u - tid * per;
        uint32_t mine = 0;
        if (owns) {
            for (uint32_t j = 0; j < per; ++j) mine += hist[hi - j];
        }
        const uint32_t before = block_exclusive(mine, scan_ws);
        if (owns && before < need && need <= before + mine) {   // exactly one thread: the prefix's entries number at least `need`
            uint32_t above = before, bin = hi;
            while (above + hist[bin] < need) above += hist[bin--];
            pass_res[0] = bin;
            pass_res[1] = above;
        }
        __syncthreads();
        g += pass_res[1];
        need -= pass_res[1];
        prefix = (prefix << w) | pass_res[0];
    }
    const uint32_t t = prefix, e = need;   // n_eff-th largest count; g entries above it, e equal ones to take

    // ---- 2. collect from the high end ----
    for (uint32_t i = a.n_eff + tid; i < a.list_len; i += INV_TOP_THREADS) keys[i] = 0ull;
    uint32_t got_gt = 0, seen_eq = 0;
    const uint32_t chunks = inv_top_chunks(n);
    // (the loop's condition is workgroup-uniform: every thread sums the same totals.  Inside a batch nothing stops early: once
    // got_gt == g no entry above t is left, and an equal entry of rank e or more is not taken)
    for (uint32_t chunk0 = 0, batch = 0; chunk0 < chunks && (got_gt < g || seen_eq < e); chunk0 += INV_TOP_WALK_BATCH, ++batch) {
        uint32_t c[INV_TOP_WALK_BATCH], at[INV_TOP_WALK_BATCH];
        uint32_t live = 0;
#pragma unroll
        for (uint32_t b = 0; b < INV_TOP_WALK_BATCH; ++b) {
            at[b] = inv_top_walk_index(n, chunk0 + b, tid);
            if (inv_top_walk_live(n, chunk0 + b, tid)) live |= 1u << b;
            c[b] = (live >> b & 1u) ? row[at[b]] : 0u;
        }
        uint32_t *ws = walk_ws + (batch & 1u) * (INV_TOP_WALK_BATCH * 8u);   // the other half is still being read by slower waves
#pragma unroll
        for (uint32_t b = 0; b < INV_TOP_WALK_BATCH; ++b) {
            const bool lv = live >> b & 1u;
            const uint64_t bg = __ballot(lv && c[b] > t), be = __ballot(lv && c[b] == t);
            if (lane == 0u) {
                ws[b * 8u + wave] = (uint32_t)__popcll(bg);
                ws[b * 8u + 4u + wave] = (uint32_t)__popcll(be);
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t b = 0; b < INV_TOP_WALK_BATCH; ++b) {
            uint32_t off_g = 0, off_e = 0, tot_g = 0, tot_e = 0;
#pragma unroll
            for (uint32_t k = 0; k < INV_TOP_THREADS / 64u; ++k) {
                const uint32_t x = ws[b * 8u + k], y = ws[b * 8u + 4u + k];
                if (k < wave) {
                    off_g += x;
                    off_e += y;
                }
                tot_g += x;
                tot_e += y;
            }
            if ((tot_g | tot_e) != 0u) {   // (workgroup-uniform)
                const bool lv = live >> b & 1u;
                const bool gt = lv && c[b] > t, eq = lv && c[b] == t;
                const uint64_t bg = __ballot(gt), be = __ballot(eq);
                if (gt) {
                    keys[got_gt + off_g + lanes_below(bg)] = inv_top_key(c[b], at[b]);        // < g
                } else if (eq) {
                    const uint32_t rank = seen_eq + off_e + lanes_below(be);
                    if (rank < e) keys[g + rank] = inv_top_key(c[b], at[b]);                  // < g + e = n_eff
                }
            }
            got_gt += tot_g;
            seen_eq += tot_e;
        }
    }
    __syncthreads();

    // ---- 3. sort descending, store ----
    for (uint32_t k = 2; k <= a.list_len; k <<= 1) {
        for (uint32_t j = k >> 1; j; j >>= 1) {
            for (uint32_t i = tid; i < a.list_len; i += INV_TOP_THREADS) {
                const uint32_t x = i ^ j;
                if (x > i) {
                    const uint64_t u = keys[i], v = keys[x];
                    if ((i & k) == 0u ? u < v : u > v) {
                        keys[i] = v;
                        keys[x] = u;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t r = tid; r < a.top; r += INV_TOP_THREADS) {
        const bool hit = r < a.n_eff;
        const uint64_t key = hit ? keys[r] : 0ull;
        a.ids[(uint64_t)q * a.top + r] = hit ? (uint32_t)key : INV_TOP_PAD_ID;
        a.hit_counts[(uint64_t)q * a.top + r] = (uint32_t)(key >> 32);
    }
}

hipError_t launch_inv_top(const InvTopArgs &a, hipStream_t stream)
{
    if (a.nq == 0 || a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(inv_top_kernel, dim3(a.nq), dim3(INV_TOP_THREADS), inv_top_lds_bytes(a.n_eff, a.digit_bits), stream, a);
    return hipGetLastError();
}

}  // namespace skl
