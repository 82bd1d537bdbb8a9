// sketch_finish.hip -- the second half of GPU sketching on the device: densify_bin and the 14-plane transpose
// of fill_usigs over the bin minima the sketch kernels left in memory, a workgroup per (sample, k) stream.  What a stream
// sends home is num_bins / 64 * 14 words, its first sign and a flag byte instead of num_bins u64 signs.
//
// densify_bin is a sequential loop; finish_plan.hpp restates it as a per-bin TARGET (the first probe that lands below the bin
// or on a bin that was never empty) followed by a RESOLVE along the targets to an originally non-empty bin.  The kernel runs
// step 1 a bin per lane, resolves by pointer jumping on the target INDICES (so the 64-bit first sign survives), and transposes
// with one __ballot per plane: with lane l holding bin 64 c + l, __ballot((v >> p) & 1) is word c * 14 + p.
//
// The same two steps also end in a u16 row instead of the planes (U16): exactly num_bins bins for ANY num_bins, `sign as u16`
// per bin -- the `.skq` row of an inverted index (inverted.rs:352-380).  Steps 1 and 2 are shared; only the chunk count of the
// "holds a value" ballot (ceil(n / 64), the lanes past n masked out of it) and the emit differ, at compile time.
//
// Two placements of one body: the targets (a u32 per bin) and one emptiness bit per bin in LDS up to FINISH_LDS_BINS_MAX bins; above
// it the targets in a global scratch array per workgroup, emptiness read from the signs, and the workgroups walk the streams.
//
// Every loop is bounded by a constant or by num_bins: a stream of empty bins only is flagged and never probed (the sequential
// loop would not end on it), a bin's probes stop at the cap (the stream is flagged FINISH_UNFINISHED and left to the host), and
// the pointer jumping runs at most FINISH_MAX_ROUNDS rounds.
#include "kernels.h"

namespace skl {

namespace {
// OR of `bits` over the workgroup, through one LDS word.  Every thread calls it; the barriers also order the targets.
__device__ __forceinline__ uint32_t wg_or(uint32_t bits, uint32_t *slot)
{
    __syncthreads();   // (the slot's previous reader is done)
    if (threadIdx.x == 0) *slot = 0;
    __syncthreads();
    if (bits) atomicOr(slot, bits);
    __syncthreads();
    return *slot;
}

// the targets are read and written by other lanes between barriers while the pointers jump: single 32-bit accesses, never cached in a register
__device__ __forceinline__ uint32_t tgt_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void tgt_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

template <bool LDS, bool U16>
__global__ __launch_bounds__(LDS ? FINISH_WG_LDS : FINISH_WG_GLOBAL) void sketch_finish_kernel(const FinishArgs g)
{
    extern __shared__ uint32_t lds[];             // LDS form: targets [num_bins], then the "holds a value" bits [ceil(num_bins / 32)]
    __shared__ uint32_t s_vote;
    __shared__ unsigned long long s_capped;       // 1 + the stream one of whose bins has run into the probe cap
    const uint32_t tid = threadIdx.x, n_threads = blockDim.x, lane = tid & 63u, wave = tid >> 6, n_waves = n_threads >> 6;
    // (blockDim.x is whole waves in either form -- finish_threads / finish_threads_u16 -- so n_waves >= 1 and the chunk loops advance)
    const uint32_t n = g.num_bins, chunks = U16 ? (uint32_t)(((uint64_t)n + 63u) >> 6) : n >> 6;
    const uint64_t words = (uint64_t)chunks * FINISH_PLANES;
    uint32_t *tgt;
    if constexpr (LDS) tgt = lds; else tgt = g.targets + (uint64_t)blockIdx.x * n;
    uint32_t *filled_bits = lds + n;
    if (tid == 0) s_capped = 0;                   // (the first vote's barriers come before its first reader)

    for (uint64_t st = blockIdx.x; st < g.n_streams; st += gridDim.x) {
        const uint64_t *orig = g.signs + st * n;
        uint64_t *out = U16 ? nullptr : g.usigs + st * words;       // (plane form)
        uint16_t *out16 = U16 ? g.bins_u16 + st * n : nullptr;      // (u16 form: the row starts 2 n st bytes in, 2-byte aligned only)

        // which bins hold a value
        uint32_t seen = 0;                        // 1: a bin with a value, 2: an empty bin
        for (uint32_t c = wave; c < chunks; c += n_waves) {
            unsigned long long m, all = ~0ull;
            if constexpr (U16) {                  // ragged tail: a lane past n reads nothing and votes neither way
                const uint32_t i = 64u * c + lane, left = n - 64u * c;   // left >= 1
                bool holds = false;
                if (lane < left) holds = orig[i] != FINISH_EMPTY;
                if (left < 64u) all = (1ull << left) - 1ull;
                m = __ballot(holds);
            } else {
                m = __ballot(orig[64u * c + lane] != FINISH_EMPTY);
            }
            seen |= (m != 0 ? 1u : 0u) | (m != all ? 2u : 0u);
            if (LDS && lane == 0) {
                filled_bits[2 * c] = (uint32_t)m;
                if (!U16 || 64u * c + 32u < n) filled_bits[2 * c + 1] = (uint32_t)(m >> 32);   // (the bits end at ceil(n / 32) words)
            }
        }
        const uint32_t have = wg_or(seen, &s_vote);
        if (!(have & 1u)) {                       // nothing to fill from: zeroed words and the flag, no probe at all
            if constexpr (U16) {
                for (uint64_t i = tid; i < n; i += n_threads) out16[i] = 0;
            } else {
                for (uint64_t w = tid; w < words; w += n_threads) out[w] = 0;
            }
            if (tid == 0) {
                if constexpr (!U16) g.first_sign[st] = FINISH_EMPTY;
                g.flags[st] = FINISH_ALL_EMPTY;
            }
            continue;
        }
        const bool densify = (have & 2u) != 0;
        if (densify) {
            // step 1: targets
            for (uint64_t i64 = tid; i64 < n; i64 += n_threads) {   // (64-bit: i + n_threads may pass 2^32)
                const uint32_t i = (uint32_t)i64;
                if (*(volatile unsigned long long *)&s_capped == st + 1) break;   // the stream goes to the host anyway
                auto is_filled = [&](uint32_t j) -> bool {
                    if constexpr (LDS) return (filled_bits[j >> 5] >> (j & 31u)) & 1u;
                    else return orig[j] != FINISH_EMPTY;
                };
                uint32_t t = i;
                if (!is_filled(i)) {
                    t = finish_target(i, n, g.max_attempts, is_filled);
                    if (t == i) *(volatile unsigned long long *)&s_capped = st + 1;
                }
                tgt_store(tgt + i, t);
            }
            __syncthreads();
            if (s_capped == st + 1) {
                if (tid == 0) g.flags[st] = FINISH_DENSIFIED | FINISH_UNFINISHED;
                continue;
            }
            // step 2: pointer jumping, in place -- whatever a lane reads is an ancestor of its bin, and the root is unique
            uint32_t round = 0;
            for (; round < FINISH_MAX_ROUNDS; ++round) {
                uint32_t changed = 0;
                for (uint64_t i64 = tid; i64 < n; i64 += n_threads) {
                    const uint32_t i = (uint32_t)i64;
                    const uint32_t t = tgt_load(tgt + i), tt = tgt_load(tgt + t);
                    if (tt != t) {
                        tgt_store(tgt + i, tt);
                        changed = 1;
                    }
                }
                if (!wg_or(changed, &s_vote)) break;
            }
            if (round == FINISH_MAX_ROUNDS) {     // (cannot happen: 33 rounds resolve any chain)
                if (tid == 0) g.flags[st] = FINISH_DENSIFIED | FINISH_UNFINISHED;
                continue;
            }
        }
        if constexpr (U16) {
            // emit: a lane per bin, `sign as u16` of the root's sign, coalesced 2-byte stores (a row is only 2-byte aligned)
            for (uint64_t i64 = tid; i64 < n; i64 += n_threads) {
                const uint32_t i = (uint32_t)i64;
                out16[i] = (uint16_t)orig[densify ? tgt_load(tgt + i) : i];
            }
        } else {
            // transpose: word c * 14 + p = bit p of bins 64 c .. 64 c + 63
            for (uint32_t c = wave; c < chunks; c += n_waves) {
                const uint32_t i = 64u * c + lane;
                const uint64_t v = orig[densify ? tgt_load(tgt + i) : i];
                unsigned long long mine = 0;
#pragma unroll
                for (uint32_t p = 0; p < FINISH_PLANES; ++p) {
                    const unsigned long long w = __ballot((v >> p) & 1ull);
                    if (lane == p) mine = w;
                }
                if (lane < FINISH_PLANES) out[(uint64_t)c * FINISH_PLANES + lane] = mine;
                if (i == 0) g.first_sign[st] = v;
            }
        }
        if (tid == 0) g.flags[st] = densify ? FINISH_DENSIFIED : 0;
    }
}
}  // namespace

hipError_t launch_sketch_finish(const FinishArgs &args, hipStream_t stream)
{
    if (args.n_streams == 0) return hipSuccess;
    const uint64_t blocks = finish_workgroups(args.n_streams, args.num_bins);
    if (blocks > 0x7FFFFFFFull || args.num_bins % 64 != 0 || args.num_bins == 0) return hipErrorInvalidValue;
    const uint32_t threads = finish_threads(args.num_bins);
    if (finish_lds_form(args.num_bins)) {
        hipLaunchKernelGGL((sketch_finish_kernel<true, false>), dim3((unsigned)blocks), dim3(threads), (size_t)finish_lds_bytes(args.num_bins), stream, args);
    } else {
        if (!args.targets) return hipErrorInvalidValue;
        hipLaunchKernelGGL((sketch_finish_kernel<false, false>), dim3((unsigned)blocks), dim3(threads), 0, stream, args);
    }
    return hipGetLastError();
}

// The u16 form: any num_bins >= 1, whole-wave workgroups, the row in args.bins_u16 (usigs / first_sign unused).
hipError_t launch_sketch_finish_u16(const FinishArgs &args, hipStream_t stream)
{
    if (args.n_streams == 0) return hipSuccess;
    if (args.num_bins == 0 || !args.bins_u16) return hipErrorInvalidValue;
    const uint64_t blocks = finish_workgroups(args.n_streams, args.num_bins);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint32_t threads = finish_threads_u16(args.num_bins);
    if (threads < 64 || threads % 64 != 0) return hipErrorInvalidValue;
    if (finish_lds_form(args.num_bins)) {
        hipLaunchKernelGGL((sketch_finish_kernel<true, true>), dim3((unsigned)blocks), dim3(threads), (size_t)finish_lds_bytes_u16(args.num_bins), stream, args);
    } else {
        if (!args.targets) return hipErrorInvalidValue;
        hipLaunchKernelGGL((sketch_finish_kernel<false, true>), dim3((unsigned)blocks), dim3(threads), 0, stream, args);
    }
    return hipGetLastError();
}

}  // namespace skl
