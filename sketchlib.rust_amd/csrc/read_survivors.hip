// read_survivors.hip -- the GPU half of read sketching with a k-mer count filter.
//
// The reference offers a window's sign to its count filter only while the sign is below the current
// minimum of its bin (Sketch::bin_sign, src/sketch/mod.rs:198-210), and bins only ever fall.  So for
// any bin state the host has already reached -- the threshold table -- a window whose sign is at or
// above its bin's threshold is never offered and cannot change the result.  This kernel hashes every
// valid window in a range of window starts of every (sample, k) stream, exactly as
// nthash_binmin_kernel does, and appends the others -- the survivors -- as (window start, sign) to a
// per-stream buffer; the host sorts them by start and replays them through the filter.
//
// One thread = SPAN consecutive window starts of one sample; a sample's threads are padded to whole
// waves, so every wave works on one stream at a time and appends with one atomic per wave and window
// step (ballot, popcount, prefix rank).  The count always advances; records past `capacity` are not
// written, and the host repeats the call with room for them.  Vector stores only.
#include "kernels.h"
#include "nthash.hpp"   // srol, sror, the seeds, mod_sign

namespace skl {

constexpr int RS_SPAN = READ_SURVIVOR_SPAN;    // window starts per thread (sketch_plan.hpp)
constexpr int RS_WG = READ_SURVIVOR_WG;

__global__ __launch_bounds__(RS_WG) void read_survivors_kernel(const ReadSurvivorArgs g)
{
    const uint64_t t = (uint64_t)blockIdx.x * RS_WG + threadIdx.x;
    if (t >= g.n_spans) return;   // whole waves: n_spans is a multiple of 64
    uint32_t lo = 0, hi = g.n_samples;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (g.span_begin[mid] <= t) lo = mid; else hi = mid;
    }
    const uint32_t sample = lo;   // the same for every lane of the wave
    const uint64_t n_codes = g.code_begin[sample + 1] - g.code_begin[sample];
    const uint64_t *offs = g.offsets + g.offset_begin[sample];
    const uint32_t n_offs = (uint32_t)(g.offset_begin[sample + 1] - g.offset_begin[sample]);
    const uint32_t *pk = g.packed + g.word_begin[sample];
    auto code = [&](uint64_t x) -> uint32_t { return (pk[x >> 4] >> ((uint32_t)(x & 15u) * 2u)) & 3u; };
    const uint64_t p0 = g.win_begin[sample] + (t - g.span_begin[sample]) * RS_SPAN;
    const uint64_t p1 = p0 + RS_SPAN < g.win_end[sample] ? p0 + RS_SPAN : g.win_end[sample];   // p1 <= p0: a padding lane
    const uint32_t lane = __lane_id();
    const uint32_t last_bin = (uint32_t)(g.num_bins - 1u);
    // first break strictly after p0
    uint32_t oi0;
    {
        uint32_t a = 0, b = n_offs;
        while (a < b) {
            const uint32_t mid = (a + b) >> 1;
            if (offs[mid] > p0) b = mid; else a = mid + 1;
        }
        oi0 = a;
    }

    for (uint32_t ki = 0; ki < g.nk; ++ki) {
        const uint32_t k = g.kmers[ki];
        const uint64_t stream = (uint64_t)sample * g.nk + ki;
        const uint64_t *thr = g.thresholds + stream * g.num_bins;
        uint64_t top_f[4], top_r[4];
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b) {
            top_f[b] = g.top_f[ki * 4 + b];
            top_r[b] = g.top_r[ki * 4 + b];
        }
        // windows of this lane: starts p0 .. p0 + n_win - 1 (a start needs k codes of the sample)
        const uint64_t last_start_excl = n_codes >= k ? n_codes - k + 1u : 0u;
        const uint64_t end = p1 < last_start_excl ? p1 : last_start_excl;
        const uint32_t n_win = end > p0 ? (uint32_t)(end - p0) : 0u;
        uint64_t fh = 0, rh = 0;
        if (n_win != 0u) {   // seed at p0; the hashes then roll through breaks (codes holds every position)
            for (uint32_t i = 0; i < k; ++i) fh = srol(fh) ^ hash_fwd(code(p0 + i));
            if (g.rc) {
                for (uint32_t i = k; i-- > 0;) rh = srol(rh) ^ hash_rc(code(p0 + i));
            }
        }
        uint32_t oi = oi0;
        // uniform trip count: every lane of the wave reaches the ballot of every step
        for (uint32_t j = 0; j < (uint32_t)RS_SPAN; ++j) {
            const uint64_t s = p0 + j;
            const bool in = j < n_win;
            bool keep = false;
            uint64_t sign = 0;
            if (in) {
                if (j != 0u) {
                    const uint32_t old_b = code(s - 1), new_b = code(s + k - 1);
                    fh = srol(fh ^ top_f[old_b]) ^ hash_fwd(new_b);
                    if (g.rc) rh = sror(rh ^ hash_rc(old_b)) ^ top_r[new_b];
                }
                while (oi < n_offs && offs[oi] <= s) ++oi;
                const uint64_t next_off = oi < n_offs ? offs[oi] : n_codes;
                if (s + k <= next_off) {   // no break strictly inside the window (next_iterator, nthash_iterator.rs:325-346)
                    const uint64_t h = g.rc ? (fh < rh ? fh : rh) : fh;   // nthash_iterator.rs:62-68
                    sign = mod_sign(h);
                    // bin = sign / bin_size: nthash.hpp bin_of(sign, g.inv_bin_size, g.bin_size, last_bin), spelled out -- the call
                    // gives this kernel another block layout
                    uint32_t bin = (uint32_t)((double)sign * g.inv_bin_size);   // off by at most one; one product settles it
                    if (bin > last_bin) bin = last_bin;
                    const uint64_t prod = (uint64_t)bin * g.bin_size;
                    if (prod > sign) --bin;
                    else if (sign - prod >= g.bin_size && bin < last_bin) ++bin;
                    keep = sign < thr[bin];
                }
            }
            const unsigned long long mask = __ballot(keep);
            if (mask != 0ull) {
                const uint32_t leader = (uint32_t)__ffsll(mask) - 1u;
                unsigned long long base = 0ull;
                if (lane == leader) base = atomicAdd(&g.counts[stream], (unsigned long long)__popcll(mask));
                base = __shfl(base, (int)leader);
                if (keep) {
                    const uint64_t pos = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
                    if (pos < g.capacity) {
                        uint64_t *rec = g.survivors + (stream * g.capacity + pos) * 2u;
                        rec[0] = s;
                        rec[1] = sign;
                    }
                }
            }
        }
    }
}

hipError_t launch_read_survivors(const ReadSurvivorArgs &args, hipStream_t stream)
{
    if (args.n_spans == 0) return hipSuccess;
    const uint64_t blocks = (args.n_spans + RS_WG - 1) / RS_WG;
    if (blocks >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(read_survivors_kernel, dim3((unsigned)blocks), dim3(RS_WG), 0, stream, args);
    return hipGetLastError();
}

}  // namespace skl
