// aa_sketch_kernel.hip -- amino-acid sketching on the GPU (gfx950): forward aaHash of every window of k valid
// residues, `% SIGN_MOD`, bin minimum -- Sketch::get_signs_no_densify (src/sketch/mod.rs:156-176) over the reference's
// AaHashIterator (src/hashing/aahash_iterator.rs:138-210), all samples and k-mer lengths of a batch in two launches.
//
// Input: one byte per stored residue, a CLASS CODE prepared on the host (0 = separator: an invalid residue or a record end;
// 1..20 = the letter).  Bytes, not 5-bit fields: six 5-bit codes fill a dword with two bits to spare (5.3 bits per residue
// against 8) and cost a shift and a mask more per residue on a path that a protein's 8 KiB of returned signs outweighs 25 : 1;
// codes, not ASCII: validity is `code != 0` and the two tables of a k-mer length (seed[new], srol^k(seed[old])) have 21 rows of
// 8 bytes, not 256 -- each within one sweep of the 64 LDS banks, so lanes that read different rows never collide -- and a level
// is only other table contents.  (A fused [old][new] table, 441 x 8 bytes, is one read per window instead of two, but 64 lanes
// spread over it collide three or four deep: measured 0.41 ms against 0.32 ms on 96 M windows, profiles/sketch_aa.md.)  There
// is no offsets array.
//
// A separator has seed 0 and roll value 0, so a hash rolled straight through one is still the XOR of srol^distance(seed) over
// the valid residues of the window: exact for every window of k valid residues, nothing is re-seeded (one seed of k - 1 steps
// per thread and k-mer length).  A thread carries the count of valid residues since the last separator; a window is hashed
// into a bin iff that count reaches k -- and, under `end_rule`, the sample's last window only if the residue before it is valid
// (the reference's iterator reaches the window at len - k only by rolling).
//
// Two forms, dealt by aa_plan.hpp: staged (a workgroup per chunk of one long sample: residues, tables and bin minima in
// LDS) and unstaged (a thread per span of any sample, packed without padding; bins in global memory).
#include "kernels.h"
#include "nthash.hpp"   // srol, mod_sign, bin_of

namespace skl {

namespace {
constexpr uint32_t AA_TAB = 21;                                   // residue codes
constexpr uint32_t AA_PITCH_DW = AA_SPAN_LDS / 4 + 1;             // dwords per staged row: 16 of residues + 1 of padding
// dwords staged: the chunk, plus what the last thread's windows reach past it (k - 1 <= 255 residues), plus the look-ahead dword
constexpr uint32_t AA_STAGED_DW = AA_CHUNK / 4 + (AA_K_STAGED_MAX - 1) / 4 + 1;   // 4 160
constexpr uint32_t AA_ROWS = (AA_STAGED_DW + AA_SPAN_LDS / 4 - 1) / (AA_SPAN_LDS / 4);   // 260
}  // namespace

// ---------------------------------------------------------------------------------------------
// Staged form: workgroup = AA_WG_LDS spans of AA_SPAN_LDS window starts of ONE sample.  The residues are staged as they are, four
// per dword, rows of 16 dwords at a pitch of 17 (lanes that read the same column of consecutive rows hit different banks); a
// thread keeps the residues that leave and enter its next four windows in two registers (one LDS dword per stream and four
// windows) and reads one 8-byte entry of each of the two 21-row tables per window.
// ---------------------------------------------------------------------------------------------
template <bool LDS_BINS>
__global__ __launch_bounds__(AA_WG_LDS) void aahash_binmin_lds_kernel(const AaSketchArgs g)
{
    __shared__ uint32_t staged[AA_ROWS * AA_PITCH_DW];
    __shared__ unsigned long long tab[AA_TAB], rtab[AA_TAB];   // seed[new]; srol^k(seed[old]) of the current k-mer length
    __shared__ unsigned long long lbins[LDS_BINS ? AA_LDS_BINS_MAX : 1];
    const uint32_t tid = threadIdx.x;
    const AaItem it = aa_long_item(g.item_begin, g.res_begin, g.n_samples, g.first_item + blockIdx.x, tid);
    const uint32_t sample = it.sample;
    const uint64_t len = g.res_begin[sample + 1] - g.res_begin[sample];
    const uint64_t wg0 = it.first - (uint64_t)tid * AA_SPAN_LDS;   // first residue of the workgroup
    if (wg0 >= len) return;                                        // (never: the plan gives a sample exactly its chunks)
    const uint8_t *src = g.codes + (g.res_begin[sample] - g.res_base);   // the sample's residues
    const uint64_t left = len - wg0;
    const uint32_t n_staged = left < (uint64_t)AA_STAGED_DW * 4u ? (uint32_t)left : AA_STAGED_DW * 4u;
    {
        // The sample starts at any byte: whole dwords are read from the aligned address below and shifted into place (the
        // buffer starts 256-byte aligned and ends 8 bytes after its last residue); bytes past the sample are separators.
        const uint8_t *p = src + wg0;
        const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
        const uint32_t *al = (const uint32_t *)(p - mis);
        for (uint32_t d = tid; d < AA_STAGED_DW; d += AA_WG_LDS) {
            uint32_t word = 0u;
            if (d * 4u < n_staged) {
                const uint32_t lo = al[d];
                word = mis ? (lo >> (8u * mis)) | (al[d + 1] << (32u - 8u * mis)) : lo;
                const uint32_t rem = n_staged - d * 4u;
                if (rem < 4u) word &= (1u << (8u * rem)) - 1u;
            }
            staged[(d >> 4) * AA_PITCH_DW + (d & 15u)] = word;
        }
    }
    if (LDS_BINS) {
        for (uint32_t b = tid; b < (uint32_t)g.num_bins; b += AA_WG_LDS) lbins[b] = ~0ull;
    }
    auto dword_at = [&](uint32_t m) -> uint32_t { return staged[(m >> 4) * AA_PITCH_DW + (m & 15u)]; };
    auto code_at = [&](uint32_t x) -> uint32_t { return (dword_at(x >> 2) >> ((x & 3u) * 8u)) & 0xFFu; };   // residue x from wg0
    const uint64_t p0 = it.first;
    const uint32_t x0 = tid * AA_SPAN_LDS;
    const uint32_t last_bin = (uint32_t)(g.num_bins - 1u);

    for (uint32_t ki = 0; ki < g.nk; ++ki) {
        const uint32_t k = g.kmers[ki];
        __syncthreads();   // staged / lbins ready (first k); everyone done with the previous k's table
        if (tid < AA_TAB) {
            tab[tid] = g.seeds[tid];
            rtab[tid] = g.roll[ki * AA_TAB + tid];
        }
        __syncthreads();
        uint64_t *bins = g.signs + ((uint64_t)(sample - g.sample_base) * g.nk + ki) * g.num_bins;
        const uint64_t n_starts = len >= k ? len - k + 1u : 0u;   // window starts of the sample
        const uint32_t n_win = p0 < n_starts ? (uint32_t)(n_starts - p0 < AA_SPAN_LDS ? n_starts - p0 : AA_SPAN_LDS) : 0u;
        if (n_win != 0u) {
            // seed: the k - 1 residues before the one that enters window 0 (tab = the seeds)
            uint64_t fh = 0;
            uint32_t run = 0;   // valid residues since the last separator
            for (uint32_t i = 0; i + 1u < k; ++i) {
                const uint32_t c = code_at(x0 + i);
                fh = srol(fh) ^ tab[c];
                run = c ? run + 1u : 0u;
            }
            // the sample's last window under the end rule: hashed only if the residue before it is valid; for the first
            // window of a thread that residue is not among the ones it walks
            const bool ends_here = g.end_rule && p0 + n_win == n_starts;
            const uint32_t before_first = ends_here && p0 != 0u ? src[p0 - 1u] : 0u;
            const uint32_t a = k - 1u;                        // lag of the entering residue
            const uint32_t da = a >> 2, pa = (a & 3u) * 8u;
            uint32_t d_prev = 0u;                             // (window 0 has no leaving residue: code 0)
            uint32_t e_prev = dword_at((x0 >> 2) + da);
            for (uint32_t q = 0; q < AA_SPAN_LDS / 4 && q * 4u < n_win; ++q) {
                const uint32_t d_cur = dword_at((x0 >> 2) + q);
                const uint32_t e_cur = dword_at(min((x0 >> 2) + q + da + 1u, AA_STAGED_DW - 1u));
                // four residues from index 4 q - 1 (leaving) and 4 q + k - 1 (entering) of this thread's row
                const uint32_t old_reg = __builtin_amdgcn_alignbit(d_cur, d_prev, 24);
                const uint32_t new_reg = pa ? __builtin_amdgcn_alignbit(e_cur, e_prev, pa) : e_prev;
                d_prev = d_cur;
                e_prev = e_cur;
#pragma unroll
                for (uint32_t jj = 0; jj < 4u; ++jj) {
                    const uint32_t j = q * 4u + jj;
                    if (j >= n_win) break;
                    const uint32_t old_c = j ? (old_reg >> (8u * jj)) & 0xFFu : 0u;
                    const uint32_t new_c = (new_reg >> (8u * jj)) & 0xFFu;
                    fh = srol(fh) ^ tab[new_c] ^ rtab[old_c];
                    run = new_c ? run + 1u : 0u;
                    if (run < k) continue;   // a separator in the window: not hashed into a bin
                    if (ends_here && j + 1u == n_win && (j ? old_c : before_first) == 0u) continue;
                    const uint64_t sign = mod_sign(fh);
                    const uint32_t bin = bin_of(sign, g.inv_bin_size, g.bin_size, last_bin);
                    if (LDS_BINS) {
                        if (sign < lbins[bin]) atomicMin(&lbins[bin], (unsigned long long)sign);
                    } else {
                        if (sign < bins[bin]) atomicMin((unsigned long long *)&bins[bin], (unsigned long long)sign);
                    }
                }
            }
        }
        if (LDS_BINS) {   // one global atomic per bin this workgroup touched
            __syncthreads();
            for (uint32_t b = tid; b < (uint32_t)g.num_bins; b += AA_WG_LDS) {
                const unsigned long long v = lbins[b];
                if (v != ~0ull) {
                    if (v < bins[b]) atomicMin((unsigned long long *)&bins[b], v);
                    lbins[b] = ~0ull;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Unstaged form: thread = one span of `short_span` window starts of any sample; consecutive threads take consecutive spans,
// across samples, so a workgroup holds a dozen short proteins.  Residues come from global memory (a protein is read by the
// few neighbouring lanes that share its cache lines), seeds and roll values of the current k-mer length from LDS, and every
// window that lowers its bin issues a global atomicMin -- for a protein of a few hundred windows over a thousand bins nearly
// every window does, which is the cost of this shape whatever the form.  Also the form of k > AA_K_STAGED_MAX.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AA_WG_SHORT) void aahash_binmin_kernel(const AaSketchArgs g)
{
    __shared__ unsigned long long s_seed[AA_TAB], s_roll[AA_TAB];
    const uint32_t tid = threadIdx.x;
    const uint64_t idx = (uint64_t)blockIdx.x * AA_WG_SHORT + tid;
    const bool active = idx < g.n_items;
    AaItem it{0u, 0u, 0u};
    if (active) it = aa_short_item(g.item_begin, g.res_begin, g.n_samples, g.short_span, g.first_item + idx);
    const uint64_t len = active ? g.res_begin[it.sample + 1] - g.res_begin[it.sample] : 0u;
    const uint8_t *src = g.codes + (active ? g.res_begin[it.sample] - g.res_base : 0u);
    const uint64_t p0 = it.first;
    const uint32_t last_bin = (uint32_t)(g.num_bins - 1u);
    if (tid < AA_TAB) s_seed[tid] = g.seeds[tid];

    for (uint32_t ki = 0; ki < g.nk; ++ki) {
        const uint32_t k = g.kmers[ki];
        __syncthreads();   // everyone done with the previous k's roll values (and s_seed written)
        if (tid < AA_TAB) s_roll[tid] = g.roll[ki * AA_TAB + tid];
        __syncthreads();
        const uint64_t n_starts = len >= k ? len - k + 1u : 0u;
        const uint32_t n_win = p0 < n_starts ? (uint32_t)(n_starts - p0 < it.count ? n_starts - p0 : it.count) : 0u;
        if (n_win == 0u) continue;   // (uniform barriers: the loop bound and the two syncs do not depend on it)
        uint64_t *bins = g.signs + ((uint64_t)(it.sample - g.sample_base) * g.nk + ki) * g.num_bins;
        uint64_t fh = 0;
        uint32_t run = 0;
        for (uint32_t i = 0; i + 1u < k; ++i) {
            const uint32_t c = src[p0 + i];
            fh = srol(fh) ^ s_seed[c];
            run = c ? run + 1u : 0u;
        }
        const bool ends_here = g.end_rule && p0 + n_win == n_starts;
        uint32_t old_c = 0u;                                           // (window 0 has no leaving residue)
        uint32_t before = ends_here && p0 != 0u ? src[p0 - 1u] : 0u;   // the residue before window j
        for (uint32_t j = 0; j < n_win; ++j) {
            const uint32_t new_c = src[p0 + j + k - 1u];
            fh = srol(fh) ^ s_seed[new_c] ^ s_roll[old_c];
            run = new_c ? run + 1u : 0u;
            const uint32_t leaving_next = src[p0 + j];
            const bool skip_last = ends_here && j + 1u == n_win && before == 0u;
            old_c = leaving_next;
            before = leaving_next;
            if (run < k || skip_last) continue;
            const uint64_t sign = mod_sign(fh);
            const uint32_t bin = bin_of(sign, g.inv_bin_size, g.bin_size, last_bin);
            if (sign < bins[bin]) atomicMin((unsigned long long *)&bins[bin], (unsigned long long)sign);
        }
    }
}

hipError_t launch_aa_sketch_signs(const AaSketchArgs &args, hipStream_t stream)
{
    if (args.n_items == 0) return hipSuccess;
    const uint64_t blocks = args.staged ? args.n_items : (args.n_items + AA_WG_SHORT - 1) / AA_WG_SHORT;
    if (blocks >= (1ull << 31)) return hipErrorInvalidValue;
    if (!args.staged) {
        hipLaunchKernelGGL(aahash_binmin_kernel, dim3((unsigned)blocks), dim3(AA_WG_SHORT), 0, stream, args);
    } else if (args.num_bins <= (uint64_t)AA_LDS_BINS_MAX) {
        hipLaunchKernelGGL(aahash_binmin_lds_kernel<true>, dim3((unsigned)blocks), dim3(AA_WG_LDS), 0, stream, args);
    } else {
        hipLaunchKernelGGL(aahash_binmin_lds_kernel<false>, dim3((unsigned)blocks), dim3(AA_WG_LDS), 0, stream, args);
    }
    return hipGetLastError();
}

}  // namespace skl
