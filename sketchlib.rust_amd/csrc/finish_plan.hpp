// finish_plan.hpp -- HOW a stream of bin minima is finished on the device (sketch_finish.hip): densify_bin
// (sketch/mod.rs:237-258) restated as two parallel steps, the launch rules of the kernel that runs them, and the plain C++ form
// of the same two steps that the library falls back to and tests/native/finish_plan_check.cpp checks against the sequential
// loop.  The kernel and the host share universal_hash and the target rule below.  No HIP header.
//
// densify_bin walks the bins in order and fills an empty bin i from the first probe j = universal_hash(i, t) % num_bins,
// t = 0, 1, ..., whose bin holds a value AT THAT MOMENT: every bin below i (already filled) or a bin that was never empty.  So
//   1. TARGET, per bin and independent of every other bin: a non-empty bin is its own target; an empty bin i takes the first
//      probe j with j < i or orig[j] != u64::MAX (a probe that lands on i itself is still empty and is passed over);
//   2. RESOLVE: a target that was itself empty lies strictly below i and took ITS target's value, so following targets ends at
//      an originally non-empty bin, the root, and the result is orig[root(i)].  By index, never by value: all 64 bits survive.
// A stream whose bins are all empty has no root (the reference's loop never ends on it): it is flagged and never probed.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define SKL_FINISH_HD __host__ __device__
#else
#define SKL_FINISH_HD
#endif

namespace skl {

constexpr uint64_t FINISH_EMPTY = ~0ull;     // an empty bin (u64::MAX)
constexpr uint32_t FINISH_PLANES = 14;       // BBITS: words per 64 bins of fill_usigs
// flag byte of a stream
constexpr uint8_t FINISH_DENSIFIED = 1;      // at least one bin was empty and filled from another
constexpr uint8_t FINISH_ALL_EMPTY = 2;      // every bin is u64::MAX: words zeroed, the error is the caller's
constexpr uint8_t FINISH_UNFINISHED = 4;     // a bin ran into the probe cap: the device's words are not valid, the host finishes the stream

// Threads per workgroup: a lane per bin up to four waves in the LDS form; the global form (large sketches, few streams) takes
// the 1 024 a workgroup may have, each thread num_bins / 1 024 bins.
constexpr uint32_t FINISH_WG_LDS = 256, FINISH_WG_GLOBAL = 1024;
// Most bins whose targets (a u32 each) and emptiness bits (num_bins / 8 bytes) live in LDS: 8 192 bins are 33 KiB, so four
// workgroups of 256 threads share a CU's 160 KiB -- 4 waves per SIMD, what the probe loop's dependent multiply-and-divide chain
// needs to keep the SIMDs busy -- and the launch stays below the 64 KiB of dynamic LDS that need no opt-in.  At the usual 1 024
// bins (4.1 KiB) the wave slots limit residency, not LDS: 8 workgroups per CU.
constexpr uint64_t FINISH_LDS_BINS_MAX = 8192;
// Probe cap per bin.  The worst probe count of a bin grows like ln(num_bins) / (fraction of non-empty bins): 489 at 99 % empty
// bins of 32 768, 9 to 12 at 50 %.  Only a single non-empty bin goes further (918 at 1 024 bins, 1 433 at 1 088, 6 070 at
// 4 096).  2 048 leaves a factor of four above every 99 %-empty sketch up to 32 768 bins and takes the single-bin sketches up
// to 1 088 bins; what needs more holds fewer than one non-empty bin in 200, is rare, and goes to the host.  A probe is about
// sixty instructions, so a bin that runs into the cap costs ~0.2 ms, and a stream stops probing once one of its bins has.
constexpr uint32_t FINISH_MAX_ATTEMPTS = 2048;
// Pointer-jumping rounds: every round at least halves a chain of at most 2^32 targets, so 33 rounds always suffice (6 seen);
// the loop is bounded by the constant, not by the data.
constexpr uint32_t FINISH_MAX_ROUNDS = 40;
// The global form's target arrays: [workgroups][num_bins] u32 in a scratch slot of at most this many bytes.
constexpr uint64_t FINISH_TARGET_BYTES = 256ull << 20;
constexpr uint32_t FINISH_GLOBAL_WGS_MAX = 1024;

inline bool finish_lds_form(uint64_t num_bins) { return num_bins <= FINISH_LDS_BINS_MAX; }
inline uint32_t finish_threads(uint64_t num_bins)   // num_bins: a multiple of 64
{
    if (!finish_lds_form(num_bins)) return FINISH_WG_GLOBAL;
    return (uint32_t)(num_bins < FINISH_WG_LDS ? num_bins : FINISH_WG_LDS);
}
inline uint32_t finish_max_attempts(long long knob) { return knob > 0 ? (uint32_t)(knob < (1ll << 30) ? knob : (1ll << 30)) : FINISH_MAX_ATTEMPTS; }
// workgroups of a launch over n_streams: one per stream in the LDS form; the global form walks the streams with as many
// workgroups as the target scratch holds arrays for (at least one: a single array may exceed FINISH_TARGET_BYTES)
inline uint64_t finish_workgroups(uint64_t n_streams, uint64_t num_bins)
{
    if (finish_lds_form(num_bins)) return n_streams;
    uint64_t fit = FINISH_TARGET_BYTES / (num_bins * sizeof(uint32_t));
    if (fit < 1) fit = 1;
    if (fit > FINISH_GLOBAL_WGS_MAX) fit = FINISH_GLOBAL_WGS_MAX;
    return n_streams < fit ? n_streams : fit;
}
inline uint64_t finish_lds_bytes(uint64_t num_bins) { return finish_lds_form(num_bins) ? num_bins * sizeof(uint32_t) + num_bins / 8 : 0; }
inline uint64_t finish_words(uint64_t num_bins) { return num_bins / 64 * FINISH_PLANES; }   // u64 words of a finished stream

// The u16 form (an inverted index's row: exactly num_bins bins, `sign as u16` each) takes any num_bins from 1 to 2^32 - 1.
// Its workgroups are WHOLE WAVES: the kernel strides its chunk loops by n_waves = blockDim.x >> 6, and a workgroup of fewer
// than 64 threads (finish_threads(10) would be 10) has n_waves == 0 -- a `c += n_waves` loop would never end.  Rounding up to
// 64 makes that impossible: the result is a multiple of 64 and at least 64 for every num_bins >= 1.  At multiples of 64 the
// values are finish_threads' / finish_lds_bytes'.
inline uint32_t finish_threads_u16(uint64_t num_bins)
{
    if (!finish_lds_form(num_bins)) return FINISH_WG_GLOBAL;
    const uint64_t whole_waves = (num_bins + 63) / 64 * 64;
    return (uint32_t)(whole_waves < FINISH_WG_LDS ? (whole_waves ? whole_waves : 64) : FINISH_WG_LDS);
}
// targets [num_bins] u32, then the "holds a value" bits, a u32 per 32 bins (the last one partly used)
inline uint64_t finish_lds_bytes_u16(uint64_t num_bins)
{
    return finish_lds_form(num_bins) ? num_bins * sizeof(uint32_t) + (num_bins + 31) / 32 * sizeof(uint32_t) : 0;
}

// sketch/mod.rs:225-231, in wrapping u64
SKL_FINISH_HD inline uint64_t finish_universal_hash(uint64_t s, uint64_t t)
{
    const uint64_t x = s * 1009ull + t * 1000003ull;
    return (x * 48271ull + 11ull) % 2147483647ull;
}

// Step 1 for the empty bin i.  is_filled(j): whether orig[j] != u64::MAX.  Returns the target, or i itself when max_attempts
// probes found none (max_attempts 0: no cap) -- an empty bin is never its own target otherwise.  *probes (if asked for): probes made.
template <class Filled>
SKL_FINISH_HD inline uint32_t finish_target(uint32_t i, uint32_t num_bins, uint32_t max_attempts, const Filled &is_filled,
                                            uint32_t *probes = nullptr)
{
    for (uint32_t t = 0; max_attempts == 0 || t < max_attempts; ++t) {
        const uint32_t j = (uint32_t)finish_universal_hash(i, t) % num_bins;
        if (j < i || is_filled(j)) {
            if (probes) *probes = t + 1;
            return j;
        }
    }
    if (probes) *probes = max_attempts;
    return i;
}

// The two steps on the host, one stream: `signs` densified in place as densify_bin leaves them; returns the flag byte.
// (Targets below i are resolved before i, so one ascending pass resolves; the kernel jumps pointers instead.)  max_attempts 0:
// no cap, the library's fall-back.  With a cap a stream may come back FINISH_UNFINISHED, its signs untouched.
inline uint8_t finish_densify_two_step(std::vector<uint64_t> &signs, uint32_t max_attempts = 0, uint32_t *worst_probes = nullptr)
{
    const uint32_t n = (uint32_t)signs.size();
    bool any_empty = false, any_filled = false;
    for (uint64_t v : signs) (v == FINISH_EMPTY ? any_empty : any_filled) = true;
    if (!any_empty) return 0;
    if (!any_filled) return FINISH_ALL_EMPTY;
    std::vector<uint32_t> tgt(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (signs[i] != FINISH_EMPTY) {
            tgt[i] = i;
            continue;
        }
        uint32_t probes = 0;
        tgt[i] = finish_target(i, n, max_attempts, [&](uint32_t j) { return signs[j] != FINISH_EMPTY; }, &probes);
        if (worst_probes && probes > *worst_probes) *worst_probes = probes;
        if (tgt[i] == i) return FINISH_UNFINISHED;
    }
    std::vector<uint32_t> root(n);
    for (uint32_t i = 0; i < n; ++i) {   // a target is originally filled (a root) or lies below i (resolved already)
        root[i] = signs[i] != FINISH_EMPTY ? i : signs[tgt[i]] != FINISH_EMPTY ? tgt[i] : root[tgt[i]];
    }
    std::vector<uint64_t> out(n);
    for (uint32_t i = 0; i < n; ++i) out[i] = signs[root[i]];
    signs.swap(out);
    return FINISH_DENSIFIED;
}

// fill_usigs (sketch/mod.rs:215-223) into finish_words(n) zeroed-or-not words: word c * 14 + p holds bit p of bins 64 c .. 64 c + 63
inline void finish_transpose(const std::vector<uint64_t> &signs, uint64_t *usigs)
{
    for (size_t c = 0; c < signs.size() / 64; ++c) {
        for (uint32_t p = 0; p < FINISH_PLANES; ++p) {
            uint64_t w = 0;
            for (uint32_t l = 0; l < 64; ++l) w |= ((signs[64 * c + l] >> p) & 1ull) << l;
            usigs[c * FINISH_PLANES + p] = w;
        }
    }
}

// One stream on the host, as the kernel leaves it: words, first sign, flag.
inline uint8_t finish_stream_host(const uint64_t *signs, uint64_t num_bins, uint64_t *usigs, uint64_t *first_sign)
{
    std::vector<uint64_t> sg(signs, signs + num_bins);
    const uint8_t flag = finish_densify_two_step(sg);
    if (flag & FINISH_ALL_EMPTY) {
        for (uint64_t w = 0; w < finish_words(num_bins); ++w) usigs[w] = 0;
    } else {
        finish_transpose(sg, usigs);
    }
    if (first_sign) *first_sign = sg[0];
    return flag;
}

// One stream on the host in the u16 form, as the kernel leaves it: densified, `sign as u16` per bin (any num_bins); returns
// the flag.  An all-empty stream gives a zeroed row.
inline uint8_t finish_stream_host_u16(const uint64_t *signs, uint64_t num_bins, uint16_t *out_u16)
{
    std::vector<uint64_t> sg(signs, signs + num_bins);
    const uint8_t flag = finish_densify_two_step(sg);
    for (uint64_t i = 0; i < num_bins; ++i) out_u16[i] = (flag & FINISH_ALL_EMPTY) ? (uint16_t)0 : (uint16_t)sg[i];
    return flag;
}

}  // namespace skl
