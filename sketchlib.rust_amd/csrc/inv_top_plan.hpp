// inv_top_plan.hpp -- HOW the best hits of an inverted query are selected on the device (inv_top.hip): the
// numbers of the launch (digits of the radix select, padded list length, LDS bytes), the index a lane of the descending walk
// reads, and inv_top_select_host(), the plain C++ form of the kernel's three steps that tests/native/inv_top_check.cpp checks
// against a sort of the keys.  The kernel takes every one of these numbers from here.  No HIP header.
//
// Hit r of a query is the indexed sample with the r-th largest key (count << 32) | index, compared as u64: counts descend and,
// at equal count, the HIGHER index comes first -- the reference's stable ascending sort of d / (2 S - d) followed by reverse()
// (src/lib.rs:1054-1055; d / (2 S - d) is strictly increasing in d, so sorting by it is sorting by d).
//
//   1. THRESHOLD: radix select on the count, most significant digit first, `w` bits a digit.  A pass histograms the current
//      digit of the entries whose higher digits equal the prefix chosen so far and walks the histogram from the top bin down to
//      the bin where the running total reaches what is still needed.  After the last pass: t = the n_eff-th largest count,
//      g = entries with count > t, e = n_eff - g >= 1 entries with count == t to take.
//   2. COLLECT from the high end: chunks of INV_TOP_THREADS entries from index n - 1 downward, lane order descending too.  An
//      entry is taken if count > t, or if count == t and fewer than e equal entries came before it in the walk: ties resolve to
//      the highest indices.  Entries above t go to list slots [0, g) in walk order, the equal ones to [g, n_eff).  (The kernel
//      loads INV_TOP_WALK_BATCH chunks at a time and then takes them one by one in this order: the same list.)
//   3. SORT the list descending (bitonic, padded to a power of two with key 0; real keys are unique, and a real key 0 is
//      (count 0, index 0), which sorts last among the real keys anyway).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace skl {

constexpr uint32_t INV_TOP_MAX = 1024;           // hits per query the LDS list holds (SKL_INVQ_TOP_MAX of the public header)
constexpr uint32_t INV_TOP_THREADS = 256;        // one workgroup per query; also the chunk of the descending walk
constexpr uint32_t INV_TOP_DIGIT_BITS = 11;      // default and widest digit: 2 048 LDS bins, one pass for S <= 2 047
constexpr uint32_t INV_TOP_PAD_ID = 0xFFFFFFFFu; // id of an entry past n_eff (its count is 0)
constexpr uint32_t INV_TOP_WALK_BATCH = 16;      // chunks of the descending walk whose loads are in flight together and whose totals cross one barrier
constexpr uint32_t INV_TOP_LDS_FIXED = 1056;     // u32: per-wave totals of the walk [2][INV_TOP_WALK_BATCH][2][4] and of the histogram scan [4], a pass's result [2]; rounded up
static_assert((2 * INV_TOP_WALK_BATCH * 8 + 4 + 2) * sizeof(uint32_t) <= INV_TOP_LDS_FIXED, "the fixed part holds the walk's totals");

inline uint32_t inv_top_n_eff(uint32_t top, uint32_t n) { return top < n ? top : n; }
// SKL_INVQ_TOP_DIGIT_BITS: 1..11 forces the width (tests drive several passes at small S), anything else is the default
inline uint32_t inv_top_digit_bits(long long knob)
{
    return knob >= 1 && knob <= (long long)INV_TOP_DIGIT_BITS ? (uint32_t)knob : INV_TOP_DIGIT_BITS;
}
inline uint32_t inv_top_bitlen(uint32_t v)
{
    uint32_t b = 0;
    for (; v; v >>= 1) ++b;
    return b;
}
// passes over the row: counts lie in [0, S]
inline uint32_t inv_top_digits(uint32_t sketch_size, uint32_t w)
{
    const uint32_t bits = inv_top_bitlen(sketch_size);
    return bits ? (bits + w - 1) / w : 1;
}
inline uint32_t inv_top_list_len(uint32_t top)   // the bitonic sort's length: the next power of two
{
    uint32_t len = 1;
    while (len < top) len <<= 1;
    return len;
}
// dynamic LDS of the launch: keys u64 [list_len], histogram u32 [2^w], the fixed part
inline uint32_t inv_top_lds_bytes(uint32_t top, uint32_t w)
{
    return inv_top_list_len(top) * (uint32_t)sizeof(uint64_t) + (1u << w) * (uint32_t)sizeof(uint32_t) + INV_TOP_LDS_FIXED;
}

// digit d (0: most significant) of a count, and the digits above it
#if defined(__HIPCC__)
#define SKL_INV_TOP_HD __host__ __device__
#else
#define SKL_INV_TOP_HD
#endif
SKL_INV_TOP_HD inline uint32_t inv_top_shift(uint32_t digits, uint32_t d, uint32_t w) { return (digits - 1u - d) * w; }
SKL_INV_TOP_HD inline uint32_t inv_top_digit(uint32_t count, uint32_t shift, uint32_t w) { return (count >> shift) & ((1u << w) - 1u); }
SKL_INV_TOP_HD inline uint32_t inv_top_above(uint32_t count, uint32_t shift, uint32_t w)   // (shift + w may be 32 or more: w = 1, S >= 2^31)
{
    return (uint32_t)((uint64_t)count >> (shift + w));
}
// the descending walk: chunks of a row of n entries, and the index lane `lane` of chunk `chunk` reads (valid while at < n)
SKL_INV_TOP_HD inline uint32_t inv_top_chunks(uint32_t n) { return (uint32_t)(((uint64_t)n + INV_TOP_THREADS - 1u) / INV_TOP_THREADS); }
SKL_INV_TOP_HD inline bool inv_top_walk_live(uint32_t n, uint32_t chunk, uint32_t lane) { return (uint64_t)chunk * INV_TOP_THREADS + lane < n; }
SKL_INV_TOP_HD inline uint32_t inv_top_walk_index(uint32_t n, uint32_t chunk, uint32_t lane) { return n - 1u - (chunk * INV_TOP_THREADS + lane); }
SKL_INV_TOP_HD inline uint64_t inv_top_key(uint32_t count, uint32_t index) { return ((uint64_t)count << 32) | index; }

struct InvTopThreshold {
    uint32_t t, g, e;   // n_eff-th largest count; entries above it; equal entries to take
};

// Step 1 on the host, pass by pass as the kernel runs it.  n >= 1, 1 <= n_eff <= n, every count < 2^(digits * w).
inline InvTopThreshold inv_top_threshold_host(const uint32_t *counts, uint32_t n, uint32_t n_eff, uint32_t digits, uint32_t w)
{
    std::vector<uint32_t> hist(1u << w);
    uint32_t prefix = 0, need = n_eff, g = 0;
    for (uint32_t d = 0; d < digits; ++d) {
        const uint32_t shift = inv_top_shift(digits, d, w);
        std::fill(hist.begin(), hist.end(), 0u);
        for (uint32_t i = 0; i < n; ++i) {
            if (inv_top_above(counts[i], shift, w) == prefix) ++hist[inv_top_digit(counts[i], shift, w)];
        }
        uint32_t above = 0, bin = (1u << w) - 1u;
        while (above + hist[bin] < need) above += hist[bin--];   // the entries of the prefix number at least `need`: ends at bin >= 0
        g += above;
        need -= above;
        prefix = (prefix << w) | bin;
    }
    return {prefix, g, need};
}

// Steps 1-3 on the host for one row: ids / counts [top], entries past n_eff padded.  n = 0: all padding.
inline void inv_top_select_host(const uint32_t *counts, uint32_t n, uint32_t sketch_size, uint32_t w, uint32_t top,
                                uint32_t *out_ids, uint32_t *out_counts, InvTopThreshold *thr_out = nullptr)
{
    const uint32_t n_eff = inv_top_n_eff(top, n);
    std::vector<uint64_t> list(inv_top_list_len(n_eff ? n_eff : 1), 0ull);
    if (n_eff) {
        const InvTopThreshold thr = inv_top_threshold_host(counts, n, n_eff, inv_top_digits(sketch_size, w), w);
        if (thr_out) *thr_out = thr;
        uint32_t got_gt = 0, seen_eq = 0;
        for (uint32_t chunk = 0; chunk < inv_top_chunks(n) && (got_gt < thr.g || seen_eq < thr.e); ++chunk) {
            for (uint32_t lane = 0; lane < INV_TOP_THREADS && inv_top_walk_live(n, chunk, lane); ++lane) {
                const uint32_t at = inv_top_walk_index(n, chunk, lane), c = counts[at];
                if (c > thr.t) list[got_gt++] = inv_top_key(c, at);
                else if (c == thr.t && seen_eq++ < thr.e) list[thr.g + seen_eq - 1] = inv_top_key(c, at);
            }
        }
        // the kernel's bitonic network, descending
        const uint32_t len = (uint32_t)list.size();
        for (uint32_t k = 2; k <= len; k <<= 1) {
            for (uint32_t j = k >> 1; j; j >>= 1) {
                for (uint32_t i = 0; i < len; ++i) {
                    const uint32_t x = i ^ j;
                    if (x > i && ((i & k) == 0 ? list[i] < list[x] : list[i] > list[x])) std::swap(list[i], list[x]);
                }
            }
        }
    }
    for (uint32_t r = 0; r < top; ++r) {
        out_ids[r] = r < n_eff ? (uint32_t)list[r] : INV_TOP_PAD_ID;
        out_counts[r] = r < n_eff ? (uint32_t)(list[r] >> 32) : 0u;
    }
}

}  // namespace skl
