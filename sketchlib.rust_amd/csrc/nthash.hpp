// nthash.hpp -- the arithmetic every sketching path shares, once: the split rotation ntHash and aaHash roll with, the ntHash
// seeds, `% SIGN_MOD`, the bin of a sign, the srol^(k-1) tables of a k-mer length and the 2-bit packing of base codes.
// Compiled for the host and the device: the kernels (sketch_kernel.hip, read_survivors.hip, aa_sketch_kernel.hip) call what
// tests/native/sketch_plan_check.cpp checks on the CPU.  No HIP header; plain g++ compiles it.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SKL_NT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SKL_NT_HD inline
#endif

namespace skl {

SKL_NT_HD uint64_t rotl1(uint64_t v) { return (v << 1) | (v >> 63); }
SKL_NT_HD uint64_t rotr1(uint64_t v) { return (v >> 1) | (v << 63); }
// swapbits033, src/hashing/mod.rs:99-103
SKL_NT_HD uint64_t swapbits033(uint64_t v)
{
    const uint64_t x = (v ^ (v >> 33)) & 1ull;
    return v ^ (x | (x << 33));
}
// the split 33 / 31-bit rotation the hashes roll with (nthash_iterator.rs:368-370, aahash_iterator.rs:15-21) and its inverse
SKL_NT_HD uint64_t srol(uint64_t v) { return swapbits033(rotl1(v)); }
SKL_NT_HD uint64_t sror(uint64_t v) { return rotr1(swapbits033(v)); }

// src/hashing/nthash_tables.rs:4-16 (index = 2-bit base code)
SKL_NT_HD uint64_t hash_fwd(uint32_t c)
{
    return c == 0 ? 0x3c8bfbb395c60474ull : c == 1 ? 0x3193c18562a02b4cull : c == 2 ? 0x295549f54be24456ull : 0x20323ed082572324ull;
}
SKL_NT_HD uint64_t hash_rc(uint32_t c) { return hash_fwd(c ^ 2u); }   // complement = code ^ 2

constexpr uint64_t SIGN_MOD = (1ull << 61) - 1;   // src/sketch/mod.rs:36
SKL_NT_HD uint64_t mod_sign(uint64_t h)
{
    const uint64_t r = (h & SIGN_MOD) + (h >> 61);   // 2^61 = 1 (mod 2^61 - 1)
    return r >= SIGN_MOD ? r - SIGN_MOD : r;
}

// SIGN_MOD.div_ceil(num_bins), sketch/mod.rs:170
SKL_NT_HD uint64_t bin_size_of(uint64_t num_bins) { return (SIGN_MOD + num_bins - 1) / num_bins; }

// bin = sign / bin_size for a sign below SIGN_MOD, without the division: the reciprocal estimate (inv_bin_size = 1.0 /
// (double)bin_size, clamped to last_bin = num_bins - 1) is off by at most one -- relative error 2^-52 on a quotient below 2^32 --
// and one exact product settles it.
SKL_NT_HD uint32_t bin_estimate(uint64_t sign, double inv_bin_size, uint32_t last_bin)
{
    const uint32_t bin = (uint32_t)((double)sign * inv_bin_size);
    return bin > last_bin ? last_bin : bin;
}
SKL_NT_HD uint32_t bin_of(uint64_t sign, double inv_bin_size, uint64_t bin_size, uint32_t last_bin)
{
    uint32_t bin = bin_estimate(sign, inv_bin_size, last_bin);
    const uint64_t prod = (uint64_t)bin * bin_size;
    if (prod > sign) --bin;
    else if (sign - prod >= bin_size && bin < last_bin) ++bin;
    return bin;
}

// srol^(k-1) of the forward / reverse-complement seed of each base: the weight of the base at distance k - 1
inline void nthash_top_tables(size_t k, uint64_t top_f[4], uint64_t top_r[4])
{
    for (uint32_t b = 0; b < 4; ++b) {
        uint64_t f = hash_fwd(b), r = hash_rc(b);
        for (size_t m = 1; m < k; ++m) {
            f = srol(f);
            r = srol(r);
        }
        top_f[b] = f;
        top_r[b] = r;
    }
}

// Sixteen one-byte codes -> one word of 2-bit codes (code c at bits 2 c).
inline uint32_t pack16(const uint8_t *src)
{
    uint64_t lo, hi;
    memcpy(&lo, src, 8);
    memcpy(&hi, src + 8, 8);
    auto squeeze = [](uint64_t v) -> uint32_t {   // 8 bytes of 2 significant bits -> 16 bits
        v &= 0x0303030303030303ull;
        v = (v | (v >> 6)) & 0x000F000F000F000Full;
        v = (v | (v >> 12)) & 0x000000FF000000FFull;
        v = (v | (v >> 24)) & 0xFFFFull;
        return (uint32_t)v;
    };
    return squeeze(lo) | (squeeze(hi) << 16);
}

// Words [w0, w1) of the ceil(n / 16) words of n one-byte codes: code c at bits 2 (c % 16) of word c / 16, the last word
// zero-padded.  out[w] receives word w.
inline void pack_code_words(const uint8_t *codes, uint64_t n, uint64_t w0, uint64_t w1, uint32_t *out)
{
    for (uint64_t w = w0; w < w1; ++w) {
        if (16 * w + 16 <= n) {
            out[w] = pack16(codes + 16 * w);
        } else {
            uint32_t word = 0;
            for (uint64_t c = 16 * w; c < n; ++c) word |= (uint32_t)(codes[c] & 3u) << (2u * (uint32_t)(c - 16 * w));
            out[w] = word;
        }
    }
}
inline void pack_codes(const uint8_t *codes, uint64_t n, uint32_t *out) { pack_code_words(codes, n, 0, (n + 15) / 16, out); }

}  // namespace skl
