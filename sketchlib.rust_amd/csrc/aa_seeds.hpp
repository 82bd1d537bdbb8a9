// aa_seeds.hpp -- the aaHash seed tables by residue code, and the roll values derived from them.  Plain C++, no HIP header:
// shared by the library (capi_aa.cpp uploads them) and the host layer (host/aahash.cpp hashes with them on the CPU).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "nthash.hpp"

namespace skl {

constexpr int AA_N_CODES = 21;   // 0 = separator, then ACDEFGHIKLMNPQRSTVWY

// The published aaHash seeds (Wong, Kazemi, Coombe, Warren, Birol: "aaHash: recursive amino acid sequence hashing",
// Bioinformatics Advances 3(1), 2023, doi:10.1093/bioadv/vbad162), by residue code.  A separator's seed is 0.
inline const uint64_t *aa_seed_table(int level)
{
    static const uint64_t L1[AA_N_CODES] = {
        0,
        0xf56d6192468323dfull /*A*/, 0x9b0b2fd724e1e1d2ull /*C*/, 0xe8c583296b03c7afull /*D*/, 0x06d8186850ee2f67ull /*E*/,
        0x921e1da156b717adull /*F*/, 0xa70dc450015e3ffeull /*G*/, 0x2242263a9d5638ffull /*H*/, 0x2469ca06d519cdefull /*I*/,
        0xd4e7f06ac0593d3bull /*K*/, 0xa5e19c0b1b40a97full /*L*/, 0xfab3d6d4dd74c000ull /*M*/, 0x4b363f2cf7bc5200ull /*N*/,
        0x21ac8af2adb65ce4ull /*P*/, 0x1d3baae9ab7cd800ull /*Q*/, 0x049015253a9dbedfull /*R*/, 0x5bf1f1d7ae699000ull /*S*/,
        0xdb0c63dd7282cf90ull /*T*/, 0x7df64ddf78874000ull /*V*/, 0xee9e700cae6aa279ull /*W*/, 0x5852ffb781a97610ull /*Y*/};
    // level 2: C G A N H P alone; ST, DE, KQR, ILMV, FWY share a seed
    constexpr uint64_t C2 = 0x1d07fd644abe9962ull, G2 = 0xf59c50929bdf4360ull, A2 = 0x6f735c82fe9c6c03ull, ST2 = 0xe7392f0ba1dbc3b0ull,
                       N2 = 0x956ddcfcd4b3961full, DE2 = 0x4ec0ef1bac4f5efaull, KQR2 = 0x1cd6ca491872ed78ull,
                       ILMV2 = 0x547ef17894921035ull, FWY2 = 0x419722edb87bf79full, H2 = 0xdd5cce5bfdc32de1ull,
                       P2 = 0x90e0c5e0c07d6598ull;
    //                                        A   C   D    E    F     G   H   I      K     L      M      N   P   Q     R     S    T    V      W     Y
    static const uint64_t L2[AA_N_CODES] = {0, A2, C2, DE2, DE2, FWY2, G2, H2, ILMV2, KQR2, ILMV2, ILMV2, N2, P2, KQR2, KQR2, ST2, ST2, ILMV2, FWY2, FWY2};
    // level 3: C G H P alone; AST, DEN, KQR, ILMV, FWY share a seed
    constexpr uint64_t C3 = 0x5713e4c10cebbfa3ull, G3 = 0xbe084b869537379bull, AST3 = 0x985fd9efa0fe5b82ull, DEN3 = 0x9aca6c4f4ef69df0ull,
                       KQR3 = 0x917de473b721df0eull, ILMV3 = 0x37cdd84aa07c5bd7ull, FWY3 = 0x51a7955f1a67a896ull,
                       H3 = 0x1d2a0ba493708fbfull, P3 = 0xfe4c47da16611245ull;
    static const uint64_t L3[AA_N_CODES] = {0, AST3, C3, DEN3, DEN3, FWY3, G3, H3, ILMV3, KQR3, ILMV3, ILMV3, DEN3, P3, KQR3, KQR3, AST3, AST3, ILMV3, FWY3, FWY3};
    return level == 1 ? L1 : level == 2 ? L2 : level == 3 ? L3 : nullptr;
}

// srol^k of each seed: what a residue contributes when it leaves a window of k (the reference tabulates these values split
// into a 31-bit and a 33-bit half, indexed by k % 31 and k % 33: aahash_tables.rs:18-35).  srol has period lcm(33, 31) = 1023.
inline void aa_roll_table(const uint64_t *seeds, size_t k, uint64_t out[AA_N_CODES])
{
    for (int c = 0; c < AA_N_CODES; ++c) {
        uint64_t v = seeds[c];
        for (size_t m = 0; m < k % 1023; ++m) v = srol(v);   // the split rotation, nthash.hpp
        out[c] = v;
    }
}

}  // namespace skl
