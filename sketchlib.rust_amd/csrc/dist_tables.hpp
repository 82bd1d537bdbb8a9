// dist_tables.hpp -- the lookup tables every dense output rests on, as pure host arithmetic: bin matches -> Jaccard index, its
// logarithm (the regression's y values and the early break's test), and the single-k distance / ANI.  Computed with the host
// libm, i.e. bit-identical to what the reference's f64 arithmetic produces on this machine (build with -ffp-contract=off).  No HIP
// header: capi_tables.cpp only allocates and copies what these return; tests/native/dist_tables_check.cpp checks them on the CPU.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace skl {

constexpr int TABLE_BBITS = 14;                          // = BBITS of kernels.h (capi_tables.cpp asserts they agree)
constexpr int TABLE_JOUT_DIST = 0, TABLE_JOUT_ANI = 1;   // = JOUT_DIST, JOUT_ANI; anything else: the kNN sort key 1 - ANI

// jaccard.rs:14,26-33 with no completeness: J as a function of samebits alone.
inline double host_jaccard(uint32_t samebits, size_t ss64)
{
    const double unionsize = (double)(64u * ss64);
    const uint32_t maxnbits = (uint32_t)ss64 * 64u;
    const uint32_t expected = maxnbits >> TABLE_BBITS;
    const uint32_t diff = samebits > expected ? samebits - expected : 0u;
    const double intersize = ((double)diff * (double)maxnbits) / (double)(maxnbits - expected);
    return intersize / unionsize;
}

// jaccard.rs:75: a k-mer length whose ln J falls below this ends the reference's loop
inline double break_tolerance(size_t ss64) { return std::log(2.0 / (double)((ss64 * 64ull) * 64ull)); }

// ln J for every count of matching bins, [64 * ss64 + 1], and the break test of jaccard.rs:89-91 on the count itself:
// ln J(count) < tolerance <=> count < min_alive -- if the table is monotone there (it is; checked, not assumed: 0xFFFFFFFF makes
// the kernels ask the table)
struct LnjTable {
    std::vector<double> lnj;
    uint32_t min_alive = 0xFFFFFFFFu;
};
inline LnjTable lnj_table(size_t ss64)
{
    LnjTable t;
    const size_t m = 64 * ss64 + 1;
    t.lnj.resize(m);
    for (size_t b = 0; b < m; ++b) t.lnj[b] = std::log(host_jaccard((uint32_t)b, ss64));
    const double tolerance = break_tolerance(ss64);
    size_t first = 0;
    while (first < m && t.lnj[first] < tolerance) ++first;
    bool monotone = true;
    for (size_t b = first; b < m; ++b) monotone = monotone && !(t.lnj[b] < tolerance);
    t.min_alive = monotone ? (uint32_t)first : 0xFFFFFFFFu;
    return t;
}

// the single-k output for every count of matching bins, [64 * ss64 + 1]: distance, ANI at k-mer length k, or the kNN key 1 - ANI
inline std::vector<float> dist_table(int jout, double k, size_t ss64)
{
    const size_t m = 64 * ss64 + 1;
    std::vector<float> tab(m);
    for (size_t b = 0; b < m; ++b) {
        const double j = host_jaccard((uint32_t)b, ss64);
        if (jout == TABLE_JOUT_DIST) {
            tab[b] = (float)(1.0 - j);  // mod.rs:99
        } else {
            // jaccard.rs:49-51
            const double ani = std::fmax(0.0, 1.0 + 1.0 / k * std::log((2.0 * j) / (1.0 + j)));
            tab[b] = jout == TABLE_JOUT_ANI ? (float)ani : (float)(1.0 - ani);  // mod.rs:97 / :173-176
        }
    }
    return tab;
}

}   // namespace skl
