// eb_stripes.hpp -- COLUMN STRIPES FOLDED ONTO THE XCDs: the third order of the early-break epilogue (epilogue.hip, beside the
// flat and the blocked one), forward (the host's grid) and inverse (the kernel's decode of its workgroup index), as plain
// functions of the launch's fields, in the style of work_map.hpp: nothing here touches a device or needs a device header
// (tests/native/eb_stripes_check.cpp hands it a plain struct).
//
// A completion reads its column sample's slice.  In the flat order workgroup b covers 256 consecutive columns of a row and lands
// on XCD b mod X, so every XCD is asked for every column slice of a length (n = 1 000 at 4 096 bins: 7 MB against a 4 MB L2).
// Here the launch's columns are cut into 2 X stripes of W = 64 ceil(n_cols / (128 X)) columns and XCD x owns stripes x and
// 2 X - 1 - x: it is asked for 2 W slices of a length and nothing else.  The FOLD balances the triangle: in self mode stripe s
// of width 64 holds 4 096 s + 2 016 pairs, so the two stripes of an XCD always sum to the same number (only the launch's last,
// partial stripe takes from it: n = 1 000 on 8 XCDs, XCD 0 holds 41 196 pairs, every other one 65 472, the mean is 62 437.5).
//
// A workgroup of 256 threads = two consecutive rows of the launch (row_begin + 2 rp, + 1) against ONE 64-column block of each
// of its XCD's two stripes: wave w takes row w & 1; waves 0 and 1 the block of stripe x, waves 2 and 3 the block of stripe
// 2 X - 1 - x.  A wave's 64 pairs are consecutive in the counts and in the output.  Workgroup b is on XCD b mod X and is slot
// b / X there; the slot enumerates (row pair, block of the stripe), block fastest: the workgroups resident on an XCD at one
// time share their rows.
//
// The functions read these fields of the argument struct (EpilogueArgs, kernels.h): self_mode, row_begin, row_end, nB_cols,
// xcd_shift, and -- written by the forward side -- stripe_w, stripe_rp.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define SKL_STRIPE_FN __host__ __device__ __forceinline__
#else
#define SKL_STRIPE_FN inline
#endif

namespace skl {

// W: columns per stripe (a multiple of 64: a 64-column block never straddles two stripes)
SKL_STRIPE_FN uint32_t eb_stripe_width(uint64_t n_cols, uint32_t xcd_shift)
{
    const uint64_t per = 128ull << xcd_shift;
    return (uint32_t)(64u * ((n_cols + per - 1u) / per));
}

// bytes of one k-mer length's slices an XCD is asked for: its two stripes' columns, ss64 chunks of 14 x 8 bytes each
SKL_STRIPE_FN uint64_t eb_stripe_slice_bytes(uint64_t n_cols, uint32_t xcd_shift, uint32_t ss64)
{
    return 2ull * eb_stripe_width(n_cols, xcd_shift) * ss64 * 112ull;
}

// pairs of rows [r0, r1) in columns [0, t): column j holds the rows below it (self mode), or every row
SKL_STRIPE_FN uint64_t eb_stripe_pairs_before(bool self_mode, uint64_t r0, uint64_t r1, uint64_t t)
{
    const uint64_t rows = r1 - r0;
    if (!self_mode) return rows * t;
    if (t <= r0 + 1u) return 0;
    if (t <= r1 + 1u) return (t - 1u - r0) * (t - r0) / 2u;
    return rows * (rows + 1u) / 2u + (t - 1u - r1) * rows;
}

// THE BALANCE: pairs of the heaviest XCD over the mean, for rows [r0, r1) against n_cols columns.  The kernel ends with its
// slowest XCD.  The fold evens out the triangle, not a column count well short of 2 X W: at n = 1 500 on 8 XCDs (W = 128) only
// stripes 0 ... 11 hold columns, XCDs 0 ... 3 own one of them each and XCDs 4 ... 7 two of the longest: 1.86.
SKL_STRIPE_FN double eb_stripe_imbalance(bool self_mode, uint64_t n_cols, uint64_t r0, uint64_t r1, uint32_t xcd_shift)
{
    const uint64_t n_xcd = 1ull << xcd_shift, w = eb_stripe_width(n_cols, xcd_shift);
    uint64_t heaviest = 0, total = 0;
    for (uint64_t x = 0; x < n_xcd; ++x) {
        uint64_t own = 0;
        for (int h = 0; h < 2; ++h) {
            const uint64_t s = h == 0 ? x : 2u * n_xcd - 1u - x;
            const uint64_t a = s * w < n_cols ? s * w : n_cols, b = (s + 1u) * w < n_cols ? (s + 1u) * w : n_cols;
            own += eb_stripe_pairs_before(self_mode, r0, r1, b) - eb_stripe_pairs_before(self_mode, r0, r1, a);
        }
        total += own;
        if (own > heaviest) heaviest = own;
    }
    return total == 0 ? 1.0 : (double)heaviest * (double)n_xcd / (double)total;
}

// Forward: sets stripe_w and stripe_rp (row pairs of the launch) -> workgroups of the launch, the same number on every XCD.
template <class G>
SKL_STRIPE_FN uint64_t plan_eb_stripes(G &g)
{
    g.stripe_w = eb_stripe_width(g.nB_cols, g.xcd_shift);
    g.stripe_rp = (g.row_end - g.row_begin + 1u) / 2u;
    return ((uint64_t)g.stripe_rp * (g.stripe_w / 64u)) << g.xcd_shift;
}

// does the 64-column block that starts at column c hold a pair of rows i0, i0 + 1?  (i0 < row_end; self mode: j > i)
template <class G>
SKL_STRIPE_FN bool eb_stripe_block_live(const G &g, uint32_t i0, uint32_t c)
{
    if (c >= g.nB_cols) return false;
    const uint32_t last = c + 63u < g.nB_cols ? c + 63u : g.nB_cols - 1u;
    return !g.self_mode || last > i0;
}

// Inverse: what workgroup `wg` of the launch covers.  none: no pair (a slot past the last row pair, blocks left of the diagonal
// or past the last column); i0: its first row; c[h]: first column of its block of stripe x (h = 0) and 2 X - 1 - x (h = 1).
struct EbStripeWg {
    bool none;
    uint32_t xcd, i0, c[2];
};
template <class G>
SKL_STRIPE_FN EbStripeWg eb_stripe_wg(const G &g, uint32_t wg)
{
    EbStripeWg w;
    const uint32_t n_xcd = 1u << g.xcd_shift, blocks = g.stripe_w / 64u;
    w.xcd = wg & (n_xcd - 1u);
    const uint32_t slot = wg >> g.xcd_shift;
    const uint32_t rp = slot / blocks, cb = slot - rp * blocks;
    w.i0 = g.row_begin + 2u * rp;
    w.c[0] = w.xcd * g.stripe_w + cb * 64u;
    w.c[1] = (2u * n_xcd - 1u - w.xcd) * g.stripe_w + cb * 64u;
    w.none = rp >= g.stripe_rp || !(eb_stripe_block_live(g, w.i0, w.c[0]) || eb_stripe_block_live(g, w.i0, w.c[1]));
    return w;
}

// ... and thread `tid` (0 ... 255) of it: its (i, j); false: no pair of the launch
template <class G>
SKL_STRIPE_FN bool eb_stripe_pair(const G &g, const EbStripeWg &w, uint32_t tid, uint32_t &i, uint32_t &j)
{
    const uint32_t wave = tid >> 6;
    i = w.i0 + (wave & 1u);
    j = ((wave >> 1) != 0u ? w.c[1] : w.c[0]) + (tid & 63u);   // (constant indices: the struct stays in registers)
    return i < g.row_end && j < g.nB_cols && (!g.self_mode || j > i);
}

}  // namespace skl
