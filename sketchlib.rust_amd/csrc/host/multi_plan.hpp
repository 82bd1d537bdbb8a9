// multi_plan.hpp -- how one call is shared among several devices of a process: the row and column partitions, the deal of the
// kNN row bands, which of the multi-device kNN forms to run and what follows when one gives up, and the sizes they move.
// Pure functions of plain values: no project header, no HIP, no C ABI call, no environment, no thread -- distances_multi.cpp
// decides with these on the calling thread and only then starts its workers; tests/native/multi_plan_check.cpp checks them on
// the CPU, against hand-derived values and against the Python drivers' statement of the same partitions (multi_gpu.py).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace skl_host {
namespace multi_plan {

// rows [0, n) of the condensed triangle split into `parts` bands of ~equal pair count
inline std::vector<size_t> self_row_bounds(size_t n, size_t parts)
{
    const size_t total = n * (n - 1) / 2;
    std::vector<size_t> b = {0};
    size_t row = 0, acc = 0;
    for (size_t w = 1; w < parts; ++w) {
        const size_t target = (total * w + parts - 1) / parts;
        while (row < n && acc < target) {
            acc += n - 1 - row;
            ++row;
        }
        b.push_back(row);
    }
    b.push_back(n);
    return b;
}

inline std::vector<size_t> even_bounds(size_t rows, size_t parts)
{
    std::vector<size_t> b;
    for (size_t w = 0; w <= parts; ++w) b.push_back(rows * w / parts);
    return b;
}

// Column windows [cut[d], cut[d + 1]) of the reference-order kNN forms: device d evaluates the pairs (i, j), i < j, whose column
// j lies in its window -- ~ (hi^2 - lo^2) / 2 of them, so the cuts lie at n * sqrt(d / W), equal pair counts, moved to band
// boundaries (a band's rows are then all inside a window or all outside it).
// multi_gpu.knn_window_cuts states the same plan for the Python drivers and differs in two places:
//   * a quotient of exactly x.5 rounds AWAY FROM ZERO here (std::llround) and to the even neighbour there (Python's round):
//     n = 5, band_rows = 1, W = 4 cuts at 3 here (5 * sqrt(1/4) = 2.5) and at 2 there;
//   * a cut that rounds past n is clamped to n here, and there to the last band boundary at or below n:
//     n = 47, band_rows = 16, W = 8 gives ..., 32, 47, 47, 47 here and ..., 32, 32, 32, 47 there.
// Both are valid and give the same lists: any ascending cuts on band boundaries share out every pair once, and a cut of n off
// a boundary only ever begins an EMPTY window [n, n) -- skl_self_dists_knn_window returns at once for col_lo == col_hi
// (capi_knn.cpp, "an empty window holds no pair"), before it asks that col_lo be a multiple of band_rows.  The window before
// it ends at n, which that check allows.
inline std::vector<size_t> knn_window_cuts(size_t n, size_t band_rows, size_t W)
{
    std::vector<size_t> cut = {0};
    for (size_t r = 1; r < W; ++r) {
        const size_t c = (size_t)std::llround((double)n * std::sqrt((double)r / (double)W) / (double)band_rows) * band_rows;
        cut.push_back(std::min(std::max(c, cut.back()), n));
    }
    cut.push_back(n);
    return cut;
}

// The row bands of device d, ascending, of the canonical-tie form: band b costs ~ n - b * band_rows, so the bands are dealt back
// and forth (0 .. W-1, W-1 .. 0, ...) and every device gets the same cost to first order (multi_gpu.knn_band_deal).
inline std::vector<uint32_t> knn_band_deal(size_t n_bands, size_t W, size_t d)
{
    std::vector<uint32_t> mine;
    for (size_t band = 0; band < n_bands; ++band) {
        const size_t lap = band / W, pos = band % W;
        if ((lap % 2 == 0 ? pos : W - 1 - pos) == d) mine.push_back((uint32_t)band);
    }
    return mine;
}

// Sizes.  An accept log holds, per row, up to knn_log_cap records of knn_log_record_width floats and as many ids; the logs of
// all W windows pass through host memory, rows [0, hi_d) of device d, which the budget bounds by n rows of one log.
inline size_t knn_log_cap(size_t knn) { return std::max<size_t>(64, 16 * knn); }
inline size_t knn_log_record_width(bool coreacc) { return coreacc ? 2 : 1; }
inline bool knn_logs_fit_host(size_t n, size_t knn, bool coreacc)
{
    return n * knn_log_cap(knn) * (knn_log_record_width(coreacc) + 1) * 4 <= (4ull << 30);
}
// a travelling heap row on the wire, in 32-bit words: keys, ids[, second values], length, threshold
inline size_t knn_heap_wire_words(size_t knn, bool coreacc) { return (coreacc ? 3 : 2) * knn + 2; }

// the running lists of every one-evaluation form live in LDS (TOPK_LDS_MAX = REFHEAP_LDS_MAX in the library)
constexpr size_t KNN_ONE_EVALUATION_MAX = 2048;

enum class KnnForm {
    Decoupled,    // reference ties: every device its column window against heaps it cleared itself, accept logs replayed per row shard
    Travelling,   // reference ties: heaps pass from device d to d + 1 band by band
    Dealt,        // canonical ties: row bands dealt over the devices, partial states merged per row shard
    RowShards,    // every pair twice, rows shared out evenly: has no precondition and cannot give up
};
enum class KnnGaveUp {
    NoForm,        // the library has no one-evaluation form for this configuration (SKL_ERR_INVALID_ARG at the first band)
    LogOverflow,   // a row's accept log took more than knn_log_cap records
};

// The form to try first.  Reference ties with knn beyond the LDS bound or fewer than two samples go straight to row shards:
// they are not offered the canonical form, whose merge would order equal keys differently.  One device shares nothing.
inline KnnForm first_knn_form(bool reference_ties, size_t knn, size_t n, size_t W, bool coreacc, bool decoupled_allowed)
{
    if (W < 2 || knn > KNN_ONE_EVALUATION_MAX) return KnnForm::RowShards;
    if (!reference_ties) return KnnForm::Dealt;
    if (n < 2) return KnnForm::RowShards;
    return decoupled_allowed && knn_logs_fit_host(n, knn, coreacc) ? KnnForm::Decoupled : KnnForm::Travelling;
}

// The form after `form` gave up for the reason `why`.  The decoupled windows hand over to the travelling heaps whatever the
// reason (those find out for themselves that there is no form); everything else ends in row shards.
inline KnnForm next_knn_form(KnnForm form, KnnGaveUp /*why*/)
{
    return form == KnnForm::Decoupled ? KnnForm::Travelling : KnnForm::RowShards;
}

}  // namespace multi_plan
}  // namespace skl_host
