// knn_plan.hpp -- HOW the kNN drivers cut and feed their bands, as data computed by pure functions.
//
// capi_knn.cpp fills a KnnRowsCall (one kNN call: band heights, symmetric or row by row, column panels) or a KnnCall (one call
// of the band driver: a whole-matrix symmetric self kNN, one band of one column window, one column panel of the row-by-row
// kNN), asks the functions below, and executes the answer: scratch of the planned sizes, then per band the planned view and
// the planned two merges in the planned order.  Nothing here touches a device: no HIP header, plain C++17
// (tests/native/knn_plan_check.cpp builds it with the host compiler alone).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "dense_plan.hpp"
#include "knobs.hpp"

namespace skl {

// = TOPK_LDS_MAX / REFHEAP_LDS_MAX of kernels.h (capi_knn.cpp asserts they agree)
constexpr uint32_t PLAN_TOPK_LDS_MAX = 2048, PLAN_REFHEAP_LDS_MAX = 2048;
constexpr size_t BAND_BYTES = 512ull << 20;          // scratch bound for host-destined / banded output
constexpr size_t KNN_SHARED_BUDGET = 32ull << 30;    // the multi-GPU drivers' fixed budget (knn_shared_band_rows)

// = topk_items_pitch() of kernels.h: next power of two >= knn (the bitonic sort's array)
inline uint64_t plan_items_pitch(uint64_t knn)
{
    uint64_t m = 1;
    while (m < knn) m <<= 1;
    return m;
}

// ---------------------------------------------------------------------------
// Band heights
// ---------------------------------------------------------------------------

// Bytes per pair and band buffer the symmetric drivers' budget counts: the record, and for core/accessory keys the share of
// the early break's two counts buffers (up to 4 lengths x 2 bytes each against four band buffers: + 4 bytes per buffer).
inline size_t coreacc_rec_with_counts(bool coreacc, size_t nk, bool fused_coreacc_ok)
{
    if (!coreacc) return sizeof(float);
    return 2 * sizeof(float) + (nk >= 3 && nk <= 8 && fused_coreacc_ok ? 4 : 0);
}

// Rows per band of the symmetric drivers: about 8 bands per participant (7/16 of the pair
// evaluations saved), each band at least 32 M pairs, four band buffers within `budget` bytes.
inline size_t symmetric_band_rows(size_t n, size_t rec, size_t budget, size_t participants)
{
    auto up16 = [](size_t x) { return (x + 15) / 16 * 16; };
    const size_t budget_rows = std::max<size_t>(16, budget / 4 / (n * rec) / 16 * 16);
    const size_t parts = std::max<size_t>(1, participants);
    return std::min(budget_rows, std::max(up16((n + 8 * parts - 1) / (8 * parts)), up16((32ull << 20) / n + 1)));
}

// The band height every participant of a multi-GPU symmetric kNN uses (skl_knn_band_rows): a fixed budget (no free-memory
// query): every participant must arrive at the same number.  `rec`: coreacc_rec_with_counts().
inline size_t knn_shared_band_rows(size_t n, size_t rec, const Knobs &knobs, size_t participants)
{
    if (knobs.knn_band_rows > 0) return std::min<size_t>(n, (size_t)knobs.knn_band_rows);   // test knob (the same for every participant)
    return std::min(n, symmetric_band_rows(n, rec, KNN_SHARED_BUDGET, participants));
}

// Symmetric self kNN (whole matrix in one call): band [b0, b1) is compared with the columns
// from b0 on only.  The pair kernel stores every record twice -- row-major for the rows of the
// band, and turned (pair_kslice.hip, out_t) as candidates of the rows below the band -- and
// both copies are merged into a running per-row top-k (topk_merge_kernel), so each (i, j) is
// evaluated once instead of twice (the reference evaluates both, mod.rs:148-171; distances are
// symmetric).  Same neighbours, same order as the row-by-row form.
inline bool knn_symmetric_ok(bool coreacc, bool fused_coreacc_ok, int forced_kernel)
{
    // (beyond 65 535 bins: single-k only -- the k-sliced form walks the k-mer length in segments, the fused
    // core/accessory form has no such walk)
    if (coreacc && !fused_coreacc_ok) return false;
    if (forced_kernel != 0 && forced_kernel != 4) return false;          // the turned store lives in pair_kslice.hip
    return true;
}

// Everything the height and panel rules read about one kNN call: rows [r0, r1) against n_cand candidates.
struct KnnRowsCall {
    size_t n_cand = 0, r0 = 0, r1 = 0, knn = 0;
    bool self_mode = false;          // rows and candidates are the same sample set
    bool coreacc = false, ref_ties = false;
    size_t nk = 0, ss64 = 0;         // of the row slab
    bool both_comp = false;          // rows AND candidates carry a completeness vector
    bool fused_coreacc_ok = true;
    int forced_kernel = 0;
    size_t free_bytes = 0;           // free device memory (0: unknown)
    Knobs knobs;

    size_t rec() const { return coreacc ? 2 * sizeof(float) : sizeof(float); }
    bool big_knn() const { return knn > (size_t)PLAN_TOPK_LDS_MAX; }
};

struct KnnRowsPlan {
    bool symmetric = false;   // every pair once (knn_self_symmetric); false: row by row (knn_rows_banded)
    size_t band_rows = 0;
    bool overlap = false;     // top-k of band i on the second stream, beside the pair kernel of band i + 1
};
inline KnnRowsPlan plan_knn_rows(const KnnRowsCall &c)
{
    KnnRowsPlan P;
    // (no upper bound on knn beyond the candidates there are, as in the reference, lib.rs:379-382 / mod.rs:325: up to
    // TOPK_LDS_MAX neighbours the lists live in LDS; more go through global memory, row by row)
    const bool big_knn = c.big_knn();
    const size_t rows = c.r1 - c.r0;
    // the key band lives only on the device: take up to a quarter of the free HBM (<= 8 GiB)
    // so that the row-wise top-k kernel has thousands of rows (= workgroups) per launch
    size_t band_bytes = BAND_BYTES;
    if (c.free_bytes) band_bytes = std::max(band_bytes, std::min<size_t>(c.free_bytes / 4, 8ull << 30));
    size_t band_rows = std::max<size_t>(1, band_bytes / 2 / (c.n_cand * c.rec()));   // two key bands
    const size_t forced_band_rows = (size_t)c.knobs.knn_band_rows;  // test knob: force several bands
    if (forced_band_rows) band_rows = forced_band_rows;
    band_rows = std::min(band_rows, rows);
    // The whole self matrix: evaluate each pair once (knn_self_symmetric) when that leaves bands
    // worth launching -- about 8 of them (7/16 of the pair evaluations saved), each at least 32 M
    // pairs, within four band buffers of up to half the free HBM (<= 32 GiB; core/accessory keys: <= 96 GiB) together.
    // (the reference's tie order depends on the ORDER candidates arrive in, ascending j for every row: the symmetric driver
    // delivers exactly that order, band by band, to a heap that lives in global memory between the bands; lists too long for
    // the LDS-resident running state go row by row)
    bool symmetric = c.self_mode && c.r0 == 0 && c.r1 == c.n_cand && knn_symmetric_ok(c.coreacc, c.fused_coreacc_ok, c.forced_kernel) &&
                     !big_knn && c.knobs.knn_symmetric;   // (SKL_KNN_SYMMETRIC=0: A/B against the row-by-row form)
    if (symmetric) {
        size_t budget = band_bytes;
        // (core/accessory keys -- no tile pruning, whose thresholds want short bands -- take taller bands: the bands' epilogue
        // finds a column group's slices in L2 for more rows, and there are fewer launches and heap replays: cfg 5 in
        // core/accessory mode, 704 / 1 408 / 2 048 / 2 816 / 4 096 rows: 25.1 / 24.7 / 24.6 / 24.6 / 24.6 s)
        const size_t budget_cap = c.coreacc ? 96ull << 30 : 32ull << 30;
        if (c.free_bytes) budget = std::max(budget, std::min<size_t>(c.free_bytes / 2, budget_cap));
        const size_t want = forced_band_rows ? forced_band_rows
                                             : symmetric_band_rows(c.n_cand, coreacc_rec_with_counts(c.coreacc, c.nk, c.fused_coreacc_ok), budget, 1);
        if (want >= c.n_cand) symmetric = false;
        else band_rows = want;
    }
    if (!symmetric && (big_knn || c.ref_ties)) {
        // per-row working arrays in global memory (knn beyond the LDS forms): keep them within 1 GiB
        const size_t per_row = big_knn ? std::max<size_t>((size_t)plan_items_pitch(c.knn) * sizeof(uint64_t), 3 * (c.knn + 1) * sizeof(float)) : 0;
        if (per_row) band_rows = std::max<size_t>(1, std::min<size_t>(band_rows, (size_t)(1ull << 30) / per_row));
    }
    P.symmetric = symmetric;
    P.band_rows = band_rows;
    P.overlap = c.knobs.knn_overlap && band_rows < rows;
    return P;
}

// COLUMN PANELS (round 5): a row-by-row kNN over many candidates -- cross kNN against a large reference set, a row range of
// the self kNN -- is fed its candidates in ascending panels of columns instead of all at once: the rows' lists tighten
// from panel to panel, and from the second panel on the pair kernel leaves the tiles whose pairs are beyond their ROW's
// bound (tile pruning, as in the symmetric driver; the columns have no lists here).  Same lists in either tie rule: a
// row still meets its candidates in ascending id.  Single-k keys without a completeness correction, lists that fit the
// LDS forms, at least 4 panels of 32 Ki columns and launches large enough for the prunable 32 x 128 tiles.
struct KnnPanels {
    size_t panel = 0;         // columns per panel
    bool eligible = false;
    size_t rows_per = 0;      // band height of the panel calls (eligible only)
};
// band_rows: the row-by-row height of plan_knn_rows()
inline KnnPanels plan_knn_panels(const KnnRowsCall &c, size_t band_rows)
{
    KnnPanels P;
    // (A/B build: SKL_KNN_PANEL forces a panel width -- and lifts the size conditions -- so that tests reach this path on
    // inputs small enough for the oracle)
    const size_t forced_panel = (size_t)std::max(0ll, c.knobs.knn_panel) / 128 * 128;
    P.panel = forced_panel ? forced_panel : std::max<size_t>(32768, (c.n_cand / 8 + 127) / 128 * 128);
    P.eligible = c.knobs.knn_prune && c.knobs.knn_row_flags && !c.coreacc && !c.both_comp &&
                 c.ss64 <= (size_t)PLAN_MAX_U16_CHUNKS && !c.big_knn() && c.knn <= (size_t)PLAN_REFHEAP_LDS_MAX && c.forced_kernel == 0 &&
                 (forced_panel ? c.n_cand > P.panel : (c.n_cand >= 4 * P.panel && (c.r1 - c.r0) * P.panel >= (size_t)(16u << 20)));
    if (!P.eligible) return P;
    // bands of rows whose records of one panel fit a quarter of the budget the caller sized `band_rows` for
    P.rows_per = std::max<size_t>(32, std::min<size_t>(c.r1 - c.r0, band_rows * c.n_cand / P.panel) / 32 * 32);
    if (c.knobs.knn_band_rows) P.rows_per = std::max<size_t>(1, (size_t)c.knobs.knn_band_rows);   // (test knob)
    P.rows_per = std::min(P.rows_per, (size_t)1 << 20);
    return P;
}

// ---------------------------------------------------------------------------
// One call of the band driver
// ---------------------------------------------------------------------------

// The bands of a call (ascending indices; band b = rows [b*band_rows, (b+1)*band_rows)) are merged into the running states
// of all n rows.
// SYMMETRIC: the whole-matrix self kNN, or a dealt share of its bands (skl_self_dists_knn_partial): all columns.
// COLUMN WINDOW (win_lo, win_hi): only the pairs whose COLUMN sample lies in [win_lo, win_hi) are
// evaluated -- band rows against columns [max(b0, win_lo), win_hi), turned copies to the rows [max(b1, win_lo), win_hi) -- which
// is one participant's share of the reference-order pipeline over several devices (skl_self_dists_knn_window).
// CROSS PANEL: the rows of one slab against the columns [win_lo, win_hi) of another (or of the same one, row
// ranges of the self kNN: self_rows), no symmetry, nothing turned -- one COLUMN PANEL of the row-by-row kNN.  The drivers
// call it panel after panel, ascending, so a row meets its candidates in ascending id, its list tightens from panel to panel,
// and from the second panel on the pair kernel prunes against the rows' bounds (the columns have no lists: bound 0).
enum KnnForm : int { KNN_SYMMETRIC = 0, KNN_WINDOW = 1, KNN_CROSS_PANEL = 2 };

// Everything the rules read about one call of the band driver.
struct KnnCall {
    KnnForm form = KNN_SYMMETRIC;
    size_t n_rows = 0, n_cols = 0;         // samples of the row slab / of the column slab (the same but for a cross panel)
    size_t band_rows = 0, knn = 0;
    size_t win_lo = 0, win_hi = 0;         // columns of the call (symmetric: [0, n_cols))
    size_t row_lo = 0, row_hi = 0;         // rows of the call (bands are clipped to them; all but a cross panel: [0, n_rows))
    bool self_rows = false;                // cross panel: rows and columns are the same sample set: a row is not its own candidate
    bool coreacc = false;
    bool ref = false;                      // the reference's tie order: heaps replayed (a row's candidates arrive in ascending id
                                           // over the bands -- turned from the bands above its own, then its own band's columns)
    bool overlap = false;                  // two sets of band buffers, the merges on the second stream
    size_t nk = 0, ss64 = 0;               // of the row slab
    bool has_comp = false;                 // the row slab carries a completeness vector
    bool fused_coreacc_ok = true;
    int forced_kernel = 0;
    // (column window, one band per call: every list the band's TURNED copy reaches already holds knn candidates, as from a
    // whole-matrix call's second band on: the early break of the core/accessory keys may start with the call's first band.
    // The band's own rows are not covered -- under accept logs they may start empty: capi_knn.cpp knn_window_impl)
    bool lists_hold_knn = false;
    size_t n_bands = 0;                    // bands the call was handed
    Knobs knobs;

    bool cross() const { return form == KNN_CROSS_PANEL; }
    size_t rec() const { return coreacc ? 2 * sizeof(float) : sizeof(float); }
};

// The call's geometry and the bytes of every scratch buffer it asks for: each holds the largest view any band of the call
// can have.  With `overlap` the flag / bit arrays are two halves, the second one `*_half` words behind the first.
struct KnnCallPlan {
    size_t t_stride = 0;      // rows of a turned record line: whole tiles of either height (TILE_ROWS_SMALL / TILE_ROWS_LARGE, dense_plan.hpp)
    size_t k_cols = 0;        // columns of a band's records (cross panel: the panel's)
    size_t bit_words = 0;     // words of a band row's marks (bit = 64-column block of the band's view)
    size_t tbit_words = 0;    // words of a column's marks in the turned band (bit = 32-row stretch; cross panel: nothing turned, 0)
    bool turned = false;      // the form stores turned copies at all
    bool prune = false;       // TILE PRUNING
    bool eb_may_ask = false;  // the EARLY BREAK's decision may be asked for (early_break_lengths)
    size_t key_band_bytes = 0, turned_band_bytes = 0;   // per buffer
    size_t flags_bytes = 0, row_bits_bytes = 0, turned_bits_bytes = 0 /* 0: not asked for */, prune_bounds_bytes = 0;
    size_t flags_half = 0, row_bits_half = 0, turned_bits_half = 0;
    size_t prune_cols_at = 0;   // word of the prune bounds where the COLUMNS' bounds start (symmetric forms: the rows' own, 0)
};
inline KnnCallPlan plan_knn_call(const KnnCall &c)
{
    KnnCallPlan P;
    const size_t n = c.n_cols, rec = c.rec();
    P.turned = !c.cross();
    P.t_stride = (c.band_rows + TILE_ROWS_LARGE - 1) / TILE_ROWS_LARGE * TILE_ROWS_LARGE;
    P.k_cols = c.cross() ? c.win_hi - c.win_lo / 64 * 64 : n;   // (= win_hi - the 64-column block holding win_lo: the panel's view)
    P.key_band_bytes = c.band_rows * P.k_cols * rec;
    P.turned_band_bytes = P.turned ? n * P.t_stride * rec : 0;
    // Row flags of the transposed band (one array per band buffer): the pair kernel marks the rows that
    // received a record below their knn-th best so far with the band's number, and the merge of the
    // transposed band (n - b1 workgroups reading band_rows records each: 2/3 of the merge time at cfg 5)
    // returns at once for the others.  The threshold the pair kernel compares with is read from the
    // running state while merges of earlier bands may still be updating it on the other stream: a
    // stale value is a higher one (a row's knn-th best only ever improves), so it flags too many rows,
    // never too few; ties never count (a band's sample ids are above every id a lower row holds).
    P.flags_bytes = 2 * n * sizeof(uint32_t);
    P.flags_half = c.overlap ? n : 0;
    // ... and for the band's own rows one bit per 64-column block (the merge of the band reads only the
    // marked stretches of a row): band_rows x ceil(columns / 2048) words per band buffer, behind the flags
    P.bit_words = (P.k_cols / 64 + 1 + 31) / 32;
    P.row_bits_bytes = 2 * c.band_rows * P.bit_words * sizeof(uint32_t);
    P.row_bits_half = c.overlap ? c.band_rows * P.bit_words : 0;
    // ... and for the turned band one bit per (column, 32-row stretch of the band), so that BOTH merges read marked stretches
    // only and a tile without a mark need not exist: TILE PRUNING (pair_prune.hpp).  Single-k keys are monotone in the
    // mismatch count, so before each band a small kernel turns every sample's current knn-th best into the mismatch count
    // beyond which a pair cannot enter its list, and the pair kernel leaves a tile once every pair of it is beyond both its
    // samples' bounds on the chunks walked so far.  The bounds come from the same (possibly stale, i.e. too high) thresholds
    // as the flags: a pair pruned now would be rejected by both lists whenever it arrived, so the lists -- ids AND order, in
    // either tie rule -- are those of the unpruned run.  Not with a completeness correction (the key then depends on the pair).
    P.tbit_words = c.cross() ? 0 : (P.t_stride / 32 + 31) / 32;   // (cross panel: the array is only a non-null mark)
    if (c.knobs.knn_row_flags) P.turned_bits_bytes = std::max<size_t>(2 * n * P.tbit_words, 64) * sizeof(uint32_t);
    P.turned_bits_half = c.overlap ? n * P.tbit_words : 0;
    P.prune = c.knobs.knn_prune && c.knobs.knn_row_flags && !c.coreacc && !c.has_comp && c.ss64 <= (size_t)PLAN_MAX_U16_CHUNKS;
    P.prune_cols_at = c.cross() ? c.n_rows + 64 : 0;
    P.prune_bounds_bytes = (c.n_rows + 64 + (c.cross() ? n + 64 : 0)) * sizeof(uint32_t);
    // EARLY BREAK (core/accessory keys; capi_eb.cpp early_break_lengths): from the call's second band on -- every list then holds
    // knn candidates, so a pair that left the reference's loop early, (1, 1), marks nothing -- the band is COUNTED at its first
    // eb_lengths k-mer lengths (k-sliced counts launch) and coreacc_epilogue_knn_kernel writes the records, the marks and the
    // turned copy (pre-filled with (1, 1)), completing the pairs still in the running.  Same records as the fused kernel's.
    P.eb_may_ask = c.coreacc && !c.cross() && c.fused_coreacc_ok && c.forced_kernel == 0 && c.knobs.knn_row_flags &&
                   (c.n_bands > 1 || c.lists_hold_knn);
    return P;
}

// Bytes of one early-break counts buffer: the largest view a band can have; u16 records (fused_coreacc_ok means at most
// 65 472 bins).
inline size_t knn_eb_counts_bytes(const KnnCall &c, int eb_lengths)
{
    return c.band_rows * c.n_cols * (size_t)eb_lengths * sizeof(uint16_t);
}

// One merge of a band's records into the running states, as plain data: rows [state_row_base, + rows) each take `cols`
// records, `stride` records apart, as candidates id_base + position.
struct KnnMerge {
    bool turned = false;          // reads the turned band (false: the key band)
    bool row_flags = false;       // only the rows the pair kernel flagged with the band's flag_value are fed
    uint32_t rows = 0, cols = 0;
    uint64_t stride = 0;
    uint32_t id_base = 0, skip_below = 0, state_row_base = 0, self_id_base = 0;
    uint32_t seg_shift = 0;       // positions per mark, log2
};

struct KnnBand {
    bool skip = true;             // no row of the call in the band, or the window lies left of it: nothing is launched
    size_t b0 = 0, b1 = 0;        // rows
    size_t c_first = 0;           // first candidate column of the band's own rows
    size_t t_first = 0;           // first row that receives the band turned (cross panel: none, win_hi)
    size_t col0 = 0;              // the view starts at the 64-column block holding c_first
    uint32_t nB = 0;              // columns of the view
    bool has_turned = false;
    uint32_t flag_value = 0;      // never 0, distinct per band of this call
    bool eb_band = false;         // counted at eb_lengths k-mer lengths, finished by the band's epilogue
    bool plain_marks_nothing = false;
    uint64_t tiles = 0;           // 32 x 128 tiles of the view (the pruning counters' denominator)
    KnnMerge merge[2];            // in launch order
};
// band: its index; it: its ordinal among the bands of this call that were not skipped
inline KnnBand plan_knn_band(const KnnCall &c, const KnnCallPlan &P, size_t band, size_t it, int eb_lengths)
{
    KnnBand B;
    B.b0 = std::max(band * c.band_rows, c.row_lo);
    B.b1 = std::min(std::min(c.n_rows, band * c.band_rows + c.band_rows), c.row_hi);
    if (B.b1 <= B.b0) return B;
    B.c_first = c.cross() ? c.win_lo : std::max(B.b0, c.win_lo);
    B.t_first = c.cross() ? c.win_hi : std::max(B.b1, c.win_lo);
    if (B.c_first >= c.win_hi) return B;               // the window lies left of this band: nothing of it here
    B.skip = false;
    // the band against the column view that starts at the 64-column block holding its first candidate column
    B.col0 = B.c_first / 64 * 64;
    B.nB = (uint32_t)(c.win_hi - B.col0);
    B.has_turned = B.t_first < c.win_hi;
    B.flag_value = (uint32_t)(it + 1);
    B.eb_band = eb_lengths > 0 && (it >= 1 || c.lists_hold_knn);
    // (bands ascend: the `it` bands before this one each gave band_rows candidates to every row the turned copy reaches,
    // and their merges run before this launch on the same stream)
    B.plain_marks_nothing = c.lists_hold_knn || it * c.band_rows >= c.knn;
    B.tiles = (uint64_t)((B.b1 - B.b0 + 31) / 32) * ((B.nB + 127) / 128);

    // rows of the band: columns [c_first, win_hi) minus themselves (the view's first c_first - col0 columns
    // reached them turned, from earlier bands, or belong to another window)
    KnnMerge own;
    own.rows = (uint32_t)(B.b1 - B.b0);
    own.cols = B.nB;
    own.stride = B.nB;
    own.id_base = (uint32_t)B.col0;
    own.skip_below = (uint32_t)B.c_first;
    own.state_row_base = (uint32_t)B.b0;
    own.self_id_base = (c.cross() && !c.self_rows) ? 0xFFFFFFFFu : (uint32_t)B.b0;
    own.seg_shift = c.ref ? 6 : 0;   // 64 positions per mark (topk_merge_kernel takes 0 as 6, and is handed 0)
    // rows below the band: the band's samples as their candidates (row r of this launch = sample t_first + r)
    KnnMerge turned;
    turned.turned = turned.row_flags = true;
    turned.rows = B.has_turned ? (uint32_t)(c.win_hi - B.t_first) : 0u;
    turned.cols = (uint32_t)(B.b1 - B.b0);
    turned.stride = P.t_stride;
    turned.id_base = (uint32_t)B.b0;
    turned.skip_below = 0;
    turned.self_id_base = turned.state_row_base = (uint32_t)B.t_first;
    turned.seg_shift = 5;
    // ORDER.  Reference ties (heaps replayed): rows below the band FIRST: for them the band's samples are the next candidates
    // in ascending id, and their own band comes later; then the band's own rows (columns [b0, n) minus themselves: everything
    // below b0 reached them turned, from the bands above).  Either way a row is fed ascending ids over the sequence of
    // launches.  Canonical ties (sorted running lists): the band's own rows first -- the two launches feed disjoint rows.
    B.merge[0] = c.ref ? turned : own;
    B.merge[1] = c.ref ? own : turned;
    return B;
}

}  // namespace skl
