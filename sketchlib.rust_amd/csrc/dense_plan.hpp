// dense_plan.hpp -- HOW a dense distance call is launched, as data computed by pure functions.
//
// capi.cpp dense_band() fills a DenseCall from the slabs, the context and the early-break decision, asks plan_row_bands()
// where to cut the call and plan_counts_launch() what each band launches, and executes the answer.  Nothing here touches a
// device: no HIP header, plain C++17 (tests/native/dense_plan_check.cpp builds it with the host compiler alone).
// The row bands are planned from the whole call, each band's launch from the band's own rows.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "knobs.hpp"

namespace skl {

// = MODE_COUNTS / MODE_JACCARD / MODE_COREACC and KSLICE_MAX_U16_CHUNKS of kernels.h (capi.cpp asserts they agree)
constexpr int PLAN_MODE_COUNTS = 0, PLAN_MODE_JACCARD = 1, PLAN_MODE_COREACC = 2;
constexpr uint32_t PLAN_MAX_U16_CHUNKS = 1023;   // sketches beyond it (65 535 bins): k-sliced forms only, u32 counts

// Launch-size rule shared with dispatch_pair_kernel: core/acc launches below this many pairs
// run k-sliced (counts + epilogue kernel), larger ones as one fused kernel.
constexpr long long SLICED_MAX_PAIRS = 32ll << 20;   // n ~ 8000 all-vs-all: equal there (scripts/ab_sweep.py)
constexpr size_t COUNTS_SCRATCH_MAX = 4ull << 30;    // bytes of bin-match counts one unfused core/accessory launch may park in HBM

// A sketch of ss64 chunks cut into at most `wanted` chunk slices of whole stages: *chunks per slice (a multiple of 8, the
// last slice shorter) -> number of slices that hold something (1: the sketch is too short to cut)
inline uint32_t slice_plan(uint32_t ss64, uint32_t wanted, uint32_t *chunks)
{
    if (wanted < 2u || ss64 < 16u) {
        *chunks = 0;
        return 1u;
    }
    const uint32_t per = ((ss64 + wanted - 1u) / wanted + 7u) / 8u * 8u;
    *chunks = per;
    return (ss64 + per - 1u) / per;
}

inline uint64_t cond_index(uint64_t i, uint64_t j, uint64_t n)
{
    return n * i - ((i * (i + 1)) >> 1) + j - 1 - i;  // distance_matrix.rs:11-14
}

// Number of pairs in rows [r0, r1) of the condensed triangle of n samples.
inline uint64_t self_rows_pairs(uint64_t r0, uint64_t r1, uint64_t n)
{
    if (n < 2) return 0;
    r1 = std::min<uint64_t>(r1, n - 1);
    if (r1 <= r0) return 0;
    auto upto = [n](uint64_t r) { return r * n - r * (r + 1) / 2; };  // pairs with i < r
    return upto(r1) - upto(r0);
}

// Everything the launch rules read about one dense call.
struct DenseCall {
    int mode = PLAN_MODE_COREACC;
    bool self_mode = true;
    uint64_t n_cols = 0, r0 = 0, r1 = 0;   // rows [r0, r1) against n_cols columns (self mode: the condensed triangle of n_cols)
    uint32_t nk = 0, ss64 = 0;
    bool has_comp = false;                 // both slabs carry a completeness vector ...
    bool comp_unit = false;                // ... and every value of both is finite and in (0, 1]
    uint32_t min_alive = 0xFFFFFFFFu;      // of the row slab (set with its ln J table: the caller ensures the table first)
    int n_cu = 256;
    int forced_kernel = 0;                 // A/B build: SKL_KERNEL; product library: always 0
    bool fused_coreacc_ok = true;          // the fused all-k kernel takes this slab (k-mer lengths, bins)
    Knobs knobs;
    // the early-break decision for the slab pair (EbPlan), as far as the rules read it
    bool eb_plan = false;                  // false: no plan (not applicable, switched off, another kernel forced)
    int eb_lengths = 0;
    bool eb_mixed = false;
    double eb_alive_share = 0.0;

    uint64_t pairs(uint64_t b0, uint64_t b1) const { return self_mode ? self_rows_pairs(b0, b1, n_cols) : (b1 - b0) * n_cols; }
    uint64_t out_base(uint64_t b0) const { return self_mode ? cond_index(b0, b0 + 1, n_cols) : b0 * n_cols; }   // first pair of row b0
};

inline bool coreacc_runs_sliced(const DenseCall &c, uint64_t pairs)
{
    if (c.forced_kernel != 0 && c.forced_kernel != 4) return false;   // another kernel forced: never slice
    if (c.ss64 > PLAN_MAX_U16_CHUNKS) return true;   // beyond 65 535 bins the fused form's u16 fields do not hold a count: always counts + epilogue
    const long long limit = c.knobs.sliced_max_pairs >= 0 ? c.knobs.sliced_max_pairs : SLICED_MAX_PAIRS;
    return pairs < (uint64_t)limit;
}

// k-sliced core/accessory launches: into how many chunk slices to cut each k-mer length (the kernel
// then runs one workgroup per (tile, k, slice) and the epilogue sums the partial counts).  Default: 1.
// Measured on MI355X (profiles/r02_k_slices_experiment.txt): at BASELINE's 1 000 genomes -- 1 400
// whole-k workgroups on 1 024 resident slots, 1.37 rounds that cost 2 -- 2 slices keep every SIMD at 4
// waves for 100 of 163 us instead of 60 of 157 us, but each workgroup pays its fixed 7 + 2 us (first
// row DMA under load, reduction and stores) on half the work, and the launch ends at the same time
// (0.1601 vs 0.1600 ms per step); 4 slices are 3 % slower, and from n = 1 400 up slices only cost.
// SKL_K_SLICES forces a value (tests keep the sliced form bit-exact; A/B runs).
inline uint32_t choose_k_slices(const Knobs &knobs, uint32_t ss64, uint32_t *chunks)
{
    const uint32_t S = knobs.k_slices > 0 ? std::min(8u, (uint32_t)knobs.k_slices) : 1u;
    return slice_plan(ss64, S, chunks);   // (slices that hold something: a short sketch gets fewer)
}

// A launch with fewer (tile, k) units than resident workgroup slots cannot fill the chip with one
// workgroup per unit: most SIMDs hold 0-2 waves and the launch takes the time of ONE unit at a
// lone wave's issue rate whatever its size (0.055-0.064 ms from 100 to 500 genomes).  Such launches are
// cut into tail_slices chunk slices per unit -- and so is the last, partial round of any launch
// SKL_TAIL_MAX_PCT lets through (default 90: launches of up to 0.9 estimated rounds, where the
// whole launch is that partial round; the partial round of a longer launch gains nothing,
// profiles/r02_ab_tail_slices.jsonl).  Slice 0 of a unit stores, the others add into a second
// plane that is zero on entry and re-zeroed by the epilogue.
// A single-k launch smaller than the chip has the same problem (one workgroup per tile on a quarter of the SIMDs, each wave
// at its own issue interval: 0.058 ms from 200 to 1 000 genomes) and takes the same cure with `evals` = its pairs.
struct TailSlicing {
    uint32_t slices = 1, chunks = 0;   // what the sketch can be cut into (slice_plan)
    bool tail = false;                 // ... and whether this launch is
};
// evals: pair x k-mer-length evaluations of the launch; allowed: the launch is of a form that can be tail-sliced at all
inline TailSlicing tail_slicing(const DenseCall &c, uint64_t evals, bool allowed)
{
    TailSlicing t;
    const uint64_t est_units = evals / 2048;
    const uint64_t slots = 4ull * (uint64_t)c.n_cu;
    // (launches of less than 1/16 round -- ~200 genomes -- are cut twice as fine when the sketch allows it)
    // (round 4: any sketch size is cut -- slices of whole stages, the last one shorter, slice_plan() -- e.g. the 157
    // chunks of `-s 10000`; and launches over sketches beyond 65 535 bins slice their last round however many rounds
    // they have: a unit of 1 563+ chunks dwarfs the fixed cost of a workgroup)
    const bool big_sketch = c.ss64 > PLAN_MAX_U16_CHUNKS;
    const uint32_t wanted = c.knobs.tail_slices == 4 && est_units * 16 <= slots && c.ss64 >= 64 ? 8u : (uint32_t)c.knobs.tail_slices;
    t.slices = slice_plan(c.ss64, wanted, &t.chunks);
    t.tail = allowed && t.slices > 1u && c.forced_kernel == 0 &&
             ((big_sketch && est_units <= 16 * slots) || est_units * 100 <= (uint64_t)std::max(0ll, c.knobs.tail_max_pct) * slots);
    return t;
}

// What a core/accessory band counts, before anything about slices: shared by the band cut and the band's launch.
struct CountsBasics {
    bool mixed = false;      // the early break decided block by block
    bool early = false;      // early break: pooled (`lengths` of nk counted) or block by block
    bool sliced = false;     // (tile, k) workgroups into a k-major scratch
    bool unfused = false;    // counts + epilogue kernel (false: one launch of the mode's own kernel)
    uint32_t lengths = 0;    // k-mer lengths the pair kernel counts (block by block: planes)
    bool cnt_u16 = false;    // the counts may be parked as u16 (a launch with chunk slices still keeps u32)
    bool blocked = false;    // the early break's epilogue walks the pairs in blocks kept on one XCD each
    bool lean_like = false;  // the lean epilogue kernel takes the launch
};
inline CountsBasics counts_basics(const DenseCall &c, uint64_t pairs)
{
    CountsBasics b;
    if (c.mode != PLAN_MODE_COREACC) return b;
    b.mixed = c.eb_plan && c.eb_mixed;
    const int eb_lengths = c.eb_plan && !b.mixed ? c.eb_lengths : 0;
    b.early = eb_lengths > 0 || b.mixed;
    // Small core/acc launches run as (tile, k) workgroups producing counts + the epilogue
    // kernel (pair_kslice.hip): 5x the workgroups of the fused kernel and two columns per lane.
    // (with the early break every launch takes the counts + epilogue form, whatever its size: three of the k-mer lengths,
    // 12 bytes of counts per pair through HBM -- nothing beside the two lengths not walked)
    b.sliced = coreacc_runs_sliced(c, pairs) || b.early;
    b.unfused = b.sliced || !c.fused_coreacc_ok;
    b.lengths = eb_lengths > 0 ? (uint32_t)eb_lengths : c.nk;
    // U16 COUNTS (round 6): sketches of up to 1 023 chunks count at most 65 472 bins per length, so a launch without
    // chunk slices (no plane to add into) parks its counts as u16: half the scratch traffic of the stream
    const bool tiny = pairs * b.lengths < 2ull * 4ull * (uint64_t)c.n_cu * 2048ull;   // (launches that may be tail-sliced keep u32: slices ADD into a plane)
    b.cnt_u16 = b.sliced && c.ss64 <= PLAN_MAX_U16_CHUNKS && !tiny && c.knobs.k_slices <= 1 && c.knobs.counts_u16 &&
                !c.knobs.fuse_epilogue && !c.knobs.epilogue_r5;   // (the A/B build's older epilogues read u32)
    // BLOCKED EPILOGUE ORDER (epilogue.hip): the early break's epilogue walks the pairs in blocks of 1 024 rows x 256 columns, each
    // block on one XCD, whose L2 then holds the block's 256 column slices while its rows pass -- instead of the launch's flat order
    // (a row after the other, all its columns), in which a slice's next reader comes a whole row later and every completion is a
    // gather from the Infinity Cache or, once the slices of one length outgrow it (cfg 3: 717 MB), from HBM.  Pays where many
    // pairs stay in the running and the launch is large: at 4.9 % alive n = 12 000 / 16 000 / 24 000 / 60 000 / 100 000:
    // 10.3 -> 9.9, 18.3 -> 17.2, 41.0 -> 38.0, 266 -> 234, 827 -> 642 ms; at 1.4 % alive (2 048 bins) +1 %: not taken.
    if (b.early) {
        b.blocked = c.knobs.eb_blocked >= 0 ? c.knobs.eb_blocked != 0   // (A/B build: forced)
                                            : c.eb_plan && c.eb_alive_share >= 0.03 && pairs >= (48ull << 20) && c.ss64 <= PLAN_MAX_U16_CHUNKS;
    }
    b.lean_like = !b.mixed && (!c.has_comp || c.comp_unit) && c.min_alive != 0xFFFFFFFFu && b.lengths >= 2 && b.lengths <= 4;
    return b;
}

// Rows [r0, r1) cut into n_bands bands of (nearly) equal pair count: cuts[0] = r0 < ... < cuts.back() = r1, every band at
// least one row (so there may be fewer bands than asked for).
inline std::vector<uint64_t> cut_row_bands(const DenseCall &c, uint64_t n_bands)
{
    const uint64_t r0 = c.r0, r1 = c.r1, pairs = c.pairs(r0, r1);
    std::vector<uint64_t> cuts(1, r0);
    for (uint64_t b = 1; b < n_bands; ++b) {
        const uint64_t target = pairs * b / n_bands;   // pairs before the cut
        uint64_t cut;
        if (c.self_mode) {   // the first row whose predecessors hold at least `target` pairs
            uint64_t lo = cuts.back() + 1, hi = r1 - 1;
            while (lo < hi) {
                const uint64_t m = (lo + hi) / 2;
                if (self_rows_pairs(r0, m, c.n_cols) < target) lo = m + 1; else hi = m;
            }
            cut = lo;
        } else {
            cut = r0 + (target + c.n_cols - 1) / c.n_cols;
        }
        cut = std::min<uint64_t>(std::max<uint64_t>(cut, cuts.back() + 1), r1 - 1);
        if (cut > cuts.back()) cuts.push_back(cut);
    }
    cuts.push_back(r1);
    return cuts;
}

// BAND PIPELINE (round 6).  The counts scratch is bounded, and a call whose counts do not fit is computed in row bands of
// equal pair count, each into its slice of the destination (without the early break only sketches beyond 65 535 bins or
// more than 6 k-mer lengths come here with that many pairs).  From 64 Mi pairs on the bands are also what hides the epilogue:
// band i's epilogue (+ completion of the pairs still in the running) is memory-bound, band i + 1's counts kernel is bound by the vector ALUs, so they
// run side by side -- counts kernels on the context's stream, epilogues on its second stream, two counts buffers.
// (the side-by-side run costs the counts kernel about what it hides of the epilogue -- an epilogue wave displaces a wave of the
// counts kernel, which fills the register file by itself -- and pays only where the epilogue is heavy: from ~3 % of the
// pairs still in the running.  n = 16 000 at 4.9 %: 18.5 against 19.4 ms; cfg 3 at 1.1 %: 782 against 748 ms.)
// Since the blocked epilogue order (counts_basics) covers that regime better -- n = 16 000: 17.2 ms blocked, 18.3-18.8
// piped; cfg 3 at two lengths: 642 blocked, 775 piped -- the pipeline was off unless asked for (A/B build,
// SKL_EB_PIPELINE=1; tests/test_gpu_early_break_r6.py keeps it exact).
// ROUND 6, LATE: with the lean epilogue (58 VGPRs, 8 waves per SIMD, a third of the instructions) the side-by-side run pays
// where it did not: 300 000 x 10 000 at 1.4 % still in the running 161.6 -> 154.0 ms, n = 30 000 at 2 048 bins 23.9 -> 23.2
// (profiles/r06_epilogue_lean.md) -- on by itself wherever that kernel runs in the flat order.
// (together with the blocked order it pays for the largest calls only: cfg 3 586 -> 575 ms, n = 40 000 95.4 -> 94.7, but
// n = 16 000 in 4 bands 15.5 -> 18.0: from 2^30 pairs)
struct RowBands {
    std::vector<uint64_t> cuts;   // band b: rows [cuts[b], cuts[b + 1]); two entries: the call is not cut
    bool overlap = false;         // band i's epilogue on the second stream, beside band i + 1's counts kernel
};
inline RowBands plan_row_bands(const DenseCall &c)
{
    RowBands out;
    out.cuts = {c.r0, c.r1};
    const uint64_t pairs = c.pairs(c.r0, c.r1);
    const CountsBasics b = counts_basics(c, pairs);
    if (!b.unfused || c.r1 - c.r0 <= 1) return out;
    bool piping = false;
    if (b.early) {
        const int pk = c.knobs.eb_pipeline;
        if (pk == 1) piping = !b.blocked && (b.mixed || (c.eb_plan && c.eb_alive_share >= 0.03) || c.knobs.early_break >= 2);
        else if (pk == 2) piping = b.lean_like;
        else if (pk == -1) piping = b.lean_like && (!b.blocked || pairs >= (1ull << 30));
    }
    const size_t cnt_bytes = b.cnt_u16 ? sizeof(uint16_t) : sizeof(uint32_t);
    if (!(pairs * b.lengths * cnt_bytes > COUNTS_SCRATCH_MAX || (piping && pairs >= (uint64_t)c.knobs.eb_pipeline_min))) return out;
    const uint64_t fit = std::max<uint64_t>(1, COUNTS_SCRATCH_MAX / (b.lengths * cnt_bytes));
    const uint64_t want = piping ? std::max<uint64_t>((uint64_t)c.knobs.eb_pipeline_min / 2, pairs / 8) : fit;
    const uint64_t n_bands = (pairs + std::min(fit, want) - 1) / std::min(fit, want);
    out.cuts = cut_row_bands(c, n_bands);
    out.overlap = piping && out.cuts.size() > 2;
    return out;
}

enum DenseForm : int {
    FORM_DIRECT = 0,           // one launch of the mode's own kernel: fused all-k core/accessory, single k, bin-match counts
    FORM_COUNTS_EPILOGUE = 1,  // core/accessory: counts into scratch, then the epilogue kernel
    FORM_SINGLE_K_TAIL = 2,    // single k, smaller than the chip: tail-sliced counts, then the epilogue turns them into the f32 output
};

// The launch of one band (or of the uncut call).
struct CountsLaunch {
    DenseForm form = FORM_DIRECT;
    uint64_t pairs = 0;
    // the two counts forms
    bool early = false, mixed = false;     // early break: at all / block by block
    uint32_t lengths = 0;                  // k-mer lengths counted
    bool sliced = false;                   // k-major scratch, (tile, k[, chunk slice]) workgroups
    bool cnt_u16 = false;                  // record width of the counts
    uint32_t k_slices = 1;                 // chunk slices per k-mer length (SKL_K_SLICES), each into a plane of its own
    bool tail = false;                     // the last, partial round of workgroups in `tail_slices` chunk slices of ...
    uint32_t tail_slices = 0;
    uint32_t slice_chunks = 0;             // ... this many chunks (or: chunks per k slice)
    bool mid_band = false;                 // 32-row tiles with the last round cut in 2
    bool two_planes = false;               // tail slices add into plane 1
    uint32_t planes = 1;
    size_t plane_bytes = 0;                // pairs x lengths x record width
    // the early break's epilogue
    bool blocked = false;                  // order: in blocks kept on one XCD each (false: flat)
    bool lean = true, ahead = true, lds_rows = false, comp_lean = false;
    // A/B build: the plain k-sliced launch may finish its pairs itself (the executor still asks the kernel whether it takes the
    // launch) / round 5's epilogue is asked for
    bool fuse_epilogue = false, epilogue_r5 = false;
};

inline CountsLaunch plan_counts_launch(const DenseCall &c, uint64_t r0, uint64_t r1)
{
    CountsLaunch L;
    L.pairs = c.pairs(r0, r1);
    const CountsBasics b = counts_basics(c, L.pairs);
    if (!b.unfused) {
        if (c.mode != PLAN_MODE_JACCARD) return L;
        const TailSlicing t = tail_slicing(c, L.pairs, true);
        if (!t.tail) return L;
        L.form = FORM_SINGLE_K_TAIL;
        L.lengths = 1;
        L.sliced = true;
        L.tail = L.two_planes = true;
        L.tail_slices = t.slices;
        L.slice_chunks = t.chunks;
        L.planes = 2;
        L.plane_bytes = L.pairs * sizeof(uint32_t);
        return L;
    }
    L.form = FORM_COUNTS_EPILOGUE;
    L.early = b.early;
    L.mixed = b.mixed;
    L.lengths = b.lengths;
    L.sliced = b.sliced;
    uint32_t k_chunks = 0;
    L.k_slices = b.sliced ? choose_k_slices(c.knobs, c.ss64, &k_chunks) : 1u;
    const uint64_t evals = L.pairs * b.lengths;
    const TailSlicing t = tail_slicing(c, evals, b.sliced && L.k_slices == 1u);
    L.tail = t.tail;
    L.tail_slices = t.slices;
    L.slice_chunks = t.chunks;
    // MID BAND (round 3): from half the 32-row threshold up to it (4-8 Mi pair x k evaluations: 1 300-1 790 genomes at
    // 5 k-mer lengths) the launch is a handful of rounds of workgroups whichever tile it takes, and its last, partial
    // round decides: 32 x 128 tiles with THAT round cut into 2 chunk slices are 0.7-4.6 % ahead of 16 x 128 tiles
    // there (profiles/r03_ab_mid_sizes.jsonl, r03_ab_mid_band.jsonl); plain 32-row tiles are not (+-4 %).  Above the
    // band plain 32-row tiles, below it 16-row tiles (cfg 2: 0.156 against 0.162 ms).
    const long long t32 = c.knobs.tile32_min;
    L.mid_band = c.knobs.mid_band && !t.tail && b.sliced && L.k_slices == 1u && t32 > 0 && t.slices > 1u &&
                 c.forced_kernel == 0 && c.ss64 >= 16 && evals * 2 >= (uint64_t)t32 && evals < (uint64_t)t32;
    if (L.mid_band) {
        L.tail = true;
        L.tail_slices = slice_plan(c.ss64, 2u, &L.slice_chunks);
    }
    if (!L.tail) {
        L.tail_slices = 0;
        L.slice_chunks = L.k_slices > 1u ? k_chunks : 0u;
    }
    L.two_planes = L.tail;
    L.cnt_u16 = b.cnt_u16 && !L.tail && L.k_slices == 1u;
    L.planes = std::max(L.two_planes ? 2u : 1u, L.k_slices);
    L.plane_bytes = L.pairs * b.lengths * (L.cnt_u16 ? sizeof(uint16_t) : sizeof(uint32_t));
    L.blocked = b.blocked;
    // (the workgroup's row slices in LDS pay from ~8 completions per workgroup of 256 pairs on: n = 16 000 at 4 096 bins, 4.9 %
    // still in the running: 18.0 against 18.7 ms; at 2 048 bins, 1.4 %: 30.8 against 27.3 -- profiles/r06_epilogue_forms.md)
    L.lds_rows = c.knobs.eb_lds_rows && c.eb_plan && c.eb_alive_share >= 0.03;
    L.ahead = c.knobs.eb_ahead;
    L.lean = c.knobs.eb_lean;
    L.comp_lean = c.has_comp && c.comp_unit;
    L.fuse_epilogue = b.sliced && !b.early && L.k_slices == 1u && !L.two_planes && c.knobs.fuse_epilogue && c.forced_kernel == 0 &&
                      c.ss64 <= PLAN_MAX_U16_CHUNKS;
    L.epilogue_r5 = c.knobs.epilogue_r5 && !b.mixed && !(b.early && (c.has_comp || c.ss64 > PLAN_MAX_U16_CHUNKS));
    return L;
}

}  // namespace skl
