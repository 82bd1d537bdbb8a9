// dense_plan.hpp -- HOW a dense distance call is launched, as data computed by pure functions.
//
// capi_dense.cpp dense_band() fills a DenseCall from the slabs, the context and the early-break decision, asks plan_row_bands()
// where to cut the call and plan_counts_launch() what each band launches, and executes the answer.  Nothing here touches a
// device: no HIP header, plain C++17 (tests/native/dense_plan_check.cpp builds it with the host compiler alone).
// The row bands are planned from the whole call, each band's launch from the band's own rows.
// Every launch of the pair kernel then asks plan_pair_shape() for its tile shape and form (capi_dense.cpp dispatch_pair_kernel), and
// a host-destined call is cut by plan_host_bands() (capi_dense.cpp dense_rows).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "eb_stripes.hpp"
#include "knobs.hpp"

namespace skl {

// = MODE_COUNTS / MODE_JACCARD / MODE_COREACC, KSLICE_MAX_U16_CHUNKS and KSLICE_SEG_CHUNKS of kernels.h (capi_dense.cpp asserts they agree)
constexpr int PLAN_MODE_COUNTS = 0, PLAN_MODE_JACCARD = 1, PLAN_MODE_COREACC = 2;
constexpr uint32_t PLAN_MAX_U16_CHUNKS = 1023;   // sketches beyond it (65 535 bins): k-sliced forms only, u32 counts
constexpr uint32_t PLAN_SEG_CHUNKS = 1016;       // ... walked in segments of this many chunks

// Launch-size rule: core/acc launches below this many pairs run k-sliced (counts + epilogue kernel), larger ones as one
// fused kernel; a launch that arrives at plan_pair_shape() as MODE_COUNTS with k_sliced set is one of the former.
constexpr long long SLICED_MAX_PAIRS = 32ll << 20;   // n ~ 8000 all-vs-all: equal there (scripts/ab_sweep.py)
constexpr uint64_t SMALL_LAUNCH_PAIRS = 8ull << 20;  // bin-match launches below this many pairs run one workgroup per (tile, k) whoever asks
constexpr uint64_t BLOCKED_MIN_PAIRS = 48ull << 20;  // pair spaces from which the early break's epilogue walks in blocks (counts_basics; eb_plan.hpp prices a completion by it)
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
                                            : c.eb_plan && c.eb_alive_share >= 0.03 && pairs >= BLOCKED_MIN_PAIRS && c.ss64 <= PLAN_MAX_U16_CHUNKS;
    }
    b.lean_like = !b.mixed && (!c.has_comp || c.comp_unit) && c.min_alive != 0xFFFFFFFFu && b.lengths >= 2 && b.lengths <= 4;
    return b;
}

// XCDs the device presents as one: an MI355X XCD has 32 CUs, so an unpartitioned (SPX) part shows 256 CUs = 8 XCDs, a CPX
// partition 32 CUs = 1.  The tile order deals workgroups to XCDs by blockIdx mod that number; SKL_XCDS forces it (tests).
inline uint32_t plan_xcd_shift(int n_cu, int knob_xcds)
{
    int x = knob_xcds > 0 ? knob_xcds : n_cu / 32;
    uint32_t shift = 0;
    while (shift < 3u && (2 << shift) <= x) ++shift;
    return shift;
}

// STRIPED EPILOGUE ORDER (eb_stripes.hpp): the early break's epilogue walks a SMALL launch in column stripes folded onto the
// XCDs, so that an XCD is asked for its two stripes' column slices only and serves its completions from its own L2 -- in
// the flat order every XCD is asked for every column slice of a length (cfg 2: 7 MB against a 4 MB L2).  Taken where the lean
// kernel takes the launch with its rows staged (`lds_rows`: from 3 % of the sampled pairs still in the running), the order
// is not the blocked one, there is more than one XCD, the two stripes' slices of one length are within STRIPES_L2_BYTES and
// the heaviest XCD holds at most STRIPES_MAX_IMBALANCE x the mean number of pairs.  SKL_EB_STRIPES=0 / 1: never / wherever the
// lean kernel stages its rows (tests).
// Measured (profiles/r08_cfg2_epilogue_stripes.md; Set U, 4 096 bins, 4.8 % still in the running, ms per call flat -> striped):
//   the bytes    n = 1 000 / 2 000 / 3 000 / 4 000 / 5 000 / 8 000 = 0.9 / 1.8 / 2.75 / 3.7 / 4.6 / 7.3 MB of slices per XCD and length:
//                0.0997 -> 0.0935, 0.328 -> 0.292, 0.692 -> 0.591, 1.186 -> 1.033, 1.84 -> 1.59, 4.6 -> 4.2: the order pays past the 4 MB
//                of an L2 too (an XCD still reads an eighth of the distinct bytes); 8 MiB is the largest size measured, and from
//                48 Mi pairs the blocked order takes over anyway
//   the balance  n = 2 000 / 1 900 / 1 800 / 1 500 = 1.05 / 1.16 / 1.29 / 1.86 x the mean: -11 %, -8 %, -6 %, +5 %: taken up to 1.3
constexpr uint64_t STRIPES_L2_BYTES = 8ull << 20;
constexpr double STRIPES_MAX_IMBALANCE = 1.3;
inline bool counts_striped(const DenseCall &c, const CountsBasics &b, bool lean, bool lds_rows, uint64_t r0, uint64_t r1)
{
    if (c.knobs.eb_stripes == 0 || !b.early || b.blocked || !b.lean_like || !lean || !lds_rows) return false;
    if (c.ss64 * 224ull > 16384ull) return false;   // (the two rows do not fit the LDS the launch may ask for: nothing is staged)
    if (c.knobs.eb_stripes > 0) return true;
    const uint32_t xs = plan_xcd_shift(c.n_cu, c.knobs.xcds);
    return xs > 0u && eb_stripe_slice_bytes(c.n_cols, xs, c.ss64) <= STRIPES_L2_BYTES &&
           eb_stripe_imbalance(c.self_mode, c.n_cols, r0, r1, xs) <= STRIPES_MAX_IMBALANCE;
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
    bool striped = false;                  // order: column stripes folded onto the XCDs (counts_striped)
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
    L.striped = counts_striped(c, b, L.lean, L.lds_rows, r0, r1);
    L.fuse_epilogue = b.sliced && !b.early && L.k_slices == 1u && !L.two_planes && c.knobs.fuse_epilogue && c.forced_kernel == 0 &&
                      c.ss64 <= PLAN_MAX_U16_CHUNKS;
    L.epilogue_r5 = c.knobs.epilogue_r5 && !b.mixed && !(b.early && (c.has_comp || c.ss64 > PLAN_MAX_U16_CHUNKS));
    return L;
}

// ONE LAUNCH OF THE PAIR KERNEL: its tile shape and form.  Product library: the chunk-split kernel (pair_kslice.hip: 16 x 128
// or 32 x 128 tiles, chunks split over the 4 waves, rows by LDS DMA; one workgroup per (tile, k) for small launches and for
// single-k Jaccard, all k + fused regression otherwise) and, for the launches it does not take, pair_ksplit.hip.  The A/B
// build adds the round-2/3 forms of the two tile shapes behind SKL_KSLICE_SHAPE and SKL_KERNEL=ksplit.
constexpr int TILE_ROWS_SMALL = 16, TILE_ROWS_LARGE = 32;   // the two tile heights (a turned kNN record line holds whole tiles of either: knn_plan.hpp)
struct PairLaunch {
    int mode = PLAN_MODE_COUNTS;
    bool self_mode = true;
    uint64_t rows = 0;          // rows of the launch
    uint32_t nB = 0, k_count = 0, ss64 = 0;
    bool k_sliced = false;      // the caller asks for one workgroup per (tile, k-mer length)
    bool mid_band = false;      // the mid-band rule (plan_counts_launch)
    uint32_t tail_slices = 0;
    bool xcd_interleave = false;   // the tiles are dealt to the XCDs in blocks of 32 (block-by-block early break)
    int n_cu = 256;
    uint32_t xcd_shift = 3;     // plan_xcd_shift()
    Knobs knobs;                // (kernel, kslice_shape, ksplit_rows, kslice_ablate: the forms the A/B build's switches force; the product library never sets them)
};
struct PairShape {
    int shape = 165, ksplit_rows = 8;   // chunk-split kernel: tile shape; pair_ksplit.hip: rows per tile
    int tile_rows = TILE_ROWS_SMALL;    // rows of the chunk-split kernel's tile
    bool sliced_launch = false;         // one workgroup per (tile, k-mer length)
    bool try_kslice = true;             // ask the chunk-split kernel first
    int ablate = 0;
    uint32_t wg_per_cu = 4, round_size = 0, tail_resident = 0;
    bool no_half_tiles = false;
    bool tile_cost_order = false;       // self mode: every XCD takes a share of the full tiles, then of the half tiles (work_map.hpp)
    // what the name needs besides
    int mode = PLAN_MODE_COUNTS;
    bool big_sketch = false;
    uint32_t tail_slices = 0;
};
// TILES DEALT BY COST (work_map.hpp).  A self-mode launch of 16 x 128 tiles walks half tiles -- 31 of cfg 2's 287 -- and a contiguous
// eighth of the tile numbering gives one XCD eight of them and another none: blocks of 64 columns walked per XCD 63 ... 72
// against a mean of 67.9 at n = 1 000, 1.27 x the mean at n = 700.  In the cost order every XCD takes its share of the full
// tiles and then its share of the half tiles (within one tile of each other in both), so that the XCDs carry the same cost and
// each ends on its cheapest workgroups.  The form: k-sliced MODE_COUNTS in self mode, half tiles walked, more than one XCD, not
// the XCD-interleaved order of block-by-block plans.  SKL_TILE_COST_ORDER = 0 / 1: never / wherever the form allows (tests);
// by rule: launches of up to TILE_COST_MAX_PAIRS pairs -- a few rounds of workgroups, where the last round's make-up and the
// XCDs' balance are a visible share of the launch (profiles/r09_cfg2_counts_order.md).
constexpr uint64_t TILE_COST_MAX_PAIRS = 2ull << 20;
inline bool tile_cost_order_rule(const PairLaunch &a, const PairShape &s, uint64_t pairs)
{
    const bool form = a.self_mode && a.mode == PLAN_MODE_COUNTS && s.sliced_launch && s.shape == 165 && !s.no_half_tiles && s.ablate == 0 &&
                      a.xcd_shift > 0u && !a.xcd_interleave && s.try_kslice && !a.knobs.fuse_epilogue;
    if (!form || a.knobs.tile_cost_order == 0) return false;
    return a.knobs.tile_cost_order > 0 || pairs <= TILE_COST_MAX_PAIRS;
}

inline PairShape plan_pair_shape(const PairLaunch &a)
{
    PairShape s;
    s.mode = a.mode;
    s.tail_slices = a.tail_slices;
    const uint32_t n_xcd = 1u << a.xcd_shift;
    const uint64_t pairs = a.self_mode ? a.rows * a.nB / 2 : a.rows * (uint64_t)a.nB;
    const bool small = pairs < SMALL_LAUNCH_PAIRS;
    // 165 = 16 x 128 tiles in the 128-register form (4 waves per SIMD): +3.5 % at n = 16 000 over the
    // 141-register form 162 (3 waves), equal at n = 1 000 (profiles/r02_ab_tight.jsonl)
    // 325 = 32 x 128 tiles (130-168 registers, 3 waves per SIMD) for launches of at least
    // tile32_min pair x k-mer-length evaluations (~4 096 units of 32 x 128): every column register is
    // used against 32 rows instead of 16, which halves the lane-slab traffic per pair -- HBM bytes per
    // launch at n = 16 000 fall from 59.5 GB to 32.0 GB and the kernel gains 1.5-6 %
    // (profiles/r02_tile32_*.md); smaller launches lose to the coarser tail (n = 1 000: +32 %).
    s.shape = 165;
    s.ksplit_rows = 8;   // 8 >= 4 rows from n = 1000 up once XCDs are balanced
    {
        const uint64_t k_walked = a.mode == PLAN_MODE_JACCARD ? 1u : a.k_count;
        if (a.knobs.tile32_min >= 0 && pairs * k_walked >= (uint64_t)a.knobs.tile32_min) s.shape = 325;
        if (a.mid_band) s.shape = 325;   // the mid-band rule (plan_counts_launch): 32-row tiles with the last round cut in 2
    }
    // what the A/B build's switches force (all 0 in the product library: nothing changes)
    if (a.knobs.kslice_shape) s.shape = a.knobs.kslice_shape;
    if (a.knobs.ksplit_rows) s.ksplit_rows = a.knobs.ksplit_rows;
    s.try_kslice = a.knobs.kernel != 3;
    s.ablate = a.knobs.kslice_ablate;
    s.tile_rows = s.shape > 1000 ? s.shape / 100 : s.shape / 10;
    s.no_half_tiles = !a.knobs.half_tiles;
    // workgroups resident per CU: 4 for every shipped form (the A/B build's 3-wave all-k 32-row form: 3)
    // (sketches beyond 65 535 bins: the k-sliced forms only -- they walk a k-mer length in segments, pair_kslice_walk.inc)
    s.big_sketch = a.ss64 > PLAN_MAX_U16_CHUNKS;
    // single-k Jaccard: the sliced and the all-k form are the same work, the sliced one
    // compiles to fewer registers; core/acc arrives here as MODE_COUNTS from dense_band when sliced
    s.sliced_launch = a.mode == PLAN_MODE_JACCARD || (a.mode == PLAN_MODE_COUNTS && (small || a.k_sliced || s.big_sketch));
    s.wg_per_cu = ((s.shape == 3255 && !s.sliced_launch) || (s.shape == 3254 && s.sliced_launch)) ? 3u : 4u;
    s.round_size = a.knobs.round_priority ? s.wg_per_cu * (uint32_t)a.n_cu / n_xcd : 0u;
    if (a.tail_slices > 1u) {
        // tail-sliced one-workgroup-per-unit launch: two planes whatever kernel ends up running (a
        // kernel without the slices leaves plane 1 as it found it: zero)
        s.tail_resident = s.wg_per_cu * (uint32_t)a.n_cu / n_xcd;
    }
    s.tile_cost_order = tile_cost_order_rule(a, s, pairs);
    return s;
}

// What skl_ctx_last_kernel() says of the launch; kslice_ok: the chunk-split kernel takes it (kslice_supported, pair_kslice.hip).
inline std::string pair_kernel_name(const PairShape &s, bool kslice_ok)
{
    static const char *mode_names[] = {"COUNTS", "JACCARD", "COREACC"};
    const std::string m = mode_names[s.mode];
    if (s.try_kslice && kslice_ok) {
        const int shape = s.shape;
        const bool sliced = s.sliced_launch;
        const int jl = (shape == 165 || shape == 325 || shape > 1000) ? 2 : shape % 10;
        const int rr = s.tile_rows;
        return "skl::pair_kernel_kslice<R=" + std::to_string(rr) + ", JL=" + std::to_string(jl) +
               ", " + m + (sliced ? ", k-sliced" : ", all k") + ((shape == 165 || shape == 325 || shape > 1000) ? ", tight" : "") + "> (" +
               std::to_string(rr) + "x" + std::to_string(jl * 64) + " tiles, chunks split over 4 waves" +
               (s.big_sketch ? "; segments of " + std::to_string(PLAN_SEG_CHUNKS) + " chunks" : "") +
               (sliced && s.mode == PLAN_MODE_COUNTS && s.tail_slices > 1u
                    ? "; " + std::to_string(s.tail_slices) + " chunk slices per unit in the last round of workgroups" : "") + ")";
    }
    return "skl::pair_kernel_ksplit<R=" + std::to_string(s.ksplit_rows) + ", " + m + "> (" + std::to_string(s.ksplit_rows) +
           "x64 tiles, chunks split over 4 waves)";
}

// HOST DESTINATION: rows [r0, r1) in bands of at most band_bytes through two device buffers -- band i is copied back while
// band i + 1 is computed.  A band is whole rows, so a single row wider than a band is a band by itself and needs a buffer
// of its own size.
struct HostBand {
    uint64_t r0 = 0, r1 = 0, pairs = 0;
    int buf = 0;               // which of the two buffers
    bool own_buffer = false;   // a single row wider than band_alloc: the buffer grows to it
};
struct HostBands {
    std::vector<HostBand> bands;
    size_t band_alloc = 0;        // bytes of the first buffer ...
    size_t second_alloc = 16;     // ... and of the second (a call of one band never uses it)
};
inline HostBands plan_host_bands(bool self_mode, uint64_t n_cols, uint64_t r0, uint64_t r1, size_t rec, size_t band_bytes)
{
    HostBands out;
    const uint64_t all_pairs = self_mode ? self_rows_pairs(r0, r1, n_cols) : (r1 - r0) * n_cols;
    out.band_alloc = (size_t)std::min<uint64_t>(band_bytes, all_pairs * rec);
    out.second_alloc = all_pairs * rec > band_bytes ? out.band_alloc : 16;
    uint64_t b0 = r0;
    while (b0 < r1) {
        HostBand b;
        b.r0 = b0;
        uint64_t b1 = b0;
        while (b1 < r1) {
            const uint64_t row_pairs = self_mode ? (n_cols - 1 - b1) : n_cols;
            if (b.pairs && (b.pairs + row_pairs) * rec > band_bytes) break;
            b.pairs += row_pairs;
            ++b1;
        }
        b.r1 = b1;
        b.buf = (int)(out.bands.size() & 1);
        b.own_buffer = b.pairs * rec > out.band_alloc;
        out.bands.push_back(b);
        b0 = b1;
    }
    return out;
}

}  // namespace skl
