// knobs.hpp -- the environment switches as a plain struct.  No HIP header: the launch plan (dense_plan.hpp) and its CPU test
// read it without a device toolchain.  capi_internal.hpp includes it; capi.cpp read_knobs() fills it.
#pragma once

// Environment switches.  They are read ONCE, when a context is created (skl_ctx_create), never on
// the launch path.  The product library READS eighteen of them (capi.cpp read_knobs: timing cadence, topology,
// the knobs that force the banded / sliced / 32-row forms and the striped epilogue order and the cost order of the tiles on small test inputs, the inverted query's band budget and the digit width of its best-hit selection, the sketching calls' batch sizes and form threshold, where and how far their streams are finished, the pair list's band); every "A/B only, results
// identical" switch below keeps its default there and is read by the A/B build alone (-DSKL_AB), as are kernel
// selection, tile shapes and the timing-only ablations.
struct Knobs {
    long long timing_every = 0;       // SKL_TIMING_EVERY: bracket every N-th pair-kernel launch with events (0: none; skl_ctx_timing_enable overrides)
    long long sliced_max_pairs = -1;  // SKL_SLICED_MAX_PAIRS: core/acc launches below this run k-sliced (-1: default)
    long long knn_band_rows = 0;      // SKL_KNN_BAND_ROWS: force the band height of the kNN drivers (tests)
    long long invq_band_bytes = 0;    // SKL_INVQ_BAND_BYTES: device memory per query band of skl_inverted_query (0: 1 GiB; tests force it low)
    long long invq_top_digit_bits = 0; // SKL_INVQ_TOP_DIGIT_BITS: bits per digit of skl_inverted_query_top's radix select (1..11; 0: 11, inv_top_plan.hpp; tests force several passes at small sketch sizes)
    long long sketch_batch_words = 0; // SKL_SKETCH_BATCH_WORDS: packed words (16 bases each) from which skl_sketch_signs closes an upload batch of whole samples (0: 8 Mi; tests force it low)
    long long aa_batch_sign_bytes = 0; // SKL_AA_BATCH_SIGN_BYTES: bytes of signs from which skl_sketch_signs_aa closes a batch of whole samples (0: 256 MiB; tests force it low)
    long long aa_long_min = 0;        // SKL_AA_LONG_MIN: residues from which a sample takes the staged form of skl_sketch_signs_aa (0: 8 192; tests force 1: every sample staged)
    long long finish_max_attempts = 0; // SKL_FINISH_MAX_ATTEMPTS: probe cap per bin of the device-side densification (0: 2 048, finish_plan.hpp; tests force it low: capped streams are finished by the host)
    bool sketch_finish_host = false;  // SKL_SKETCH_FINISH=host: skl_sketch_finish / skl_sketch_usigs_* download the signs and densify + transpose on host threads (A/B timing, escape hatch; the same bytes)
    long long pairs_band = 0;         // SKL_PAIRS_BAND: listed pairs per upload band of skl_*_dists_pairs (0: 64 Mi; tests force it low)
    int k_slices = 0;                 // SKL_K_SLICES: chunk slices per k of k-sliced core/acc launches (0: chosen per launch)
    int xcds = 0;                       // SKL_XCDS: XCDs the tile order assumes (0: from the device's CU count: 256 CUs = 8, a 32-CU partition = 1)
    int eb_stripes = -1;                // SKL_EB_STRIPES: the early break's epilogue walks the pairs in column stripes folded onto the XCDs (eb_stripes.hpp): -1 by rule (dense_plan.hpp counts_striped), 0 never, 1 wherever the lean kernel stages its rows (tests)
    int tile_cost_order = -1;           // SKL_TILE_COST_ORDER: self-mode k-sliced counts launches deal their tiles to the XCDs by cost, half tiles last (work_map.hpp): -1 by rule (dense_plan.hpp tile_cost_order_rule), 0 never, 1 wherever the form allows (tests)
    int group_span = 2;                 // SKL_GROUP_SPAN: column groups whose tiles are numbered side by side (work_map.hpp lookup_tile_at)
    long long tile32_min = 8ll << 20;   // SKL_TILE32_MIN: pair x k evaluations from which launches use 32 x 128 tiles (-1: never, 0: always); 8 Mi since the k-sliced 32-row form holds 4 waves per SIMD (profiles/r03_ab_tile32_threshold.jsonl)
    bool mid_band = true;               // SKL_MID_BAND=0: no mid-band rule (32-row tiles + 2 slices of the last round at 0.5-1 x tile32_min evaluations; A/B only, results are identical)
    int tail_slices = 4;                // SKL_TAIL_SLICES: chunk slices per unit in the last, partial round of a k-sliced core/acc launch (0/1: off)
    bool half_tiles = true;             // SKL_HALF_TILES=0: 64-column blocks of a tile without a pair of the launch are walked anyway (A/B only, results are identical)
    bool round_priority = true;         // SKL_ROUND_PRIORITY=0: k-sliced workgroups of later rounds keep the default wave priority (A/B only, results are identical)
    long long tail_max_pct = 90;        // SKL_TAIL_MAX_PCT: ... for launches of up to this many estimated rounds of workgroups (in percent)
    bool knn_symmetric = true;        // SKL_KNN_SYMMETRIC=0: row-by-row self kNN
    bool knn_row_flags = true;        // SKL_KNN_ROW_FLAGS=0: the merge of the transposed band visits every row (A/B only, results are identical)
    bool knn_overlap = true;          // SKL_KNN_OVERLAP=0: top-k and pair kernel on one stream
    bool fuse_epilogue = false;       // A/B build, SKL_FUSE_EPILOGUE=1: the core/accessory epilogue of plain k-sliced launches inside the pair kernel (results identical; slower: profiles/r05_fused_epilogue.md)
    int early_break = 1;              // A/B build, SKL_EARLY_BREAK: 0 core/accessory launches count every k-mer length; 1 (default) the early break where a
                                      // sample of the pairs says it pays; 2..7 forced with that many lengths counted (tests).  Results identical.
    int eb_pipeline = -1;             // -1: the row bands of a large early-break call overlap (band i's epilogue beside band i + 1's counts kernel) where the lean epilogue runs in the flat order; A/B build, SKL_EB_PIPELINE=0 / 1 / 2: never / the old rule (general kernel too: from 3 % still in the running, or forced lengths; never with the blocked order) / wherever the lean kernel runs
    long long eb_pipeline_min = 64ll << 20;  // A/B build, SKL_EB_PIPELINE_MIN: pairs from which an early-break call is cut into overlapping row bands (tests force it low)
    int eb_blocked = -1;              // A/B build, SKL_EB_BLOCKED=0|1: the early break's epilogue walks the pairs in flat order / in 256 x 256 blocks per XCD (-1: by the size of the column slices)
    int eb_blk_row_shift = 10;        // A/B build, SKL_EB_BLK_ROW_SHIFT: rows per block (log2) of the blocked epilogue
    int knn_epi_blocked = 1;          // A/B build, SKL_KNN_EPI_BLOCKED=0 / 2: the kNN bands' early-break epilogue in row-major order / column-group-major per XCD whatever the view's width (default: from 16 384 columns; 2.52 -> 2.43 s at n = 300 000)
    bool eb_lean = true;              // A/B build, SKL_EB_LEAN=0: every early-break launch through the general epilogue kernel
    bool eb_ahead = true;             // A/B build, SKL_EB_AHEAD=0: completions one after the other, nothing requested ahead
    bool eb_lds_rows = true;          // A/B build, SKL_EB_LDS_ROWS=0: completions read the row sample's slice from memory, not from the workgroup's LDS copy
    bool counts_u16 = true;           // A/B build, SKL_COUNTS_U16=0: the counts scratch keeps u32 records
    bool epilogue_r5 = false;         // A/B build, SKL_EPILOGUE_R5=1: round 5's epilogue (alive pairs completed where they are found; timing)
    bool knn_sparse = true;           // A/B build, SKL_KNN_SPARSE=0: tiles that survive the probe are walked whole (results identical)
    long long knn_panel = 0;          // A/B build, SKL_KNN_PANEL: column-panel width of the row-by-row kNN forced (tests; 0: by size)
    bool knn_prune = true;            // SKL_KNN_PRUNE=0: the symmetric self kNN finishes every tile (A/B; results are identical)
    bool refheap_wave = true;         // SKL_REFHEAP_WAVE=0: the heap replays (one-shot and resumable) run one workgroup per row even for knn <= 256 (A/B only, results are identical)
    bool topk_stream = true;          // SKL_TOPK_STREAM=0: radix select instead of the streaming merge
    bool cand_symmetric = true;       // SKL_CAND_SYMMETRIC=0: evaluate symmetric candidate lists in full
    bool inline_prefix = true;        // SKL_INLINE_PREFIX=0: the tile lookup always searches the prefix table in global memory (A/B only, results are identical)
    bool cand_lanes = false;          // SKL_CAND_KERNEL=lanes: round 3's candidate-list kernel (lanes over the candidates; A/B only, results are identical)
    bool cand_row_order = true;       // SKL_CAND_ROW_ORDER=0: candidate-list rows dispatched in sample order, not by first candidate (A/B only, results are identical)
    bool sketch_global = false;       // SKL_SKETCH_KERNEL=global: the unstaged sketching kernel
#ifdef SKL_AB
    int kernel = 0;                   // SKL_KERNEL: 0 none, 3 ksplit, 4 kslice
    int kslice_shape = 0;             // SKL_KSLICE_SHAPE: 165 / 325 (shipped), 1651 / 1652 / 3254 / 3255 (their round-2/3 forms)
    int ksplit_rows = 0;              // SKL_KSPLIT_ROWS: 4 or 8
    int kslice_ablate = 0;            // SKL_KSLICE_ABLATE: timing only, outputs wrong by construction
#endif
};
