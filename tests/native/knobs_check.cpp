// knobs_check.cpp -- csrc/knobs.hpp alone (no HIP header, no library): the reader knobs_from() over a map in place of the
// environment.  Built twice by tests/test_knobs_cpu.py, with and without -DSKL_AB.
//
// The expected values below are written out BY HAND, transcribed from the reader this table replaced (one assignment per
// switch); nothing here is derived from knobs.def except the list of names and the "no other field moved" comparison.
// Prints `product NAME` / `ab NAME` for every switch of the table, then `ok <checks>`.
#include "../../sketchlib.rust_amd/csrc/knobs.hpp"

#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

static std::map<std::string, std::string> g_env;
static const char *look(const char *name)
{
    const auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}

static size_t g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        ++g_checks;                                           \
        if (!(cond)) {                                        \
            ++g_failed;                                       \
            fprintf(stderr, "FAILED line %d: ", __LINE__);    \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
        }                                                     \
    } while (0)

// every field as a number, in the table's order
static std::vector<long long> fields(const Knobs &k)
{
    std::vector<long long> v;
#define KNOB_INT(cls, type, field, ...) v.push_back((long long)k.field);
#define KNOB_INT_UNLESS_0(cls, type, field, ...) v.push_back((long long)k.field);
#define KNOB_WORD(cls, field, ...) v.push_back((long long)k.field);
#define KNOB_CHOICE(cls, field, ...) v.push_back((long long)k.field);
#include "../../sketchlib.rust_amd/csrc/knobs.def"
    return v;
}
// the table's variables by class
static std::vector<std::string> names_PRODUCT, names_AB;
static void list_names()
{
#define KNOB_INT(cls, type, field, name, ...) names_##cls.push_back(name);
#define KNOB_INT_UNLESS_0(cls, type, field, name, ...) names_##cls.push_back(name);
#define KNOB_WORD(cls, field, name, ...) names_##cls.push_back(name);
#define KNOB_CHOICE(cls, field, name, ...) names_##cls.push_back(name);
#include "../../sketchlib.rust_amd/csrc/knobs.def"
}

struct Expect {
    const char *name;
    bool ab_only;
    long long (*get)(const Knobs &);
    long long dflt;                                             // unset, and the empty string
    std::vector<std::pair<const char *, long long>> cases;      // the variable's text -> the field (A/B build; product build too unless ab_only)
};
#define F(field) [](const Knobs &k) -> long long { return (long long)k.field; }

// a switch that is on unless its number is 0 / off unless its number is not 0: inside, "below" and "above" are all "not 0"
#define ON_UNLESS_0 {{"0", 0}, {"1", 1}, {"2", 1}, {"-1", 1}, {"abc", 0}, {"1x", 1}}
#define OFF_UNLESS_NOT_0 {{"0", 0}, {"1", 1}, {"7", 1}, {"-1", 1}, {"abc", 0}}
// no clamp at all: the number as it is
#define AS_IT_IS {{"3", 3}, {"-2", -2}, {"100000", 100000}, {"abc", 0}, {"12abc", 12}}
// held to >= 0 only
#define AT_LEAST_0 {{"64", 64}, {"0", 0}, {"-1", 0}, {"-99999999999", 0}, {"99999999999", 99999999999ll}, {"abc", 0}, {"5 rows", 5}}

static const std::vector<Expect> EXPECT = {
    // ---- the product library's
    {"SKL_TIMING_EVERY", false, F(timing_every), 0, AT_LEAST_0},
    {"SKL_SLICED_MAX_PAIRS", false, F(sliced_max_pairs), -1, {{"1000", 1000}, {"0", 0}, {"-7", -7}, {"99999999999", 99999999999ll}, {"abc", 0}}},
    {"SKL_KNN_BAND_ROWS", false, F(knn_band_rows), 0, AT_LEAST_0},
    {"SKL_INVQ_BAND_BYTES", false, F(invq_band_bytes), 0, AT_LEAST_0},
    {"SKL_INVQ_TOP_DIGIT_BITS", false, F(invq_top_digit_bits), 0, AT_LEAST_0},
    {"SKL_SKETCH_BATCH_WORDS", false, F(sketch_batch_words), 0, {{"0", 0}, {"5", 5}, {"1", 1}, {"-4", 1}, {"99999999999", 99999999999ll}, {"abc", 0}}},
    {"SKL_AA_BATCH_SIGN_BYTES", false, F(aa_batch_sign_bytes), 0, AT_LEAST_0},
    {"SKL_AA_LONG_MIN", false, F(aa_long_min), 0, AT_LEAST_0},
    {"SKL_PAIRS_BAND", false, F(pairs_band), 0, AT_LEAST_0},
    {"SKL_FINISH_MAX_ATTEMPTS", false, F(finish_max_attempts), 0, AT_LEAST_0},
    {"SKL_SKETCH_FINISH", false, F(sketch_finish_host), 0, {{"host", 1}, {"device", 0}, {"Host", 0}, {"hostx", 0}, {"1", 0}}},
    {"SKL_TAIL_SLICES", false, F(tail_slices), 4, {{"2", 2}, {"0", 0}, {"8", 8}, {"-1", 0}, {"9", 8}, {"abc", 0}}},
    {"SKL_TAIL_MAX_PCT", false, F(tail_max_pct), 90, {{"50", 50}, {"-5", -5}, {"1000", 1000}, {"abc", 0}}},
    {"SKL_TILE32_MIN", false, F(tile32_min), 8388608, {{"100", 100}, {"0", 0}, {"-1", -1}, {"-5", -5}, {"99999999999", 99999999999ll}, {"abc", 0}}},
    {"SKL_GROUP_SPAN", false, F(group_span), 2, {{"4", 4}, {"1", 1}, {"64", 64}, {"0", 1}, {"-3", 1}, {"65", 64}, {"abc", 1}}},
    {"SKL_XCDS", false, F(xcds), 0, {{"4", 4}, {"8", 8}, {"-1", 0}, {"9", 8}, {"abc", 0}}},
    {"SKL_EB_STRIPES", false, F(eb_stripes), -1, {{"0", 0}, {"1", 1}, {"-1", -1}, {"-5", -1}, {"3", 1}, {"abc", 0}}},
    {"SKL_TILE_COST_ORDER", false, F(tile_cost_order), -1, {{"0", 0}, {"1", 1}, {"-1", -1}, {"-5", -1}, {"3", 1}, {"abc", 0}}},
    // ---- the A/B build's
    {"SKL_K_SLICES", true, F(k_slices), 0, AS_IT_IS},
    {"SKL_ROUND_PRIORITY", true, F(round_priority), 1, ON_UNLESS_0},
    {"SKL_HALF_TILES", true, F(half_tiles), 1, ON_UNLESS_0},
    {"SKL_MID_BAND", true, F(mid_band), 1, ON_UNLESS_0},
    {"SKL_KNN_SYMMETRIC", true, F(knn_symmetric), 1, ON_UNLESS_0},
    {"SKL_KNN_OVERLAP", true, F(knn_overlap), 1, ON_UNLESS_0},
    {"SKL_KNN_PRUNE", true, F(knn_prune), 1, ON_UNLESS_0},
    {"SKL_KNN_PANEL", true, F(knn_panel), 0, AS_IT_IS},
    {"SKL_KNN_SPARSE", true, F(knn_sparse), 1, ON_UNLESS_0},
    {"SKL_EARLY_BREAK", true, F(early_break), 1, {{"3", 3}, {"0", 0}, {"7", 7}, {"-1", 0}, {"8", 7}, {"abc", 0}}},
    {"SKL_EPILOGUE_R5", true, F(epilogue_r5), 0, OFF_UNLESS_NOT_0},
    {"SKL_EB_PIPELINE", true, F(eb_pipeline), -1, AS_IT_IS},
    {"SKL_EB_PIPELINE_MIN", true, F(eb_pipeline_min), 67108864, {{"100", 100}, {"2", 2}, {"1", 2}, {"0", 2}, {"-8", 2}, {"99999999999", 99999999999ll}, {"abc", 2}}},
    {"SKL_COUNTS_U16", true, F(counts_u16), 1, ON_UNLESS_0},
    {"SKL_EB_LDS_ROWS", true, F(eb_lds_rows), 1, ON_UNLESS_0},
    {"SKL_EB_AHEAD", true, F(eb_ahead), 1, ON_UNLESS_0},
    {"SKL_EB_LEAN", true, F(eb_lean), 1, ON_UNLESS_0},
    {"SKL_KNN_EPI_BLOCKED", true, F(knn_epi_blocked), 1, {{"0", 0}, {"2", 2}, {"-1", 0}, {"3", 2}, {"abc", 0}}},
    {"SKL_EB_BLOCKED", true, F(eb_blocked), -1, AS_IT_IS},
    {"SKL_EB_BLK_ROW_SHIFT", true, F(eb_blk_row_shift), 10, AS_IT_IS},
    {"SKL_FUSE_EPILOGUE", true, F(fuse_epilogue), 0, OFF_UNLESS_NOT_0},
    {"SKL_FUSE_VARIANT", true, F(fuse_variant), 0, {{"2", 2}, {"-1", 4294967295ll}, {"abc", 0}}},
    {"SKL_REFHEAP_WAVE", true, F(refheap_wave), 1, ON_UNLESS_0},
    {"SKL_KNN_ROW_FLAGS", true, F(knn_row_flags), 1, ON_UNLESS_0},
    {"SKL_TOPK_STREAM", true, F(topk_stream), 1, ON_UNLESS_0},
    {"SKL_CAND_SYMMETRIC", true, F(cand_symmetric), 1, ON_UNLESS_0},
    {"SKL_CAND_ROW_ORDER", true, F(cand_row_order), 1, ON_UNLESS_0},
    {"SKL_CAND_KERNEL", true, F(cand_lanes), 0, {{"lanes", 1}, {"rows", 0}, {"Lanes", 0}, {"lanes ", 0}, {"1", 0}}},
    {"SKL_INLINE_PREFIX", true, F(inline_prefix), 1, ON_UNLESS_0},
    {"SKL_SKETCH_KERNEL", true, F(sketch_global), 0, {{"global", 1}, {"staged", 0}, {"GLOBAL", 0}, {"1", 0}}},
    {"SKL_KERNEL", true, F(kernel), 0, {{"ksplit", 3}, {"kslice", 4}, {"lds", 0}, {"3", 0}, {"Kslice", 0}}},
    {"SKL_KSLICE_SHAPE", true, F(kslice_shape), 0, {{"3255", 3255}, {"165", 165}, {"-1", -1}, {"abc", 0}}},
    {"SKL_KSPLIT_ROWS", true, F(ksplit_rows), 0, {{"4", 4}, {"8", 8}, {"-1", -1}, {"abc", 0}}},
    {"SKL_KSLICE_ABLATE", true, F(kslice_ablate), 0, {{"2", 2}, {"-1", -1}, {"abc", 0}}},
    {"SKL_FORCE_LOG_VARIANT", true, F(force_log_variant), -2, {{"-1", -1}, {"0", 0}, {"1", 1}, {"-2", -2}, {"-9", -2}, {"5", 1}, {"abc", 0}}},
};

#ifdef SKL_AB
constexpr bool AB_BUILD = true;
#else
constexpr bool AB_BUILD = false;
#endif

int main()
{
    list_names();
    const std::vector<long long> base = fields(Knobs());
    // nothing set: the defaults, which are also the struct's initialisers
    CHECK(fields(knobs_from(look)) == base, "an empty environment does not give the struct's defaults");
    for (const Expect &e : EXPECT) CHECK(e.get(Knobs()) == e.dflt, "%s: default %lld, expected %lld", e.name, e.get(Knobs()), e.dflt);
    // the hand list and the table name the same variables, in the same classes
    CHECK(EXPECT.size() == names_PRODUCT.size() + names_AB.size() && base.size() == EXPECT.size(), "%zu expectations, %zu + %zu names, %zu fields",
          EXPECT.size(), names_PRODUCT.size(), names_AB.size(), base.size());
    for (const Expect &e : EXPECT) {
        size_t found = 0;
        for (const std::string &n : e.ab_only ? names_AB : names_PRODUCT) found += n == e.name ? 1 : 0;
        CHECK(found == 1, "%s: %zu times in the table's %s class", e.name, found, e.ab_only ? "A/B" : "product");
    }
    for (const Expect &e : EXPECT) {
        const bool read = AB_BUILD || !e.ab_only;   // the product build reads no A/B-only switch: setting one changes nothing
        std::vector<std::pair<const char *, long long>> cases = e.cases;
        cases.push_back({"", e.dflt});              // an empty string counts as unset
        for (const auto &c : cases) {
            g_env.clear();
            g_env[e.name] = c.first;
            const Knobs k = knobs_from(look);
            const long long want = read ? c.second : e.dflt;
            CHECK(e.get(k) == want, "%s=\"%s\": %lld, expected %lld", e.name, c.first, e.get(k), want);
            const std::vector<long long> got = fields(k);
            size_t moved = 0;
            for (size_t i = 0; i < got.size() && i < base.size(); ++i) moved += got[i] != base[i] ? 1 : 0;
            CHECK(moved == (want != e.dflt ? 1u : 0u), "%s=\"%s\": %zu fields left their defaults", e.name, c.first, moved);
        }
    }
    {   // several at once: each lands in its own field
        g_env.clear();
        g_env["SKL_TAIL_SLICES"] = "3";
        g_env["SKL_XCDS"] = "1";
        g_env["SKL_KERNEL"] = "kslice";
        g_env["SKL_EARLY_BREAK"] = "5";
        const Knobs k = knobs_from(look);
        CHECK(k.tail_slices == 3 && k.xcds == 1, "tail_slices %d xcds %d", k.tail_slices, k.xcds);
        CHECK(k.kernel == (AB_BUILD ? 4 : 0) && k.early_break == (AB_BUILD ? 5 : 1), "kernel %d early_break %d", k.kernel, k.early_break);
    }
    for (const std::string &n : names_PRODUCT) printf("product %s\n", n.c_str());
    for (const std::string &n : names_AB) printf("ab %s\n", n.c_str());
    if (g_failed) {
        printf("FAILED %zu of %zu\n", g_failed, g_checks);
        return 1;
    }
    printf("ok %zu\n", g_checks);
    return 0;
}
