// sketch_plan_check.cpp -- csrc/nthash.hpp and csrc/sketch_plan.hpp on the CPU, the two headers alone: the arithmetic the sketch
// kernels share with the host (mod_sign, bin_of, the split rotation, the top tables, the 2-bit packer) against the obvious slow
// form, and the plans (spans per sample, upload batches, the read-survivor span table, the close-before cutter with the caps of
// its five call sites) against values worked out by hand.  Host compiler only; also the program the sanitizer build runs.
//
//   sketch_plan_check <section>     mod_sign | bin_of | hash | pack | plan | upload | cutter | spans:  "ok <section> ..." and status
//                                   0, or the first mismatch and status 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../sketchlib.rust_amd/csrc/nthash.hpp"
#include "../../sketchlib.rust_amd/csrc/sketch_plan.hpp"

using namespace skl;
using Cuts = std::vector<size_t>;
using U64s = std::vector<uint64_t>;

#define REQUIRE(cond)                                                  \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("MISMATCH %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static int check_mod_sign()
{
    std::mt19937_64 rng(61);
    U64s in{0, SIGN_MOD - 1, SIGN_MOD, SIGN_MOD + 1, 1ull << 61, (1ull << 62) - 1, ~0ull};
    for (int i = 0; i < 5000; ++i) in.push_back(rng());
    for (int i = 0; i < 1000; ++i) in.push_back(SIGN_MOD * (1 + rng() % 7) + (rng() % 5) - 2);   // around the multiples of SIGN_MOD
    for (uint64_t h : in) REQUIRE(mod_sign(h) == h % SIGN_MOD);
    printf("ok mod_sign %zu\n", in.size());
    return 0;
}

// bin_of(sign) == sign / bin_size at every bin edge; how often the estimate was off either way and each correction fired
static int check_bin_of()
{
    std::mt19937_64 rng(170);
    uint64_t total_dec = 0, total_inc = 0;
    for (uint64_t nb : {1ull, 63ull, 64ull, 1000ull, 4096ull, 4097ull, 100032ull, 1ull << 20}) {
        const uint64_t bs = bin_size_of(nb);
        REQUIRE(bs == SIGN_MOD / nb + (SIGN_MOD % nb != 0));
        const double inv = 1.0 / (double)bs;
        const uint32_t last = (uint32_t)(nb - 1);
        U64s bins;
        if (nb <= 4097) {
            for (uint64_t b = 0; b < nb; ++b) bins.push_back(b);
        } else {
            bins = {0, nb - 1};
            for (int i = 0; i < 4000; ++i) bins.push_back(rng() % nb);
        }
        U64s signs{SIGN_MOD - 1};
        for (uint64_t b : bins) {
            const uint64_t e = b * bs;
            for (uint64_t s : {e - 1, e, e + 1}) {
                if (s < SIGN_MOD) signs.push_back(s);   // (e - 1 of bin 0 wraps and is left out)
            }
        }
        uint64_t clamped = 0, over = 0, under = 0, dec = 0, inc = 0;
        for (uint64_t s : signs) {
            const uint64_t want = s / bs;
            REQUIRE(want <= last);
            const uint32_t raw = (uint32_t)((double)s * inv);   // the plain reciprocal estimate
            const uint32_t est = bin_estimate(s, inv, last), got = bin_of(s, inv, bs, last);
            REQUIRE(est == (raw > last ? last : raw));
            REQUIRE(est + 1 >= want && est <= want + 1);        // off by at most one
            REQUIRE(got == want);
            clamped += raw > last;
            over += est > want;
            under += est < want;
            dec += got < est;
            inc += got > est;
        }
        REQUIRE(dec == over && inc == under);
        // Overshoots (edge - 1 rounds up to the edge on its way to double) occur at every bin count above one; with one bin only
        // the clamp can act.  Undershoots: the estimate is monotone in the sign -- the conversion to double and the product by
        // a positive constant both are -- so within a bin it is lowest at the bin's edge, and a bin count whose EVERY edge was
        // tried without an undershoot has none at any sign: there the `++bin` branch cannot be reached and no sign can be added
        // that reaches it.  That is so at 63, 64, 1000, 4096 and 4097 bins (all edges tried) and at 2^20 (a power-of-two bin
        // size: the reciprocal is exact and every edge is a double); 100 032 bins undershoots at about a quarter of its edges.
        // Random signs inside the bins confirm the consequence where the edges showed none.
        if (nb == 1) REQUIRE(clamped == 1 && over == 0 && under == 0);
        else REQUIRE(over > 0);
        if (under == 0) {
            REQUIRE(nb <= 4097 || (bs & (bs - 1)) == 0);
            for (int i = 0; i < 4000; ++i) {
                const uint64_t s = rng() % SIGN_MOD;
                REQUIRE(bin_estimate(s, inv, last) >= s / bs && bin_of(s, inv, bs, last) == s / bs);
            }
        }
        printf("bins %llu signs %zu clamped %llu over %llu under %llu\n", (unsigned long long)nb, signs.size(),
               (unsigned long long)clamped, (unsigned long long)over, (unsigned long long)under);
        total_dec += dec;
        total_inc += inc;
    }
    REQUIRE(total_dec > 0 && total_inc > 0);   // both branches of the correction are reached
    printf("ok bin_of %llu %llu\n", (unsigned long long)total_dec, (unsigned long long)total_inc);
    return 0;
}

static int check_hash()
{
    std::mt19937_64 rng(33);
    for (int i = 0; i < 5000; ++i) {
        const uint64_t v = i < 4 ? hash_fwd((uint32_t)i) : rng();
        REQUIRE(sror(srol(v)) == v && srol(sror(v)) == v);
        REQUIRE(rotr1(rotl1(v)) == v && swapbits033(swapbits033(v)) == v);
        REQUIRE(srol(v) == swapbits033((v << 1) | (v >> 63)));
    }
    for (uint32_t c = 0; c < 4; ++c) {
        REQUIRE(hash_rc(c) == hash_fwd(c ^ 2u));
        for (uint32_t d = 0; d < c; ++d) REQUIRE(hash_fwd(c) != hash_fwd(d));
    }
    for (size_t k : {1, 2, 31, 129, 300}) {
        uint64_t top_f[4], top_r[4];
        nthash_top_tables(k, top_f, top_r);
        for (uint32_t b = 0; b < 4; ++b) {
            uint64_t f = hash_fwd(b), r = hash_rc(b);
            for (size_t m = 0; m + 1 < k; ++m) {
                f = srol(f);
                r = srol(r);
            }
            REQUIRE(top_f[b] == f && top_r[b] == r);
        }
    }
    printf("ok hash\n");
    return 0;
}

static int check_pack()
{
    std::mt19937_64 rng(16);
    for (size_t n : {0, 1, 15, 16, 17, 31, 32, 33, 1000}) {
        std::vector<uint8_t> codes(n);
        for (auto &c : codes) c = (uint8_t)(rng() & 3u);
        const size_t words = (n + 15) / 16;
        std::vector<uint32_t> got(words + 1, 0xA5A5A5A5u), want(words, 0);
        for (size_t c = 0; c < n; ++c) want[c / 16] |= (uint32_t)codes[c] << (2 * (c % 16));   // (bits past the last code stay zero)
        pack_codes(codes.data(), n, got.data());
        REQUIRE(got[words] == 0xA5A5A5A5u);   // nothing past the last word
        got.pop_back();
        REQUIRE(got == want);
        for (size_t w = 0; w + 1 < words || (w < words && n % 16 == 0); ++w) REQUIRE(pack16(codes.data() + 16 * w) == want[w]);
        std::vector<uint32_t> part(words, 0xA5A5A5A5u);   // a range of words, as the library's packing threads take them
        pack_code_words(codes.data(), n, words / 2, words, part.data());
        for (size_t w = 0; w < words; ++w) REQUIRE(part[w] == (w < words / 2 ? 0xA5A5A5A5u : want[w]));
    }
    printf("ok pack\n");
    return 0;
}

static U64s prefix(const U64s &lengths)
{
    U64s begin(lengths.size() + 1, 0);
    for (size_t i = 0; i < lengths.size(); ++i) begin[i + 1] = begin[i] + lengths[i];
    return begin;
}

static int check_plan()
{
    REQUIRE(SKETCH_SPAN == 256 && SKETCH_WG == 256 && SKETCH_SPAN_LDS == 128 && SKETCH_WG_LDS == 512 && SKETCH_LDS_BINS_MAX == 4096);
    REQUIRE(READ_SURVIVOR_SPAN == 64 && READ_SURVIVOR_WG % 64 == 0);
    const U64s lengths{0, 1, 127, 128, 129, 65535, 65536, 65537};
    const U64s cb = prefix(lengths);
    // the form: the staged kernel takes k <= 129
    REQUIRE(sketch_plan(cb.data(), lengths.size(), 129, false).lds_form);
    REQUIRE(!sketch_plan(cb.data(), lengths.size(), 130, false).lds_form);
    REQUIRE(!sketch_plan(cb.data(), lengths.size(), 129, true).lds_form);
    REQUIRE(!sketch_plan(cb.data(), lengths.size(), 21, true).lds_form);
    const U64s words{0, 1, 8, 8, 9, 4096, 4096, 4097};
    {   // staged: 128 starts per span, 512 spans per workgroup
        const SketchPlan p = sketch_plan(cb.data(), lengths.size(), 31, false);
        REQUIRE(p.span_begin == prefix({0, 512, 512, 512, 512, 512, 512, 1024}));
        REQUIRE(p.word_begin == prefix(words));
    }
    {   // unstaged: 256 starts per span, 256 spans per workgroup
        const SketchPlan p = sketch_plan(cb.data(), lengths.size(), 130, false);
        REQUIRE(p.span_begin == prefix({0, 256, 256, 256, 256, 256, 256, 512}));
        REQUIRE(p.word_begin == prefix(words));
    }
    {   // empty samples at the front, in the middle and at the end
        const U64s e{0, 5, 0, 0, 70000, 0};
        const U64s eb = prefix(e);
        const SketchPlan p = sketch_plan(eb.data(), e.size(), 21, false);
        REQUIRE(p.lds_form);
        REQUIRE(p.span_begin == prefix({0, 512, 0, 0, 1024, 0}));
        REQUIRE(p.word_begin == prefix({0, 1, 0, 0, 4375, 0}));
        REQUIRE(sketch_plan(eb.data(), e.size(), 300, false).span_begin == prefix({0, 256, 0, 0, 512, 0}));
    }
    const SketchPlan none = sketch_plan(cb.data(), 0, 21, false);
    REQUIRE(none.span_begin == U64s{0} && none.word_begin == U64s{0});
    printf("ok plan\n");
    return 0;
}

// the two shapes of tests/test_gpu_sketch_edges.py test_batches_at_small_shapes, in bases
static int check_upload()
{
    const U64s short_lengths{0, 1, 20, 21, 22, 15, 16, 17, 0, 0, 200, 0, 70000, 0, 0};
    const U64s seven_lengths{2000, 70000, 16 * 300, 33333, 2001, 65536, 4099};
    const U64s sb = prefix(short_lengths), vb = prefix(seven_lengths);
    const U64s sw = sketch_plan(sb.data(), short_lengths.size(), 21, false).word_begin;
    const U64s vw = sketch_plan(vb.data(), seven_lengths.size(), 31, false).word_begin;
    REQUIRE(sw == prefix({0, 1, 2, 2, 2, 1, 1, 2, 0, 0, 13, 0, 4375, 0, 0}));
    REQUIRE(vw == prefix({125, 4375, 300, 2084, 126, 4096, 257}));
    auto cut = [](const U64s &wb, uint64_t setting) { return sketch_upload_batches(wb.data(), wb.size() - 1, setting); };
    // setting 1: every non-empty sample a batch (the empty ones before it ride along), a trailing batch of empty samples
    REQUIRE(cut(sw, 1) == (Cuts{0, 2, 3, 4, 5, 6, 7, 8, 11, 13, 15}));
    REQUIRE(cut(sw, 4096) == (Cuts{0, 13, 15}));
    REQUIRE(cut(sw, 3) == (Cuts{0, 3, 5, 8, 11, 13, 15}));   // the first batch reaches 3 words exactly
    REQUIRE(cut(sw, SKETCH_BATCH_WORDS) == (Cuts{0, 15}));
    REQUIRE(cut(vw, 1) == (Cuts{0, 1, 2, 3, 4, 5, 6, 7}));   // (the last sample is never closed behind)
    REQUIRE(cut(vw, 4096) == (Cuts{0, 2, 6, 7}));
    REQUIRE(cut(vw, 125) == (Cuts{0, 1, 2, 3, 4, 5, 6, 7}));   // met exactly by the first sample
    REQUIRE(cut(vw, SKETCH_BATCH_WORDS) == (Cuts{0, 7}));
    REQUIRE(cut(vw, 4375 + 125) == (Cuts{0, 2, 6, 7}));       // met exactly by two samples together
    REQUIRE(cut(U64s{0}, 1) == (Cuts{0, 0}));
    REQUIRE(SKETCH_BATCH_WORDS == 8ull << 20);
    printf("ok upload\n");
    return 0;
}

static Cuts cut(const U64s &sizes, const CutCaps &caps)
{
    return cut_before(sizes.size(), [&](size_t i) { return sizes[i]; }, caps);
}

static int check_cutter()
{
    const uint64_t Gi = 1ull << 30;
    // the rule itself
    REQUIRE(cut({5, 100, 5}, {10, 0, 0}) == (Cuts{0, 1, 2, 3}));          // a single item over the sum cap: a batch of its own
    REQUIRE(cut({5, 5, 5}, {1000, 100, 10}) == (Cuts{0, 1, 2, 3}));       // ... over the count cap
    REQUIRE(cut({4, 6, 1}, {10, 0, 0}) == (Cuts{0, 2, 3}));               // a batch that exactly fills the cap stays whole
    REQUIRE(cut({1, 1, 1, 1, 1, 1}, {1000, 2, 6}) == (Cuts{0, 3, 6}));    // ... and so for the count cap
    REQUIRE(cut({1, 1, 1, 1, 1, 1, 1}, {1000, 1, 3}) == (Cuts{0, 3, 6, 7}));
    REQUIRE(cut({0, 0, 10, 0, 0, 10, 0}, {10, 0, 0}) == (Cuts{0, 5, 7}));   // empty items close nothing
    REQUIRE(cut({0, 0, 0}, {0, 0, 0}) == (Cuts{0, 3}));
    REQUIRE(cut({}, {10, 1, 10}) == (Cuts{0, 0}));                          // n = 0: one empty batch
    // 1. one amino-acid call: 1 Gi residues, 1 GiB of signs on the device
    REQUIRE(cut({Gi / 2, Gi / 2, 1}, caps_aa_call(1, 1024)) == (Cuts{0, 2, 3}));
    REQUIRE(cut(U64s(131073, 1), caps_aa_call(1, 1024)) == (Cuts{0, 131072, 131073}));   // 8 KiB of signs each
    REQUIRE(cut(U64s(33, 0), caps_aa_call(4, 1 << 20)) == (Cuts{0, 32, 33}));            // 32 MiB each
    // 2. one DNA call: 4 Gi bases, any number of samples
    REQUIRE(cut({2 * Gi, 2 * Gi, 1, 4 * Gi + 1, 1}, caps_dna_call()) == (Cuts{0, 2, 3, 4, 5}));
    REQUIRE(cut(U64s(1000, 0), caps_dna_call()) == (Cuts{0, 1000}));
    // 3. read sets under a count filter: max(64, nk) streams, 1 Gi bases
    REQUIRE(cut(U64s(130, 1), caps_filtered_reads(1)) == (Cuts{0, 64, 128, 130}));
    REQUIRE(cut(U64s(25, 1), caps_filtered_reads(5)) == (Cuts{0, 12, 24, 25}));     // 12 x 5 = 60 streams; 13 would be 65
    REQUIRE(cut(U64s(3, 1), caps_filtered_reads(64)) == (Cuts{0, 1, 2, 3}));
    REQUIRE(cut(U64s(3, 1), caps_filtered_reads(70)) == (Cuts{0, 1, 2, 3}));        // more lengths than 64: one sample at a time
    REQUIRE(cut({Gi / 2, Gi / 2, Gi / 2}, caps_filtered_reads(1)) == (Cuts{0, 2, 3}));
    // 4. one u16 call (inverted index rows): 4 Gi bases, 1 GiB of signs on the device
    REQUIRE(cut({4 * Gi - 1, 1, 1}, caps_u16_call(1024)) == (Cuts{0, 2, 3}));
    REQUIRE(cut({4 * Gi, 1}, caps_u16_call(1024)) == (Cuts{0, 1, 2}));
    REQUIRE(cut(U64s(5, 0), caps_u16_call(1 << 26)) == (Cuts{0, 2, 4, 5}));         // 512 MiB each
    REQUIRE(cut(U64s(3, 0), caps_u16_call(1 << 27)) == (Cuts{0, 1, 2, 3}));
    // 5. an index's read sets under a count filter: one k-mer length, so 64 samples
    REQUIRE(cut(U64s(65, 1), caps_filtered_reads(1)) == (Cuts{0, 64, 65}));
    REQUIRE(cut({Gi, Gi}, caps_filtered_reads(1)) == (Cuts{0, 1, 2}));
    REQUIRE(cut({Gi / 2, Gi / 2}, caps_filtered_reads(1)) == (Cuts{0, 2}));
    printf("ok cutter\n");
    return 0;
}

static int check_spans()
{
    //                 inside     end < begin  64 x 64 starts  one more   past the end  empty
    const U64s lengths{100,       5000,        4096,           4097,      100,          0};
    const U64s wb     {50,        3000,        0,              0,         200,          0};
    const U64s we     {1000,      2000,        4096,           ~0ull,     300,          10};
    const U64s cb = prefix(lengths);
    const size_t n = lengths.size();
    const U64s head = read_survivor_spans(cb.data(), wb.data(), we.data(), n);
    REQUIRE(head.size() == 3 * n + 1);
    REQUIRE(U64s(head.begin(), head.begin() + n) == (U64s{50, 3000, 0, 0, 100, 0}));            // window ranges clamped to the sample
    REQUIRE(U64s(head.begin() + n, head.begin() + 2 * n) == (U64s{100, 3000, 4096, 4097, 100, 0}));
    REQUIRE(U64s(head.begin() + 2 * n, head.end()) == prefix({64, 0, 64, 128, 0, 0}));          // whole waves of 64-start spans
    REQUIRE(read_survivor_spans(cb.data(), wb.data(), we.data(), 0) == U64s{0});
    printf("ok spans\n");
    return 0;
}

int main(int argc, char **argv)
{
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "mod_sign") return check_mod_sign();
    if (what == "bin_of") return check_bin_of();
    if (what == "hash") return check_hash();
    if (what == "pack") return check_pack();
    if (what == "plan") return check_plan();
    if (what == "upload") return check_upload();
    if (what == "cutter") return check_cutter();
    if (what == "spans") return check_spans();
    fprintf(stderr, "usage: sketch_plan_check mod_sign|bin_of|hash|pack|plan|upload|cutter|spans\n");
    return 2;
}
