// finish_plan_check.cpp -- csrc/finish_plan.hpp on the CPU: the launch rules of the finish kernel as numbers, and the two-step
// restatement of densify_bin (target, then resolve) against the sequential loop of the host sketcher (skl_host::densify_bin)
// and its transpose against skl_host::fill_usigs.  Host compiler only.
//
//   finish_plan_check plan <num_bins>...        one line per size: num_bins lds_form threads lds_bytes workgroups(5000 streams) words
//   finish_plan_check consts                    lds_bins_max max_attempts max_rounds attempts(knob 8) attempts(knob 0)
//   finish_plan_check patterns <num_bins>       every pattern at this size against skl_host; one line per pattern: name flag worst_probes
//   finish_plan_check capped <max_attempts>     reads u64 signs from stdin; prints the flag the two steps give under that cap
//   finish_plan_check stream                    reads u64 signs from stdin; writes flag (1 byte), densified signs, words to stdout
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../sketchlib.rust_amd/csrc/finish_plan.hpp"
#include "../../sketchlib.rust_amd/csrc/host/sketch.hpp"

using namespace skl;

static std::vector<uint64_t> read_stdin()
{
    std::vector<uint64_t> v;
    uint64_t x;
    while (fread(&x, sizeof x, 1, stdin) == 1) v.push_back(x);
    return v;
}

static std::vector<uint64_t> random_signs(size_t n, std::mt19937_64 &rng)
{
    std::vector<uint64_t> v(n);
    for (auto &x : v) x = rng() % ((1ull << 61) - 1);
    return v;
}

static int fail(const char *what, const std::string &name, size_t n)
{
    printf("MISMATCH %s: pattern %s at %zu bins\n", what, name.c_str(), n);
    return 1;
}

// one pattern: the two steps against the sequential loop, the transpose against fill_usigs
static int check(const std::string &name, const std::vector<uint64_t> &orig)
{
    const size_t n = orig.size();
    std::vector<uint64_t> want = orig, got = orig;
    const bool want_densified = skl_host::densify_bin(want);
    uint32_t worst = 0;
    const uint8_t flag = finish_densify_two_step(got, 0, &worst);
    if (flag != (want_densified ? FINISH_DENSIFIED : 0)) return fail("flag", name, n);
    if (got != want) return fail("signs", name, n);
    std::vector<uint64_t> words_want(finish_words(n), 0), words_got(finish_words(n), ~0ull);
    skl_host::fill_usigs(words_want.data(), want);
    finish_transpose(got, words_got.data());
    if (words_got != words_want) return fail("words", name, n);
    std::vector<uint64_t> words_all(finish_words(n), ~0ull);
    uint64_t first = 0;
    if (finish_stream_host(orig.data(), n, words_all.data(), &first) != flag || words_all != words_want || first != want[0]) return fail("stream", name, n);
    printf("%s %u %u\n", name.c_str(), (unsigned)flag, worst);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plan") {
        for (int a = 2; a < argc; ++a) {
            const uint64_t n = strtoull(argv[a], nullptr, 10);
            printf("%llu %d %u %llu %llu %llu\n", (unsigned long long)n, finish_lds_form(n) ? 1 : 0, finish_threads(n),
                   (unsigned long long)finish_lds_bytes(n), (unsigned long long)finish_workgroups(5000, n), (unsigned long long)finish_words(n));
        }
        return 0;
    }
    if (mode == "consts") {
        printf("%llu %u %u %u %u\n", (unsigned long long)FINISH_LDS_BINS_MAX, FINISH_MAX_ATTEMPTS, FINISH_MAX_ROUNDS, finish_max_attempts(8),
               finish_max_attempts(0));
        return 0;
    }
    if (mode == "patterns" && argc == 3) {
        const size_t n = strtoull(argv[2], nullptr, 10);
        std::mt19937_64 rng(1234 + n);
        const std::vector<uint64_t> full = random_signs(n, rng);
        int bad = check("full", full);
        for (const auto &pos : {std::pair<const char *, size_t>{"single_first", 0}, {"single_middle", n / 2}, {"single_last", n - 1}}) {
            std::vector<uint64_t> v(n, FINISH_EMPTY);
            v[pos.second] = full[pos.second];
            bad |= check(pos.first, v);
        }
        {
            std::vector<uint64_t> v = full;
            v[0] = FINISH_EMPTY;
            bad |= check("bin0_empty", v);
            v = full;
            v[n - 1] = FINISH_EMPTY;
            bad |= check("last_empty", v);
            v = full;
            for (size_t i = 0; i < n / 2; ++i) v[i] = FINISH_EMPTY;
            bad |= check("first_half_empty", v);
            v = full;
            for (size_t i = n / 2; i < n; ++i) v[i] = FINISH_EMPTY;
            bad |= check("second_half_empty", v);
        }
        for (const auto &pc : {std::pair<const char *, unsigned>{"empty_1pct", 1}, {"empty_50pct", 50}, {"empty_99pct", 99}}) {
            std::vector<uint64_t> v = full;
            size_t left = 0;
            for (size_t i = 0; i < n; ++i) {
                if (rng() % 100 < pc.second) v[i] = FINISH_EMPTY; else ++left;
            }
            if (left == 0) v[n / 3] = full[n / 3];   // (never the all-empty stream: the sequential loop does not end on it)
            bad |= check(pc.first, v);
        }
        std::vector<uint64_t> none(n, FINISH_EMPTY), words(finish_words(n), ~0ull);
        uint64_t first = 0;
        if (finish_stream_host(none.data(), n, words.data(), &first) != FINISH_ALL_EMPTY || first != FINISH_EMPTY ||
            words != std::vector<uint64_t>(finish_words(n), 0)) {
            bad |= fail("all-empty", "all_empty", n);
        }
        return bad;
    }
    if (mode == "capped" && argc == 3) {
        std::vector<uint64_t> v = read_stdin();
        const std::vector<uint64_t> before = v;
        const uint8_t flag = finish_densify_two_step(v, (uint32_t)strtoul(argv[2], nullptr, 10));
        if ((flag & FINISH_UNFINISHED) && v != before) return 1;   // left untouched for the fall-back
        printf("%u\n", (unsigned)flag);
        return 0;
    }
    if (mode == "stream") {
        std::vector<uint64_t> v = read_stdin();
        const uint8_t flag = finish_densify_two_step(v);
        std::vector<uint64_t> words(finish_words(v.size()), 0);
        if (!(flag & FINISH_ALL_EMPTY)) finish_transpose(v, words.data());
        fwrite(&flag, 1, 1, stdout);
        fwrite(v.data(), sizeof(uint64_t), v.size(), stdout);
        fwrite(words.data(), sizeof(uint64_t), words.size(), stdout);
        return 0;
    }
    fprintf(stderr, "usage: finish_plan_check plan|consts|patterns|capped|stream ...\n");
    return 2;
}
