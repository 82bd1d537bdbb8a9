// inv_top_check -- csrc/inv_top_plan.hpp on the CPU (tests/test_inv_top_plan_cpu.py builds it with the host compiler and
// -fsanitize=address,undefined and runs it directly): inv_top_select_host(), which follows the kernel's digit walk, chunked
// descending collect and bitonic network, against a plain sort of the u64 keys (count << 32) | index.
//
//   inv_top_check plan S w top ...   one line per triple: S w top digits list_len lds_bytes
//   inv_top_check consts             INV_TOP_MAX INV_TOP_THREADS INV_TOP_DIGIT_BITS width(knob 0) width(3) width(12) width(-1)
//   inv_top_check grid               the whole grid below; prints "ok <cases>" or the first difference (exit 1)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "inv_top_plan.hpp"

using namespace skl;

namespace {

const char *const KINDS[] = {"random", "all_equal", "two_valued", "threshold_0"};

std::vector<uint32_t> make_row(int kind, uint32_t n, uint32_t S, uint32_t top, std::mt19937_64 &rng)
{
    std::vector<uint32_t> row(n);
    auto below = [&](uint64_t m) { return (uint32_t)(rng() % m); };
    switch (kind) {
    case 0:
        for (auto &c : row) c = below((uint64_t)S + 1);
        break;
    case 1: {
        const uint32_t v = below(3) == 0 ? S : below((uint64_t)S + 1);
        std::fill(row.begin(), row.end(), v);
        break;
    }
    case 2: {
        const uint32_t lo = below(S), hi = lo + 1 + below(S - lo);   // lo < hi <= S
        for (auto &c : row) c = below(2) ? hi : lo;
        break;
    }
    default: {   // fewer non-zero entries than hits asked for: the threshold is 0 and the list is filled from the highest indices
        const uint32_t n_eff = inv_top_n_eff(top, n);
        const uint32_t k = below(n_eff);   // 0 .. n_eff - 1
        for (uint32_t i = 0; i < k; ++i) row[below(n)] = 1 + below(S);
        break;
    }
    }
    return row;
}

int grid()
{
    const uint32_t NS[] = {1, 63, 64, 255, 256, 257, 700}, SS[] = {1, 10, 1000, 2047, 2048, 5000}, WS[] = {1, 3, 8, 11};
    std::mt19937_64 rng(20240607);
    size_t cases = 0;
    for (uint32_t n : NS) {
        const uint32_t TOPS[] = {1, 2, 64, n, n + 3, 1024};
        for (uint32_t S : SS) {
            for (uint32_t top : TOPS) {
                for (int kind = 0; kind < 4; ++kind) {
                    const std::vector<uint32_t> row = make_row(kind, n, S, top, rng);
                    const uint32_t n_eff = inv_top_n_eff(top, n);
                    std::vector<uint64_t> keys(n);
                    for (uint32_t i = 0; i < n; ++i) keys[i] = ((uint64_t)row[i] << 32) | i;
                    std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
                    const uint32_t t = (uint32_t)(keys[n_eff - 1] >> 32);
                    const uint32_t g = (uint32_t)std::count_if(row.begin(), row.end(), [&](uint32_t c) { return c > t; });
                    for (uint32_t w : WS) {
                        std::vector<uint32_t> ids(top, 7u), counts(top, 7u);
                        InvTopThreshold thr{0, 0, 0};
                        inv_top_select_host(row.data(), n, S, w, top, ids.data(), counts.data(), &thr);
                        ++cases;
                        bool ok = thr.t == t && thr.g == g && thr.e == n_eff - g && thr.e >= 1;
                        for (uint32_t r = 0; r < top && ok; ++r) {
                            ok = r < n_eff ? ids[r] == (uint32_t)keys[r] && counts[r] == (uint32_t)(keys[r] >> 32)
                                           : ids[r] == 0xFFFFFFFFu && counts[r] == 0u;
                        }
                        if (!ok) {
                            std::printf("MISMATCH n=%u S=%u w=%u top=%u kind=%s: threshold (%u %u %u), expected (%u %u %u)\n", n, S, w, top,
                                        KINDS[kind], thr.t, thr.g, thr.e, t, g, n_eff - g);
                            return 1;
                        }
                    }
                }
            }
        }
    }
    // an empty row is all padding
    uint32_t ids[3] = {1, 1, 1}, counts[3] = {1, 1, 1};
    inv_top_select_host(nullptr, 0, 10, 11, 3, ids, counts);
    for (int r = 0; r < 3; ++r) {
        if (ids[r] != 0xFFFFFFFFu || counts[r] != 0u) {
            std::printf("MISMATCH empty row\n");
            return 1;
        }
    }
    // the walk's mapping: chunk c, lane l reads n - 1 - (256 c + l), every index exactly once, descending
    for (uint32_t n : NS) {
        uint32_t expect = n;
        for (uint32_t c = 0; c < inv_top_chunks(n); ++c) {
            for (uint32_t l = 0; l < INV_TOP_THREADS && inv_top_walk_live(n, c, l); ++l) {
                if (inv_top_walk_index(n, c, l) != --expect) {
                    std::printf("MISMATCH walk n=%u chunk=%u lane=%u\n", n, c, l);
                    return 1;
                }
            }
        }
        if (expect != 0 || inv_top_walk_live(n, inv_top_chunks(n), 0)) {
            std::printf("MISMATCH walk n=%u does not end at index 0\n", n);
            return 1;
        }
    }
    std::printf("ok %zu\n", cases);
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "grid") == 0) return grid();
    if (argc >= 2 && strcmp(argv[1], "consts") == 0) {
        std::printf("%u %u %u %u %u %u %u\n", INV_TOP_MAX, INV_TOP_THREADS, INV_TOP_DIGIT_BITS, inv_top_digit_bits(0), inv_top_digit_bits(3),
                    inv_top_digit_bits(12), inv_top_digit_bits(-1));
        return 0;
    }
    if (argc >= 5 && strcmp(argv[1], "plan") == 0 && (argc - 2) % 3 == 0) {
        for (int i = 2; i + 2 < argc; i += 3) {
            const uint32_t S = (uint32_t)strtoul(argv[i], nullptr, 10), w = (uint32_t)strtoul(argv[i + 1], nullptr, 10),
                           top = (uint32_t)strtoul(argv[i + 2], nullptr, 10);
            std::printf("%u %u %u %u %u %u\n", S, w, top, inv_top_digits(S, w), inv_top_list_len(top), inv_top_lds_bytes(top, w));
        }
        return 0;
    }
    std::fprintf(stderr, "usage: inv_top_check grid | consts | plan S w top ...\n");
    return 2;
}
