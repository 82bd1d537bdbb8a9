// aa_check -- stand-alone checks of the amino-acid sketcher's host code (csrc/host/aahash.cpp) and of the work plan of its GPU
// call (csrc/aa_plan.hpp), built with the host compiler alone (no ROCm include path, never loads the library); also the
// program the sanitizer run compiles with -fsanitize=address,undefined (tests/test_aa_native_cpu.py).
//
//   aa_check plan <k> <long_min> <len>...        every window start of every sample covered exactly once by the items of the
//                                                two forms, items inside their samples, batches whole and within their caps;
//                                                prints "ok <starts checked>"
//   aa_check signs <level> <k> <bins> <concat> <fasta>...   per sample "name<TAB>len<TAB>invalid<TAB>sign,sign,..." (undensified,
//                                                bin minima of the CPU path; "none" where no window is hashed)
//   aa_check sketch <prefix> <level> <concat> <sketch_size> <k,k,...> <fasta>...   the CPU path end to end (sketch_files)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../sketchlib.rust_amd/csrc/aa_plan.hpp"
#include "../../sketchlib.rust_amd/csrc/host/aahash.hpp"

using namespace skl_host;

static int check_plan(int argc, char **argv)
{
    const size_t k = (size_t)atoll(argv[2]);
    const uint64_t long_min = (uint64_t)atoll(argv[3]);
    std::vector<uint64_t> res_begin{0};
    for (int i = 4; i < argc; ++i) res_begin.push_back(res_begin.back() + (uint64_t)atoll(argv[i]));
    const size_t n = res_begin.size() - 1;
    const skl::AaPlan plan = skl::aa_plan(res_begin.data(), n, k, long_min);
    std::vector<std::vector<uint8_t>> seen(n);
    for (size_t s = 0; s < n; ++s) seen[s].assign((size_t)(res_begin[s + 1] - res_begin[s]), 0);
    auto mark = [&](const skl::AaItem &it) {
        if (it.sample >= n) throw std::runtime_error("item of no sample");
        if (it.count && it.first + it.count > seen[it.sample].size()) throw std::runtime_error("item past its sample");
        for (uint32_t j = 0; j < it.count; ++j) {
            if (seen[it.sample][it.first + j]++) throw std::runtime_error("window start covered twice");
        }
    };
    for (uint64_t t = 0; t < plan.span_begin[n]; ++t) {
        const skl::AaItem it = skl::aa_short_item(plan.span_begin.data(), res_begin.data(), (uint32_t)n, plan.short_span, t);
        if (it.count == 0) throw std::runtime_error("idle thread in the unstaged form");   // packed: no padding
        mark(it);
    }
    for (uint64_t wg = 0; wg < plan.wg_begin[n]; ++wg) {
        for (uint32_t tid = 0; tid < skl::AA_WG_LDS; ++tid) mark(skl::aa_long_item(plan.wg_begin.data(), res_begin.data(), (uint32_t)n, wg, tid));
    }
    uint64_t checked = 0;
    for (size_t s = 0; s < n; ++s) {
        const bool staged = plan.wg_begin[s + 1] != plan.wg_begin[s], unstaged = plan.span_begin[s + 1] != plan.span_begin[s];
        if (staged && unstaged) throw std::runtime_error("a sample in both forms");
        if (staged && (k > skl::AA_K_STAGED_MAX || seen[s].size() < long_min)) throw std::runtime_error("staged against the rule");
        for (uint8_t c : seen[s]) {
            if (c != 1) throw std::runtime_error("window start not covered");
            ++checked;
        }
    }
    // batches: whole samples, in order, each within the caps unless it is a single sample
    for (uint64_t cap : {uint64_t(1), uint64_t(3 * 8 * 64), uint64_t(1) << 40}) {
        const std::vector<size_t> cuts = skl::aa_batches(res_begin.data(), n, 1, 64, cap, 1000);
        if (cuts.front() != 0 || cuts.back() != n) throw std::runtime_error("batches do not span the samples");
        for (size_t b = 0; b + 1 < cuts.size(); ++b) {
            const size_t m = cuts[b + 1] - cuts[b];
            if (n && m == 0) throw std::runtime_error("empty batch");
            if (m > 1 && (m * 8 * 64 > cap || res_begin[cuts[b + 1]] - res_begin[cuts[b]] > 1000)) throw std::runtime_error("batch past its cap");
        }
    }
    std::printf("ok %llu\n", (unsigned long long)checked);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc >= 4 && !strcmp(argv[1], "plan")) return check_plan(argc, argv);
        if (argc >= 7 && !strcmp(argv[1], "signs")) {
            const int level = atoi(argv[2]);
            const size_t k = (size_t)atoll(argv[3]);
            const uint64_t bins = (uint64_t)atoll(argv[4]);
            const bool concat = atoi(argv[5]) != 0;
            std::vector<std::string> files(argv + 6, argv + argc);
            for (const AaSample &a : load_aa_samples({"s", files}, concat)) {
                std::vector<uint64_t> signs((size_t)bins, UINT64_MAX);
                const bool any = aa_bin_minima(a.codes.data(), a.codes.size(), k, level, true, signs.data(), bins);
                std::cout << a.name << "\t" << a.codes.size() << "\t" << a.invalid << "\t";
                if (!any) std::cout << "none";
                for (size_t b = 0; any && b < signs.size(); ++b) std::cout << (b ? "," : "") << signs[b];
                std::cout << "\n";
            }
            return 0;
        }
        if (argc >= 8 && !strcmp(argv[1], "sketch")) {
            SeqType st;
            st.aa = true;
            st.level = atoi(argv[3]);
            st.concat_fasta = atoi(argv[4]) != 0;
            std::vector<size_t> kmers;
            for (char *tok = strtok(argv[6], ","); tok; tok = strtok(nullptr, ",")) kmers.push_back((size_t)atoll(tok));
            std::vector<std::string> files(argv + 7, argv + argc);
            const MultiSketch m = sketch_files(argv[2], {{"s", files}}, kmers, (uint64_t)atoll(argv[5]), true, 2, 5, 20, st);
            std::printf("ok %zu\n", m.metadata().size());
            return 0;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
    std::fprintf(stderr, "usage: aa_check plan|signs|sketch ...\n");
    return 2;
}
