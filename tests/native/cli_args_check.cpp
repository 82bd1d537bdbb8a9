// cli_args_check.cpp -- csrc/host/cli/args.hpp on its own: the argument reader and every value reader over the edges of
// their input.  One line per case: <case><TAB><outcome>, the outcome being "ok ..." with what was read, "usage: <message>"
// (newlines as \n) or "help".  tests/test_cli_args_cpu.py holds the expected lines.
#include <cstdio>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

#include "args.hpp"

using namespace skl_cli;

namespace {

void report(const std::string &name, const std::function<std::string()> &fn)
{
    std::string outcome;
    try {
        outcome = "ok " + fn();
    } catch (const UsageError &u) {
        outcome = "usage: ";
        for (const char c : u.message) outcome += c == '\n' ? std::string("\\n") : std::string(1, c);
    } catch (const HelpRequested &) {
        outcome = "help";
    }
    std::printf("%s\t%s\n", name.c_str(), outcome.c_str());
}

// the walk of a command's loop: every argument as the reader shows it; the flags in `valued` take a value
std::string walk(std::vector<const char *> argv, Syntax syntax, std::initializer_list<const char *> valued = {})
{
    // (a copy of exactly argc pointers on the heap: reading argv[argc] is an AddressSanitizer report)
    ArgReader r((int)argv.size(), argv.data(), 0, syntax);
    std::string out;
    while (r.next()) {
        if (r.is_help()) throw HelpRequested{};
        bool takes = false;
        for (const char *f : valued) takes = takes || r.is(f);
        out += "[" + r.arg() + (r.is_option() ? " option" : " word");
        if (takes) out += " = '" + r.value(r.arg() + " <V>") + "'";
        out += "]";
    }
    return out;
}

std::string n(size_t x) { return std::to_string((unsigned long long)x); }

std::string inputs(std::vector<const char *> argv, bool takes_single_strand)
{
    SketchInputArgs in(takes_single_strand);
    ArgReader r((int)argv.size(), argv.data(), 0);
    while (r.next()) {
        if (in.accept(r)) continue;
        if (r.is_option()) r.unexpected();
        in.seq_files.push_back(r.arg());
    }
    in.check();
    return "files=" + n(in.seq_files.size()) + " list=" + in.file_list.value_or("-") + " min_count=" + n(in.min_count) + " min_qual=" + n(in.min_qual) +
           " threads=" + n(in.threads) + " single_strand=" + n(in.single_strand) + " sketch_device=" + std::to_string(in.sketch_device) +
           " gpu=" + n(in.gpu) + " device=" + std::to_string(in.device);
}

}  // namespace

int main()
{
    const Syntax plain{}, equals{true, ""}, attached_o{false, "o"}, dist{true, "ok"};
    // ---- the reader ----
    report("reader/empty", [&] { return walk({}, plain); });
    report("reader/words", [&] { return walk({"a", "-", "-x", "--y", ""}, plain); });
    report("reader/flag-last", [&] { return walk({"a", "--knn"}, plain, {"--knn"}); });
    report("reader/value-detached", [&] { return walk({"-o", "file", "b"}, plain, {"-o"}); });
    report("reader/value-is-a-flag", [&] { return walk({"-o", "--knn", "b"}, plain, {"-o", "--knn"}); });
    report("reader/equals-empty", [&] { return walk({"--x="}, equals, {"--x"}); });
    report("reader/equals-value", [&] { return walk({"--x=a=b", "c"}, equals, {"--x"}); });
    report("reader/equals-on-a-switch", [&] { return walk({"--x=1"}, equals); });
    report("reader/equals-off", [&] { return walk({"--x=a"}, plain, {"--x"}); });
    report("reader/equals-short", [&] { return walk({"-x=a"}, equals, {"-x"}); });
    report("reader/attached", [&] { return walk({"-ofile", "b"}, attached_o, {"-o"}); });
    report("reader/attached-detached", [&] { return walk({"-o", "file", "b"}, attached_o, {"-o"}); });
    report("reader/attached-last", [&] { return walk({"-o"}, attached_o, {"-o"}); });
    report("reader/attached-other-letter", [&] { return walk({"-kx"}, attached_o, {"-k"}); });
    report("reader/attached-off", [&] { return walk({"-ofile"}, plain, {"-o"}); });
    report("reader/attached-long", [&] { return walk({"--ofile"}, attached_o, {"-o"}); });
    report("reader/dist-syntax", [&] { return walk({"-k21", "-ofile", "--knn=5", "-k", "31", "--knn", "6", "-k="}, dist, {"-k", "-o", "--knn"}); });
    report("reader/help", [&] { return walk({"a", "--help"}, plain); });
    report("reader/help-short", [&] { return walk({"-h"}, plain); });
    report("reader/unexpected", [&]() -> std::string { unexpected("--frob"); });
    // ---- usize ----
    for (const char *v : {"0", "7", "9999999999999999999", "18446744073709551615", "18446744073709551616", "999999999999999999999", "",
                          "-1", "-", "+1", " 1", "1 ", "1x", "x", "3.5", "0x10"}) {
        report(std::string("usize/") + v, [&] { return n(usize("--knn <KNN>", v)); });
    }
    // ---- bounded ----
    for (const char *v : {"0", "65535", "65536", "00000000000000000001", "000000000000000000001", "18446744073709551615",
                          "18446744073709551616", "-1", "x", ""}) {
        report(std::string("bounded-u16/") + v, [&] { return n(bounded("--min-count <MIN_COUNT>", v, 0, 0xFFFF)); });
    }
    for (const char *v : {"255", "256"}) report(std::string("bounded-u8/") + v, [&] { return n(bounded("--min-qual <MIN_QUAL>", v, 0, 0xFF)); });
    for (const char *v : {"0", "1", "1024", "1025", "99999999999999999999999"}) {
        report(std::string("bounded-top/") + v, [&] { return n(bounded("--top <N>", v, 1, 1024)); });
    }
    // ---- list ----
    for (const char *v : {"7", "1,2,3", "17,31,4", "1,,2", "", ",", "1,", ",1", "1,x", "1,-2", "18446744073709551616,0"}) {
        report(std::string("list/") + v, [&] {
            std::string out;
            for (const size_t x : list("--k-vals <K_VALS>", v)) out += (out.empty() ? "" : " ") + n(x);
            return out;
        });
    }
    // ---- threads ----
    for (const char *v : {"1", "4", "0", "-2", "x", "", "1x", "+3", "99999999999999999999999"}) {
        report(std::string("threads-strict/") + v, [&] { return n(threads_strict("--threads <THREADS>", v)); });
        report(std::string("threads-lenient/") + v, [&] { return n(threads_lenient("--threads <THREADS>", v)); });
    }
    // ---- float ----
    for (const char *v : {"0.5", "1e-3", "1", "-0.25", "x", "", "0.5x", "inf"}) {
        report(std::string("float/") + v, [&] {
            char buf[32];
            std::snprintf(buf, sizeof buf, "%g", float_strict("--completeness-cutoff <COMPLETENESS_CUTOFF>", v));
            return std::string(buf);
        });
    }
    // ---- choices ----
    for (const char *v : {"canonical", "reference", "Canonical", ""}) {
        report(std::string("choice-inline/") + v, [&] { return n(choice("--knn-ties <RULE>", v, {"canonical", "reference"}, ChoiceStyle::Inline)); });
    }
    for (const char *v : {"match-count", "any-bins", "some-bins", ""}) {
        report(std::string("choice-block/") + v,
               [&] { return n(choice("--query-type <QUERY_TYPE>", v, {"match-count", "all-bins", "any-bins"}, ChoiceStyle::Block)); });
    }
    report("choice/one", [&] { return n(choice("--x <X>", "b", {"a"}, ChoiceStyle::Inline)); });
    // ---- required, conflicts ----
    report("require/all-given", [&] { require({{true, "<DB1>"}, {true, "<DB2>"}}); return std::string(); });
    report("require/second", [&] { require({{true, "<DB1>"}, {false, "<DB2>"}}); return std::string(); });
    report("require/all-three", [&] { require({{false, "<DB>"}, {false, "<SAMPLES>"}, {false, "<OUTPUT_FILE>"}}); return std::string(); });
    report("require/none-listed", [&] { require({}); return std::string(); });
    report("conflict", [&]() -> std::string { conflict("--pairs <FILE>", "--knn <KNN>"); return ""; });
    // ---- --knn-ties, --level ----
    for (std::vector<const char *> argv : {std::vector<const char *>{"--knn-ties", "canonical"}, {"--knn-ties", "reference"}, {"--knn-ties", "x"}, {"--knn-ties"},
                                            {"--knn-ties=canonical"}}) {
        report("knn-ties/" + std::string(argv.size() > 1 ? argv[1] : argv[0]), [&] {
            ArgReader r((int)argv.size(), argv.data(), 0, dist);
            r.next();
            return n(knn_ties_canonical(r));
        });
    }
    for (std::vector<const char *> argv : {std::vector<const char *>{"--level", "level1"}, {"--level", "level2"}, {"--level", "level3"}, {"--level", "level4"},
                                            {"--level", "3"}, {"--level"}}) {
        report("level/" + std::string(argv.size() > 1 ? argv[1] : "none"), [&] {
            ArgReader r((int)argv.size(), argv.data(), 0);
            r.next();
            return std::to_string(aa_level(r));
        });
    }
    // ---- the sketch input group ----
    report("inputs/neither", [&] { return inputs({}, true); });
    report("inputs/files", [&] { return inputs({"a.fa", "b.fa"}, true); });
    report("inputs/list", [&] { return inputs({"-f", "rfile.txt"}, true); });
    report("inputs/both", [&] { return inputs({"-f", "rfile.txt", "a.fa"}, true); });
    report("inputs/all-options", [&] { return inputs({"a.fa", "--min-count", "65535", "--min-qual", "255", "--threads", "0", "--single-strand"}, true); });
    report("inputs/gpu-then-device", [&] { return inputs({"a.fa", "--gpu", "--device", "2"}, true); });
    report("inputs/device-then-gpu", [&] { return inputs({"a.fa", "--device", "2", "--gpu"}, true); });
    report("inputs/device-alone", [&] { return inputs({"a.fa", "--device", "3"}, false); });
    report("inputs/no-single-strand", [&] { return inputs({"a.fa", "--single-strand"}, false); });
    report("inputs/min-count-over", [&] { return inputs({"a.fa", "--min-count", "65536"}, true); });
    report("inputs/min-qual-over", [&] { return inputs({"a.fa", "--min-qual", "256"}, true); });
    report("inputs/value-missing-f", [&] { return inputs({"a.fa", "-f"}, true); });
    report("inputs/value-missing-device", [&] { return inputs({"a.fa", "--device"}, true); });
    report("inputs/unknown", [&] { return inputs({"a.fa", "--k-vals"}, true); });
    return 0;
}
