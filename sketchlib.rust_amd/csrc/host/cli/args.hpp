// args.hpp -- the one argument reader of the command line and its typed value readers (clap's messages, src/cli.rs).
// Header only and free of project headers: tests/native/cli_args_check.cpp drives it on its own.
//
// A usage error or a help request is THROWN (UsageError, HelpRequested); main.cpp alone turns them into the stderr block
// and the exit code, with the usage line the command handed it.
//
// Differences between the commands that are kept as they were, each a setting at the command's call site (harmonising
// one is a change of that setting plus a re-recorded tests/golden/generated/cli_usage.json):
//   * only `dist` splits --flag=value (Syntax::equals);
//   * only `dist` (-oFILE, -kN) and `merge` (-oFILE) take a value attached to a short option (Syntax::attached);
//   * `dist --threads` is strict (0, a sign or a letter is a usage error: threads_strict); every other --threads takes
//     max(1, n) (threads_lenient);
//   * `dist --completeness-cutoff` is strict (float_strict); `inverted precluster` takes strtod's reading, 0 for a word;
//   * a missing value names the flag as `dist` and the options with a fixed name do ('-k <KMER>', '-o <OUTPUT>'), or by the
//     bare argument as typed ('-k', '--device'): the name is the argument of ArgReader::value at every call;
//   * `inverted build | query | precluster` have no --help (it is an unknown flag there), `inverted --help` is an unknown
//     subcommand, and `inverted` alone reports its missing subcommand under the usage line of `dist`;
//   * `merge`, `delete` and `info` accept and ignore -v / --verbose / --quiet;
//   * -v after `dist` also turns on the closing "Complete in" line; after `inverted <sub>` it turns on the INFO lines only;
//   * `sketch`, `append`, `inverted build`: --gpu means device 0 and --device D means device D, the later one winning;
//     `inverted query`: --device names the device of the query, --gpu only moves the sketching there too;
//   * `inverted query` has no --single-strand (the index decides).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <initializer_list>
#include <optional>
#include <string>
#include <utility>
#include <vector>

namespace skl_cli {

struct UsageError {
    std::string message;
};
struct HelpRequested {};

// What a command's arguments may look like beyond `--flag value` and `-f value`.
struct Syntax {
    bool equals = false;          // --flag=value is split at the first '='
    const char *attached = "";    // the short options that take their value attached: -oFILE
};

[[noreturn]] inline void unexpected(const std::string &arg) { throw UsageError{"unexpected argument '" + arg + "' found"}; }

// argv[first..argc) one argument at a time:  while (r.next()) { if (r.is("-o")) out = r.value("-o <OUTPUT>"); ... }
class ArgReader {
  public:
    ArgReader(int argc, const char *const *argv, int first, Syntax syntax = {}) : argc_(argc), argv_(argv), i_(first - 1), syntax_(syntax) {}

    bool next()
    {
        if (++i_ >= argc_) return false;
        arg_ = argv_[i_];
        inline_.reset();
        if (syntax_.equals && arg_.rfind("--", 0) == 0) {
            const size_t eq = arg_.find('=');
            if (eq != std::string::npos) {
                inline_ = arg_.substr(eq + 1);
                arg_.resize(eq);
            }
        } else if (arg_.size() > 2 && arg_[0] == '-' && arg_[1] != '-' && std::string(syntax_.attached).find(arg_[1]) != std::string::npos) {
            inline_ = arg_.substr(2);
            arg_.resize(2);
        }
        return true;
    }
    const std::string &arg() const { return arg_; }   // (without its =value or attached value)
    bool is(const char *a, const char *b = nullptr) const { return arg_ == a || (b && arg_ == b); }
    bool is_help() const { return is("-h", "--help"); }
    bool is_option() const { return arg_.size() > 1 && arg_[0] == '-'; }
    [[noreturn]] void unexpected() const { skl_cli::unexpected(arg_); }
    // the value of the current flag; `shown` is how the flag is named when there is none
    std::string value(const std::string &shown)
    {
        if (inline_) return *inline_;
        if (i_ + 1 >= argc_) throw UsageError{"a value is required for '" + shown + "' but none was supplied"};
        return argv_[++i_];
    }

  private:
    int argc_;
    const char *const *argv_;
    int i_;
    Syntax syntax_;
    std::string arg_;
    std::optional<std::string> inline_;
};

[[noreturn]] inline void invalid_value(const std::string &flag, const std::string &v, const std::string &why)
{
    throw UsageError{"invalid value '" + v + "' for '" + flag + "'" + why};
}

// what strtoull reads to the end of the word, a leading '-' refused: a number past 2^64 - 1 reads as 2^64 - 1
inline size_t usize(const std::string &flag, const std::string &v)
{
    char *end = nullptr;
    if (v.empty() || v[0] == '-') invalid_value(flag, v, ": invalid digit found in string");
    const unsigned long long x = std::strtoull(v.c_str(), &end, 10);
    if (end != v.c_str() + v.size()) invalid_value(flag, v, ": invalid digit found in string");
    return (size_t)x;
}

// a u16 / u8 option as clap parses it: out of range is a usage error (more than 20 digits: whatever strtoull made of them)
inline size_t bounded(const std::string &flag, const std::string &v, size_t min, size_t max)
{
    const size_t x = usize(flag, v);
    if (x < min || x > max || v.size() > 20) invalid_value(flag, v, ": " + v + " is not in " + std::to_string(min) + "..=" + std::to_string(max));
    return x;
}

inline std::vector<size_t> list(const std::string &flag, const std::string &v)   // a,b,c: every element a usize
{
    std::vector<size_t> out;
    size_t pos = 0;
    while (pos <= v.size()) {
        const size_t comma = v.find(',', pos);
        out.push_back(usize(flag, v.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos)));
        if (comma == std::string::npos) break;
        pos = comma + 1;
    }
    return out;
}

inline size_t threads_strict(const std::string &flag, const std::string &v)
{
    char *end = nullptr;
    const long long t = std::strtoll(v.c_str(), &end, 10);
    if (v.empty() || end != v.c_str() + v.size()) invalid_value(flag, v, ": `" + v + "` isn't a valid number of cores");
    if (t < 1) invalid_value(flag, v, ": Threads must be one or higher");
    return (size_t)t;
}

inline size_t threads_lenient(const std::string &flag, const std::string &v) { return std::max<size_t>(1, usize(flag, v)); }

inline double float_strict(const std::string &flag, const std::string &v)
{
    char *end = nullptr;
    const double x = std::strtod(v.c_str(), &end);
    if (v.empty() || end != v.c_str() + v.size()) invalid_value(flag, v, ": invalid float literal");
    return x;
}

// the index of v among the choices; the two ways clap's messages list them
enum class ChoiceStyle { Inline /* ": possible values: a, b" */, Block /* "\n  [possible values: a, b]" */ };
inline size_t choice(const std::string &flag, const std::string &v, std::initializer_list<const char *> choices, ChoiceStyle style)
{
    std::string all;
    size_t i = 0;
    for (const char *c : choices) {
        if (v == c) return i;
        all += (i++ ? ", " : "") + std::string(c);
    }
    invalid_value(flag, v, style == ChoiceStyle::Inline ? ": possible values: " + all : "\n  [possible values: " + all + "]");
}

// {given?, name} in the order of the usage line: every one not given is listed, one error
inline void require(std::initializer_list<std::pair<bool, const char *>> args)
{
    std::string missing;
    for (const auto &a : args) {
        if (!a.first) missing += std::string("\n  ") + a.second;
    }
    if (!missing.empty()) throw UsageError{"the following required arguments were not provided:" + missing};
}

inline void conflict(const std::string &a, const std::string &b) { throw UsageError{"the argument '" + a + "' cannot be used with '" + b + "'"}; }

// --knn-ties <RULE> of `dist` and `inverted precluster`: true = canonical, false = reference
inline bool knn_ties_canonical(ArgReader &r)
{
    return choice("--knn-ties <RULE>", r.value("--knn-ties <RULE>"), {"canonical", "reference"}, ChoiceStyle::Inline) == 0;
}

// --level <LEVEL> of `sketch` and `append`: 1, 2 or 3
inline int aa_level(ArgReader &r)
{
    return 1 + (int)choice("--level <LEVEL>", r.value(r.arg()), {"level1", "level2", "level3"}, ChoiceStyle::Block);
}

// The input options of everything that sketches: `sketch`, `append`, `inverted build`, `inverted query`.
struct SketchInputArgs {
    explicit SketchInputArgs(bool takes_single_strand) : takes_single_strand(takes_single_strand) {}
    const bool takes_single_strand;
    std::vector<std::string> seq_files;   // the command's loop pushes its positional arguments here
    std::optional<std::string> file_list;
    uint16_t min_count = 5;   // DEFAULT_MINCOUNT / DEFAULT_MINQUAL, cli.rs:12-15 (read sets only)
    uint8_t min_qual = 20;    // (compared with the raw quality byte)
    size_t threads = 1;
    bool single_strand = false;
    int sketch_device = -1;   // the device to sketch on, -1 = the host: --gpu = 0, --device D = D, the later one winning
    bool gpu = false;         // `inverted query` reads these two instead: --gpu given; --device D, whether or not --gpu is
    int device = 0;

    bool accept(ArgReader &r)   // true: the current argument was one of the group's
    {
        if (r.is("-f")) file_list = r.value("-f <FILE_LIST>");
        else if (r.is("--min-count")) min_count = (uint16_t)bounded("--min-count <MIN_COUNT>", r.value(r.arg()), 0, 0xFFFF);
        else if (r.is("--min-qual")) min_qual = (uint8_t)bounded("--min-qual <MIN_QUAL>", r.value(r.arg()), 0, 0xFF);
        else if (r.is("--threads")) threads = threads_lenient("--threads <THREADS>", r.value(r.arg()));
        else if (r.is("--gpu")) { gpu = true; sketch_device = 0; }
        else if (r.is("--device")) sketch_device = device = (int)usize("--device <D>", r.value(r.arg()));
        else if (takes_single_strand && r.is("--single-strand")) single_strand = true;
        else return false;
        return true;
    }
    void check() const
    {
        if (seq_files.empty() == !file_list.has_value()) throw UsageError{"exactly one of <SEQ_FILES>... or -f <FILE_LIST> must be given"};
    }
};

}  // namespace skl_cli
