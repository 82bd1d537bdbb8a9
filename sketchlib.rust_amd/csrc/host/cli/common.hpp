// common.hpp -- what the commands of the CLI share besides the argument reader (args.hpp): logging, the output sink, phase
// times, a thread pool over an index range, the device start beside the file loading, and the way out after a listing.
#pragma once

#include <chrono>
#include <cstdlib>
#include <functional>
#include <future>
#include <iostream>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "../distances.hpp"
#include "../io.hpp"
#include "args.hpp"

namespace skl_cli {

using namespace skl_host;

// global -v / --verbose / --quiet, given before the command (main.cpp) or, where a command takes them, after it
struct Verbosity {
    bool verbose = false, quiet = false;
    bool accept(const ArgReader &r)
    {
        if (r.is("-v", "--verbose")) verbose = true;
        else if (r.is("--quiet")) quiet = true;
        else return false;
        return true;
    }
    bool info() const { return verbose && !quiet; }
};

// A command: its arguments are argv[first..argc); `usage` is its line of main.cpp's table, for its help text.  Returns the
// exit code; throws UsageError / HelpRequested / Panic / std::exception, all of them caught in main.cpp alone.
using Command = int (*)(int argc, char **argv, int first, Verbosity &v, const char *usage);

int run_dist(int, char **, int, Verbosity &, const char *);
int run_sketch(int, char **, int, Verbosity &, const char *);
int run_append(int, char **, int, Verbosity &, const char *);
int run_merge(int, char **, int, Verbosity &, const char *);
int run_delete(int, char **, int, Verbosity &, const char *);
int run_info(int, char **, int, Verbosity &, const char *);
int run_inverted_build(int, char **, int, Verbosity &, const char *);
int run_inverted_query(int, char **, int, Verbosity &, const char *);
int run_inverted_precluster(int, char **, int, Verbosity &, const char *);

// lib.rs:230-237: verbose -> Info, quiet -> Error, default -> Warn
struct Logger {
    explicit Logger(const Verbosity &v) : info_on(v.info()), warn_on(!v.quiet) {}
    bool info_on, warn_on;
    void info(const std::string &m) const { if (info_on) std::cerr << "INFO  [sketchlib] " << m << "\n"; }
    void warn(const std::string &m) const { if (warn_on) std::cerr << "WARN  [sketchlib] " << m << "\n"; }
};

// skl_ctx_flags() & SKL_CTX_FLAG_LOG_UNMATCHED, warned of once by the commands that apply a completeness correction
extern const char *const LOG_UNMATCHED_WARNING;
void warn_if_log_unmatched(const Logger &log, skl_ctx *ctx);

// Listings go through a TextSink: the named file (blocks written at offsets from all formatting threads), else stdout
// (in order).  A file that cannot be opened is a Panic.
std::unique_ptr<TextSink> open_sink(const std::optional<std::string> &output);

// Seconds since the command began its work; `report`: SKL_CLI_TIMING asks for the command's TIMING line on stderr.
struct Stopwatch {
    const bool report = std::getenv("SKL_CLI_TIMING") != nullptr;
    const std::chrono::steady_clock::time_point start = std::chrono::steady_clock::now();
    double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count(); }
};

// fn(i) for every i in [0, n), handed out one at a time to `threads` threads (the caller is one of them); the first
// exception any of them met is rethrown once all have stopped.
void parallel_for_index(size_t n, size_t threads, const std::function<void(size_t)> &fn);

// The device contexts (HIP runtime start, stream, first allocations: 0.1-0.25 s) come up on their own thread while the
// files are read; whatever goes wrong there is reported by get(), where the context is first needed, after the loading errors.
std::future<std::unique_ptr<Device>> start_device(int device);
std::future<std::unique_ptr<DeviceSet>> start_devices(const std::vector<int> &devices);

// Set by a command once its listing is written; leave_after_success(rc) is main()'s way out after its last line of output.
extern bool g_listing_complete;
int leave_after_success(int rc);

}  // namespace skl_cli
