// common.cpp -- see common.hpp
#include "common.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <mutex>
#include <thread>

#include "sketchlib_dist.h"

namespace skl_cli {

const char *const LOG_UNMATCHED_WARNING =
    "this host's libm log() is neither form of glibc's x86-64 log the GPU reproduces bit for bit: with a completeness "
    "correction, core distances of flat fits (the same bin-match count at every k-mer length) may be 0 where a CPU run "
    "of sketchlib on this host prints 1, or the reverse; all other values agree to 1e-6";

void warn_if_log_unmatched(const Logger &log, skl_ctx *ctx)
{
    if (skl_ctx_flags(ctx) & SKL_CTX_FLAG_LOG_UNMATCHED) log.warn(LOG_UNMATCHED_WARNING);
}

std::unique_ptr<TextSink> open_sink(const std::optional<std::string> &output)
{
    if (!output) return std::make_unique<StreamSink>(std::cout);
    try {
        return std::make_unique<FileSink>(*output);
    } catch (const std::exception &e) {
        throw Panic(e.what());
    }
}

void parallel_for_index(size_t n, size_t threads, const std::function<void(size_t)> &fn)
{
    std::atomic<size_t> next{0};
    std::exception_ptr err;
    std::mutex mu;
    auto work = [&] {
        try {
            for (size_t i; (i = next.fetch_add(1)) < n;) fn(i);
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu);
            if (!err) err = std::current_exception();
        }
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    if (err) std::rethrow_exception(err);
}

std::future<std::unique_ptr<Device>> start_device(int device)
{
    return std::async(std::launch::async, [device] { return std::make_unique<Device>(device); });
}

std::future<std::unique_ptr<DeviceSet>> start_devices(const std::vector<int> &devices)
{
    return std::async(std::launch::async, [devices] { return std::make_unique<DeviceSet>(devices); });
}

// The listing is complete and flushed: leave without tearing down what the operating system reclaims anyway -- the slabs
// in HBM, gigabytes of host vectors, the worker pool, the HIP runtime (0.05 s of a 0.19 s run on 1 000 genomes, 0.5 s
// after a million).  Files are written with pwrite (nothing buffered in the process); SKL_CLI_FAST_EXIT=0 keeps the
// orderly exit.
// (called by main() AFTER its last line of output -- the verbose "Complete in" line -- with the command's exit code; a
// failed flush of the listing (ENOSPC, EPIPE) turns a success into exit code 1 and takes the orderly way out)
bool g_listing_complete = false;

int leave_after_success(int rc)
{
    std::cout.flush();
    std::cerr.flush();
    const bool flushed = std::cout.good() && fflush(nullptr) == 0;
    if (!flushed) {
        std::fprintf(stderr, "Error: writing the output failed\n");
        return rc ? rc : 1;
    }
    if (rc != 0 || !g_listing_complete) return rc;
    const char *e = std::getenv("SKL_CLI_FAST_EXIT");
    if (e && e[0] == '0') return rc;
    // a profiler or another preloaded tool writes its results from exit handlers: leave in order for it
    for (const char *tool : {"LD_PRELOAD", "HSA_TOOLS_LIB", "ROCP_TOOL_LIBRARIES", "ROCPROFILER_REGISTER_FORCE_LOAD"}) {
        const char *v = std::getenv(tool);
        if (v && v[0]) return rc;
    }
    std::_Exit(0);
}

}  // namespace skl_cli
