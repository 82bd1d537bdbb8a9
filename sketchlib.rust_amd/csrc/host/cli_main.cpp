// cli_main.cpp -- `sketchlib dist`, the reference's command line for this path
// (src/cli.rs:185-231, src/lib.rs:303-453) on top of the gfx950 engine.
//
// Same positional arguments, flags, defaults, stdout format and exit behaviour
// (panic -> 101, error -> 1, usage -> 2).  `--threads` (default 1, as in the reference) sets
// the host threads that format the dense text output; the distances themselves run on the
// GPU.  `--device` is the one addition.
#include <atomic>
#include <charconv>
#include <mutex>
#include <future>
#include <thread>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <algorithm>
#include <iostream>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "dbmaint.hpp"
#include "distances.hpp"
#include "inverted.hpp"
#include "sketchlib_dist.h"
#include "io.hpp"
#include "multisketch.hpp"
#include "sketch.hpp"

using namespace skl_host;

namespace {

struct DistArgs {
    std::string ref_db;
    std::optional<std::string> query_db, output, subset, ref_completeness_file, query_completeness_file;
    std::optional<std::string> pairs;   // --pairs <FILE>: distances of the listed pairs only
    std::optional<std::string> multi_device_flag;   // "--gpus <N>" / "--devices <LIST>" as given
    std::optional<size_t> knn, kmer;
    int knn_ties = SKL_KNN_TIES_REFERENCE;
    bool ani = false;
    size_t threads = 1;
    double completeness_cutoff = 0.64;
    bool verbose = false, quiet = false;
    std::vector<int> devices = {0};   // --device D | --devices a,b,.. | --gpus N
    bool npy = false;                  // --npy: dense output as a NumPy .npy array instead of text
    size_t band_bytes = 0;             // --band-mb: host memory per streamed output band (0: default)
    size_t band() const
    {
        // finer-than-MB override, for tests that want many bands on a small database
        if (const char *e = std::getenv("SKL_DIST_BAND_BYTES")) return std::max<size_t>(1, std::strtoull(e, nullptr, 10));
        // default: 256 MB, and at least 8 MB per output thread (a band is a barrier for the workers that format it)
        return band_bytes ? band_bytes : std::max<size_t>(256ull << 20, threads * (8ull << 20));
    }
};

const char *g_usage = "sketchlib dist [OPTIONS] <REF_DB> [QUERY_DB]";

[[noreturn]] void usage_error(const std::string &msg)
{
    std::cerr << "error: " << msg << "\n\n"
              << "Usage: " << g_usage << "\n\n"
              << "For more information, try '--help'.\n";
    std::exit(2);
}

void print_help()
{
    std::cout <<
        "Calculate pairwise distances using sketches\n\n"
        "Usage: sketchlib dist [OPTIONS] <REF_DB> [QUERY_DB]\n\n"
        "Arguments:\n"
        "  <REF_DB>    The .skm file used as the reference\n"
        "  [QUERY_DB]  The .skm file used as the query (omit for ref v ref)\n\n"
        "Options:\n"
        "  -o <OUTPUT>                     Output filename (omit to output to stdout)\n"
        "      --knn <KNN>                 Calculate sparse distances with k nearest-neighbours (ref-vs-ref or ref-vs-query)\n"
        "      --knn-ties <RULE>           Neighbours at EQUAL distance: reference (default) = exactly the ids and order\n"
        "                                  the reference binary prints (its BinaryHeap replayed on the GPU);\n"
        "                                  canonical = lowest index first (a property of the data alone; the distances\n"
        "                                  per row are the reference's, tied rows may list other ids).  Either rule\n"
        "                                  evaluates every pair once on any number of GPUs\n"
        "      --subset <SUBSET>           Sample names to analyse\n"
        "      --pairs <FILE>              Only the distances of the sample pairs listed in FILE: one pair per line,\n"
        "                                  name1<TAB>name2 (further columns ignored: the output of `dist --knn` is a valid\n"
        "                                  pairs file); both names from REF_DB, or name1 from REF_DB and name2 from\n"
        "                                  QUERY_DB.  One output line per input pair, in input order\n"
        "  -k <KMER>                       K-mer length (if provided only calculate Jaccard distance)\n"
        "      --ani                       Calculate ANI rather than Jaccard dists, using Poisson model\n"
        "      --threads <THREADS>         Number of CPU threads [default: 1]\n"
        "      --ref-completeness-file <F> File listing reference sample completeness estimates 0.0-1.0\n"
        "      --query-completeness-file <F> File listing query sample completeness estimates 0.0-1.0\n"
        "      --completeness-cutoff <C>   minimum completeness product for the correction [default: 0.64]\n"
        "      --device <D>                GPU to run on [default: 0]\n"
        "      --npy                       Dense output as a NumPy .npy array (f32, one row per pair in the\n"
        "                                  order of the text lines) instead of text; needs -o\n"
        "      --band-mb <MB>              Host memory per streamed dense output band [default: 256, and at least 8 per thread]\n"
        "      --gpus <N>                  Split the pair space over GPUs 0..N-1 (row bands)\n"
        "      --devices <LIST>            Same, with an explicit comma separated device list\n"
        "  -v, --verbose                   Show progress messages\n"
        "      --quiet                     Don't show any messages\n"
        "  -h, --help                      Print help\n";
}

size_t parse_usize(const std::string &flag, const std::string &v)
{
    char *end = nullptr;
    if (v.empty() || v[0] == '-') usage_error("invalid value '" + v + "' for '" + flag + "': invalid digit found in string");
    const unsigned long long x = std::strtoull(v.c_str(), &end, 10);
    if (end != v.c_str() + v.size()) usage_error("invalid value '" + v + "' for '" + flag + "': invalid digit found in string");
    return (size_t)x;
}

DistArgs parse_dist(int argc, char **argv, int first)
{
    DistArgs a;
    std::vector<std::string> positional;
    for (int i = first; i < argc; ++i) {
        std::string arg = argv[i];
        std::optional<std::string> inline_val;
        if (arg.rfind("--", 0) == 0) {
            const size_t eq = arg.find('=');
            if (eq != std::string::npos) {
                inline_val = arg.substr(eq + 1);
                arg = arg.substr(0, eq);
            }
        }
        auto value = [&](const std::string &flag) -> std::string {
            if (inline_val) return *inline_val;
            if (i + 1 >= argc) usage_error("a value is required for '" + flag + "' but none was supplied");
            return argv[++i];
        };
        if (arg == "-h" || arg == "--help") { print_help(); std::exit(0); }
        else if (arg == "-v" || arg == "--verbose") a.verbose = true;
        else if (arg == "--quiet") a.quiet = true;
        else if (arg == "-o") a.output = value("-o <OUTPUT>");
        else if (arg == "--knn") a.knn = parse_usize("--knn <KNN>", value("--knn <KNN>"));
        else if (arg == "--knn-ties") {
            const std::string v = value("--knn-ties <RULE>");
            if (v == "canonical") a.knn_ties = SKL_KNN_TIES_CANONICAL;
            else if (v == "reference") a.knn_ties = SKL_KNN_TIES_REFERENCE;
            else usage_error("invalid value '" + v + "' for '--knn-ties <RULE>': possible values: canonical, reference");
        }
        else if (arg == "--subset") a.subset = value("--subset <SUBSET>");
        else if (arg == "--pairs") a.pairs = value("--pairs <FILE>");
        else if (arg == "-k") a.kmer = parse_usize("-k <KMER>", value("-k <KMER>"));
        else if (arg == "--ani") a.ani = true;
        else if (arg == "--threads") {
            const std::string v = value("--threads <THREADS>");
            char *end = nullptr;
            const long long t = std::strtoll(v.c_str(), &end, 10);
            if (v.empty() || end != v.c_str() + v.size()) {
                usage_error("invalid value '" + v + "' for '--threads <THREADS>': `" + v + "` isn't a valid number of cores");
            }
            if (t < 1) usage_error("invalid value '" + v + "' for '--threads <THREADS>': Threads must be one or higher");
            a.threads = (size_t)t;
        }
        else if (arg == "--ref-completeness-file") a.ref_completeness_file = value(arg);
        else if (arg == "--query-completeness-file") a.query_completeness_file = value(arg);
        else if (arg == "--completeness-cutoff") {
            const std::string v = value(arg);
            char *end = nullptr;
            a.completeness_cutoff = std::strtod(v.c_str(), &end);
            if (v.empty() || end != v.c_str() + v.size()) usage_error("invalid value '" + v + "' for '--completeness-cutoff <COMPLETENESS_CUTOFF>': invalid float literal");
        }
        else if (arg == "--device") a.devices = {(int)parse_usize("--device <D>", value(arg))};
        else if (arg == "--npy") a.npy = true;
        else if (arg == "--band-mb") a.band_bytes = std::max<size_t>(1, parse_usize("--band-mb <MB>", value(arg))) << 20;
        else if (arg == "--gpus") {
            const size_t ngpu = parse_usize("--gpus <N>", value(arg));
            a.multi_device_flag = "--gpus <N>";
            if (ngpu < 1) usage_error("invalid value for '--gpus <N>': must be one or higher");
            a.devices.clear();
            for (size_t d = 0; d < ngpu; ++d) a.devices.push_back((int)d);
        }
        else if (arg == "--devices") {
            a.devices.clear();
            a.multi_device_flag = "--devices <LIST>";
            const std::string v = value(arg);
            size_t pos = 0;
            while (pos <= v.size()) {
                const size_t comma = v.find(',', pos);
                a.devices.push_back((int)parse_usize("--devices <LIST>", v.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos)));
                if (comma == std::string::npos) break;
                pos = comma + 1;
            }
        }
        else if (arg.size() > 2 && arg[0] == '-' && arg[1] != '-' && (arg[1] == 'o' || arg[1] == 'k')) {
            // clap accepts -k21 / -oFILE
            if (arg[1] == 'o') a.output = arg.substr(2);
            else a.kmer = parse_usize("-k <KMER>", arg.substr(2));
        }
        else if (arg.size() > 1 && arg[0] == '-') usage_error("unexpected argument '" + arg + "' found");
        else positional.push_back(arg);
    }
    if (positional.empty()) usage_error("the following required arguments were not provided:\n  <REF_DB>");
    if (positional.size() > 2) usage_error("unexpected argument '" + positional[2] + "' found");
    a.ref_db = positional[0];
    if (positional.size() == 2) a.query_db = positional[1];
    if (a.ani && !a.kmer) {  // #[arg(long, requires("kmer"))]
        usage_error("the following required arguments were not provided:\n  -k <KMER>");
    }
    if (a.pairs) {   // a list of pairs is neither a neighbour search nor a subset, and runs on one device as text
        const char *other = a.knn ? "--knn <KNN>" : a.subset ? "--subset <SUBSET>" : a.npy ? "--npy" : nullptr;
        if (other) usage_error(std::string("the argument '--pairs <FILE>' cannot be used with '") + other + "'");
        if (a.multi_device_flag) usage_error("the argument '--pairs <FILE>' cannot be used with '" + *a.multi_device_flag + "'");
    }
    return a;
}

// skl_ctx_flags() & SKL_CTX_FLAG_LOG_UNMATCHED, printed once when a completeness correction is asked for
const char *const LOG_UNMATCHED_WARNING =
    "this host's libm log() is neither form of glibc's x86-64 log the GPU reproduces bit for bit: with a completeness "
    "correction, core distances of flat fits (the same bin-match count at every k-mer length) may be 0 where a CPU run "
    "of sketchlib on this host prints 1, or the reverse; all other values agree to 1e-6";

struct Logger {
    bool info_on, warn_on;
    void info(const std::string &m) const { if (info_on) std::cerr << "INFO  [sketchlib] " << m << "\n"; }
    void warn(const std::string &m) const { if (warn_on) std::cerr << "WARN  [sketchlib] " << m << "\n"; }
};

// A dense matrix held whole in memory (multi-device path): text or .npy.
void write_whole(const DistanceMatrix &d, TextSink &sink, size_t n, const DistArgs &a)
{
    if (!a.npy) {
        d.write_rows(sink, 0, n, d.distances.data(), a.threads);
        return;
    }
    const std::string h = distances::npy_header(d.n_distances, d.jaccard.n_dist_cols());
    sink.finish(sink.begin(h.data(), h.size()), h.data(), h.size());
    const char *bytes = reinterpret_cast<const char *>(d.distances.data());
    const size_t len = d.distances.size() * sizeof(float);
    sink.finish(sink.begin(bytes, len), bytes, len);
}

// The listing is complete and flushed: leave without tearing down what the operating system reclaims anyway -- the slabs
// in HBM, gigabytes of host vectors, the worker pool, the HIP runtime (0.05 s of a 0.19 s run on 1 000 genomes, 0.5 s
// after a million).  Files are written with pwrite (nothing buffered in the process); SKL_CLI_FAST_EXIT=0 keeps the
// orderly exit.
// (called by main() AFTER its last line of output -- the verbose "Complete in" line -- with the command's exit code; a
// failed flush of the listing (ENOSPC, EPIPE) turns a success into exit code 1 and takes the orderly way out)
bool g_listing_complete = false;   // set by run_dist / run_inverted / run_inverted_query once the listing is written

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

int run_dist(const DistArgs &a)
{
    if (a.npy && (!a.output || a.knn)) {
        usage_error("--npy needs -o <file> and a dense (no --knn) output");
    }
    const bool timing = std::getenv("SKL_CLI_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto since_start = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    double t_loaded = 0, t_device = 0;
    // lib.rs:230-237: verbose -> Info, quiet -> Error, default -> Warn
    const Logger log{a.verbose && !a.quiet, !a.quiet};
    log.info("Using " + std::to_string(a.threads) + " threads");   // cli.rs:75-86 (host threads unused)
    if (a.threads > 2 * host_cpu_budget()) {
        log.info("This process may use " + std::to_string(host_cpu_budget()) + " CPUs (affinity / cgroup quota): the output is formatted by " +
                 std::to_string(2 * host_cpu_budget()) + " threads");
    }
    // The device contexts (HIP runtime start, stream, first allocations: 0.1-0.25 s) come up on their own thread while the
    // database is read; whatever goes wrong there is reported where the contexts are first needed, after the loading errors.
    std::future<std::unique_ptr<DeviceSet>> dev_starting =
        std::async(std::launch::async, [devices = a.devices] { return std::make_unique<DeviceSet>(devices); });

    // listings go through a TextSink (regular file: blocks written at offsets from all
    // formatting threads; stdout: in order)
    std::ostream *os = &std::cout;
    std::unique_ptr<TextSink> sink;
    if (a.output) {
        try {
            sink = std::make_unique<FileSink>(*a.output);
        } catch (const std::exception &e) {
            throw Panic(e.what());
        }
    }
    if (!sink) sink = std::make_unique<StreamSink>(*os);

    const std::string ref_db_name = strip_sketch_extension(a.ref_db);
    MultiSketch references;
    try {
        references = MultiSketch::load_metadata(ref_db_name);
    } catch (const std::exception &) {
        throw Panic("Could not read sketch metadata from " + a.ref_db + ".skm");  // lib.rs:322-323
    }
    // A distance at one k-mer length only ever reads that slice of each sample (jaccard.rs:6-45 through get_sketch_slice):
    // of a database with several lengths, only that slice is read, held and uploaded.  Not when the query database lists
    // other lengths than the reference database: that pair of databases is refused by the library (SKL_ERR_INCOMPATIBLE;
    // the reference would apply the reference database's k INDEX to the queries, mod.rs:253-269), as before.
    std::optional<MultiSketch> queries_peeked;
    if (a.kmer && references.kmer_lengths().size() > 1 && references.get_k_idx(*a.kmer)) {
        bool same_lengths = true;
        if (a.query_db) {
            try {
                queries_peeked = MultiSketch::load_metadata(strip_sketch_extension(*a.query_db));
                same_lengths = queries_peeked->kmer_lengths() == references.kmer_lengths();
            } catch (const std::exception &) {
                same_lengths = false;   // (reported where the reference reports it, after the reference database is read)
            }
        }
        if (same_lengths) {
            const size_t k_idx = *references.get_k_idx(*a.kmer);
            references.select_kmer(k_idx);
            if (queries_peeked) queries_peeked->select_kmer(k_idx);
        }
    }
    log.info("Loading sketch data from " + ref_db_name + ".skd");
    try {
        if (a.subset) {
            references.read_sketch_data_block(ref_db_name, read_subset_names(*a.subset));
        } else {
            references.read_sketch_data(ref_db_name);
        }
    } catch (const std::exception &e) {
        throw Panic(e.what());
    }
    const size_t n = references.number_samples_loaded();

    std::vector<std::string> warnings;
    std::optional<std::vector<double>> ref_comp;
    if (a.ref_completeness_file) {
        // an unreadable / malformed file is an Err returned from main in the reference (lib.rs:334-339,
        // `?`): "Error: ..." and exit code 1, which is what main() here does with std::exception
        ref_comp = read_completeness_file(*a.ref_completeness_file, references, &warnings);
    }

    DistType dist_type;
    try {
        dist_type = distances::set_k(references, a.kmer, a.ani);
    } catch (const std::exception &e) {
        throw Panic(std::string("Error setting k size: ") + e.what());  // lib.rs:341-343
    }
    log.info(dist_type.describe());

    std::optional<MultiSketch> queries;
    if (a.query_db) {
        const std::string query_db_name = strip_sketch_extension(*a.query_db);
        try {
            if (queries_peeked) queries = std::move(*queries_peeked);
            else queries = MultiSketch::load_metadata(query_db_name);
        } catch (const std::exception &) {
            throw Panic("Could not read sketch metadata from " + *a.query_db + ".skm");
        }
        log.info("Loading query sketch data from " + query_db_name + ".skd");
        try {
            queries->read_sketch_data(query_db_name);   // panics in the reference too (lib.rs:351)
        } catch (const std::exception &e) {
            throw Panic(e.what());
        }
    }
    std::optional<std::vector<double>> query_comp;
    if (queries && a.query_completeness_file) {
        query_comp = read_completeness_file(*a.query_completeness_file, *queries, &warnings);
    }
    for (const auto &w : warnings) log.warn(w);

    t_loaded = since_start();
    const std::unique_ptr<DeviceSet> dev_owner = dev_starting.get();
    DeviceSet &dev = *dev_owner;
    t_device = since_start();
    if (a.devices.size() > 1) log.info("Using " + std::to_string(a.devices.size()) + " GPU contexts (row-band partition)");
    for (size_t d = 0; d < dev.size(); ++d) {
        if (skl_ctx_set_knn_ties(dev[d].ctx(), a.knn_ties) != SKL_OK) throw std::runtime_error(skl_last_error());
    }
    if ((ref_comp || query_comp) && (skl_ctx_flags(dev[0].ctx()) & SKL_CTX_FLAG_LOG_UNMATCHED)) log.warn(LOG_UNMATCHED_WARNING);
    const std::vector<double> *rc = ref_comp ? &*ref_comp : nullptr;
    const std::vector<double> *qc = query_comp ? &*query_comp : nullptr;
    if (a.pairs) {
        // an unreadable file, a malformed line or an unknown sample: "Error: ..." and exit code 1, like a bad completeness file
        std::vector<std::string> ref_names, query_names;
        for (size_t i = 0; i < n; ++i) ref_names.push_back(references.sketch_name(i));
        if (queries) {
            for (size_t i = 0; i < queries->number_samples_loaded(); ++i) query_names.push_back(queries->sketch_name(i));
        }
        const std::vector<std::string> &second_names = queries ? query_names : ref_names;
        const PairsFile pairs = read_pairs_file(*a.pairs, ref_names, second_names, queries ? "query" : "reference");
        log.info("Calculating the distances of " + std::to_string(pairs.size()) + " listed pairs");
        if (dist_type.kind == DistType::CoreAcc && references.kmer_lengths().size() < 2) {
            throw Panic("Need at least two k-mer lengths to calculate core/accessory distances");
        }
        if (pairs.size() != 0) {
            distances::dists_pairs(dev[0], references, queries ? &*queries : nullptr, pairs, ref_names, second_names, dist_type, rc, qc,
                                   a.completeness_cutoff, *sink, a.threads);
        }
    } else if (!queries) {
        if (!a.knn) {
            log.info("Calculating all ref vs ref distances");
            if (n < 2) {
                if (dist_type.kind == DistType::CoreAcc && references.kmer_lengths().size() < 2) {
                    throw Panic("Need at least two k-mer lengths to calculate core/accessory distances");
                }
                return 0;  // empty upper triangle
            }
            if (a.devices.size() == 1) {
                // one device: stream row bands (compute band i+1 while band i is written)
                log.info("Writing out in long matrix form");
                distances::self_dists_all_streamed(dev[0], references, n, dist_type, rc, a.completeness_cutoff,
                                                   *sink, a.threads, a.band(), a.npy);
            } else {
                const DistanceMatrix d = distances::self_dists_all(dev, references, n, dist_type, a.quiet, rc,
                                                                   a.completeness_cutoff);
                log.info("Writing out in long matrix form");
                write_whole(d, *sink, n, a);
            }
        } else {
            size_t nn = *a.knn;
            if (nn >= n) {  // lib.rs:379-382
                log.warn("knn=" + std::to_string(nn) + " is higher than number of samples=" + std::to_string(n));
                nn = n - 1;
            }
            if (nn == 0) throw Panic("chunk size must be non-zero");  // par_chunks_mut(0)
            log.info("Calculating sparse ref vs ref distances with " + std::to_string(nn) + " nearest neighbours");
            const SparseDistanceMatrix d = distances::self_dists_knn(dev, references, n, nn, dist_type, a.quiet,
                                                                     rc, a.completeness_cutoff);
            log.info("Writing out in sparse matrix form");
            d.write(*sink, a.threads);
        }
    } else {
        const size_t n_query = queries->number_samples_loaded();
        if (a.knn) {
            size_t nn = *a.knn;
            if (nn > n) {  // lib.rs:411-414
                log.warn("knn=" + std::to_string(nn) + " is higher than number of reference samples=" + std::to_string(n));
                nn = n;
            }
            log.info("Calculating sparse ref vs query distances with " + std::to_string(nn) + " nearest neighbours");
            const SparseDistanceMatrix d = distances::cross_dists_knn(dev, references, *queries, n, n_query, nn,
                                                                      dist_type, a.quiet, rc, qc,
                                                                      a.completeness_cutoff);
            log.info("Writing out in sparse matrix form");
            d.write(*sink, a.threads);
        } else {
            log.info("Calculating all ref vs query distances");
            if (a.devices.size() == 1) {
                log.info("Writing out in long matrix form");
                distances::cross_dists_all_streamed(dev[0], references, *queries, n, n_query, dist_type, rc, qc,
                                                    a.completeness_cutoff, *sink, a.threads, a.band(), a.npy);
            } else {
                const DistanceMatrix d = distances::cross_dists_all(dev, references, *queries, n, n_query, dist_type,
                                                                    a.quiet, rc, qc, a.completeness_cutoff);
                log.info("Writing out in long matrix form");
                write_whole(d, *sink, n, a);
            }
        }
    }
    os->flush();
    if (timing) {
        const OutputTiming &t = output_timing();
        std::fprintf(stderr, "TIMING load=%.3fs device_wait=%.3fs dist+output=%.3fs (gpu_wait=%.3fs format=%.3fs sink=%.3fs)\n",
                     t_loaded, t_device - t_loaded, since_start() - t_device, t.wait_s, t.format_s, t.sink_s);
    }
    g_listing_complete = true;
    return 0;
}

// ---- `sketchlib sketch` (src/cli.rs:121-183, src/lib.rs:242-301), DNA assemblies and read sets ----
struct SketchArgs {
    std::vector<std::string> seq_files;
    std::optional<std::string> file_list, output;
    std::vector<size_t> k_vals, k_seq;
    uint64_t sketch_size = 1000;   // DEFAULT_SKETCHSIZE, cli.rs:17
    bool single_strand = false;
    size_t threads = 1;
    bool verbose = false, quiet = false;
    int gpu = -1;   // --gpu [D]: hash and take bin minima on device D (default: CPU)
    uint16_t min_count = 5;   // DEFAULT_MINCOUNT, cli.rs:12-15 (read sets only)
    uint8_t min_qual = 20;    // DEFAULT_MINQUAL (read sets only; compared with the raw quality byte)
};

// a u16 / u8 option as clap parses it: out of range is a usage error
size_t parse_bounded(const std::string &flag, const std::string &v, size_t max)
{
    const size_t x = parse_usize(flag, v);
    if (x > max || v.size() > 20) usage_error("invalid value '" + v + "' for '" + flag + "': " + v + " is not in 0..=" + std::to_string(max));
    return x;
}

void print_sketch_help()
{
    std::cout <<
        "Create sketches from input data\n\n"
        "Usage: sketchlib sketch [OPTIONS] -o <OUTPUT> <--k-vals <K_VALS>|--k-seq <K_SEQ>> <SEQ_FILES|-f <FILE_LIST>>\n\n"
        "A sample whose first file starts with a FASTQ record is a read set (one or two files, e.g. a pair); its\n"
        "k-mers pass a count filter (--min-count) and its bases a quality filter (--min-qual).  FASTA samples\n"
        "ignore both.  With --seq-type aa the files are protein FASTA: the 20 amino-acid letters are hashed (aaHash,\n"
        "forward only), anything else breaks the windows it lies in.\n\n"
        "Options:\n"
        "  -f <FILE_LIST>                  File listing sample names and their files (name<TAB>file[<TAB>file])\n"
        "  -o <OUTPUT>                     Output prefix (.skm / .skd)\n"
        "  -k, --k-vals <K_VALS>           K-mer lengths (comma separated)\n"
        "      --k-seq <K_SEQ>             K-mer lengths as start,end,step\n"
        "  -s, --sketch-size <SIZE>        Bins per k-mer length [default: 1000]\n"
        "      --seq-type <SEQ_TYPE>       Type of sequence to hash [default: dna] [possible values: dna, aa]\n"
        "      --level <LEVEL>             aa: aaHash level; level2 groups ST, DE, KQR, ILMV, FWY, level3 also A with ST and\n"
        "                                  N with DE [default: level1] [possible values: level1, level2, level3]\n"
        "      --concat-fasta              aa: every FASTA record is a sample of its own, named <name>_<n>\n"
        "      --single-strand             Ignore the reverse complement (aa: only the flag in the metadata changes)\n"
        "      --min-count <MIN_COUNT>     Read sets: minimum k-mer count [default: 5]\n"
        "      --min-qual <MIN_QUAL>       Read sets: minimum quality byte of a base, compared raw (no Phred offset)\n"
        "                                  [default: 20]\n"
        "      --threads <THREADS>         Number of CPU threads [default: 1]\n"
        "      --gpu                       Hash on the GPU (device 0); read sets replay the count filter on the host\n"
        "      --device <D>                The same on device D\n"
        "  -v, --verbose                   Show progress messages\n"
        "      --quiet                     Don't show any messages\n"
        "  -h, --help                      Print help\n";
}

std::vector<size_t> parse_list(const std::string &flag, const std::string &v)
{
    std::vector<size_t> out;
    size_t pos = 0;
    while (pos <= v.size()) {
        const size_t comma = v.find(',', pos);
        const std::string tok = v.substr(pos, comma == std::string::npos ? std::string::npos : comma - pos);
        out.push_back(parse_usize(flag, tok));
        if (comma == std::string::npos) break;
        pos = comma + 1;
    }
    return out;
}

int run_sketch(int argc, char **argv, int first, bool verbose, bool quiet)
{
    g_usage = "sketchlib sketch [OPTIONS] -o <OUTPUT> <--k-vals <K_VALS>|--k-seq <K_SEQ>> <SEQ_FILES|-f <FILE_LIST>>";
    SketchArgs a;
    SeqType seq;
    a.verbose = verbose;
    a.quiet = quiet;
    for (int i = first; i < argc; ++i) {
        std::string arg = argv[i];
        auto value = [&](const std::string &flag) -> std::string {
            if (i + 1 >= argc) usage_error("a value is required for '" + flag + "' but none was supplied");
            return argv[++i];
        };
        if (arg == "-h" || arg == "--help") { print_sketch_help(); std::exit(0); }
        else if (arg == "-v" || arg == "--verbose") a.verbose = true;
        else if (arg == "--quiet") a.quiet = true;
        else if (arg == "-f") a.file_list = value("-f <FILE_LIST>");
        else if (arg == "-o") a.output = value("-o <OUTPUT>");
        else if (arg == "-k" || arg == "--k-vals") a.k_vals = parse_list("--k-vals <K_VALS>", value(arg));
        else if (arg == "--k-seq") a.k_seq = parse_list("--k-seq <K_SEQ>", value(arg));
        else if (arg == "-s" || arg == "--sketch-size") a.sketch_size = parse_usize("--sketch-size <SKETCH_SIZE>", value(arg));
        else if (arg == "--single-strand") a.single_strand = true;
        else if (arg == "--threads") a.threads = std::max<size_t>(1, parse_usize("--threads <THREADS>", value(arg)));
        else if (arg == "--gpu") a.gpu = 0;
        else if (arg == "--device") a.gpu = (int)parse_usize("--device <D>", value(arg));
        else if (arg == "--seq-type") {
            const std::string v = value(arg);
            if (v == "pdb") { std::cerr << "error: structures are not part of this build (--seq-type pdb); it sketches dna and aa\n"; return 2; }
            if (v != "dna" && v != "aa") usage_error("invalid value '" + v + "' for '--seq-type <SEQ_TYPE>'\n  [possible values: dna, aa, pdb]");
            seq.aa = v == "aa";
        }
        else if (arg == "--min-count") a.min_count = (uint16_t)parse_bounded("--min-count <MIN_COUNT>", value(arg), 0xFFFF);
        else if (arg == "--min-qual") a.min_qual = (uint8_t)parse_bounded("--min-qual <MIN_QUAL>", value(arg), 0xFF);
        else if (arg == "--level") {
            const std::string v = value(arg);
            if (v != "level1" && v != "level2" && v != "level3") usage_error("invalid value '" + v + "' for '--level <LEVEL>'\n  [possible values: level1, level2, level3]");
            seq.level = v.back() - '0';
        }
        else if (arg == "--concat-fasta") seq.concat_fasta = true;
        else if (arg.size() > 1 && arg[0] == '-') usage_error("unexpected argument '" + arg + "' found");
        else a.seq_files.push_back(arg);
    }
    if (!a.output) usage_error("the following required arguments were not provided:\n  -o <OUTPUT>");
    if (a.seq_files.empty() == !a.file_list.has_value()) {
        usage_error("exactly one of <SEQ_FILES>... or -f <FILE_LIST> must be given");
    }
    if (a.k_vals.empty() == a.k_seq.empty()) usage_error("exactly one of --k-vals or --k-seq must be given");
    if (seq.concat_fasta && !seq.aa) throw Panic("--concat-fasta currently only supported with --seq-type aa");   // lib.rs:258-260
    if (!seq.aa) seq.level = 1;   // (--level is read with aa only)
    const Logger log{a.verbose && !a.quiet, !a.quiet};
    const std::vector<InputFastx> inputs = a.file_list ? read_rfile(*a.file_list) : read_input_fastas(a.seq_files);
    log.info("Parsed " + std::to_string(inputs.size()) + " samples in input list");
    const std::vector<size_t> kmers = parse_kmers(a.k_vals, a.k_seq);
    const uint64_t bins = (a.sketch_size + 63) / 64 * 64;
    log.info("Running sketching: sketch_size:" + std::to_string(bins) + " threads:" + std::to_string(a.threads));
    try {
        if (a.gpu >= 0) {
            log.info("Hashing on GPU " + std::to_string(a.gpu));
            Device dev(a.gpu);
            sketch_files_gpu(dev, *a.output, inputs, kmers, a.sketch_size, !a.single_strand, a.threads, a.min_count, a.min_qual, seq);
        } else {
            sketch_files(*a.output, inputs, kmers, a.sketch_size, !a.single_strand, a.threads, a.min_count, a.min_qual, seq);
        }
    } catch (const std::exception &e) {
        throw Panic(e.what());   // the reference panics on unreadable / empty input
    }
    return 0;
}

// ---- `sketchlib merge | append | delete | info` (src/cli.rs:240-322, src/lib.rs:454-483 and 793-947) ----
// merge, delete and info are file operations (dbmaint.cpp): no device context is made.
int run_merge(int argc, char **argv, int first)
{
    g_usage = "sketchlib merge -o <OUTPUT> <DB1> <DB2>";
    std::vector<std::string> dbs;
    std::optional<std::string> output;
    for (int i = first; i < argc; ++i) {
        const std::string arg = argv[i];
        if (arg == "-h" || arg == "--help") {
            std::cout << "Merge two sketch files (.skm and .skd pair)\n\nUsage: " << g_usage << "\n\n"
                         "Arguments:\n  <DB1>  The first .skd (sketch data) file\n  <DB2>  The second .skd (sketch data) file\n\n"
                         "Options:\n  -o <OUTPUT>  Output filename for the merged sketch\n  -h, --help   Print help\n";
            std::exit(0);
        }
        else if (arg == "-v" || arg == "--verbose" || arg == "--quiet") continue;
        else if (arg == "-o") {
            if (i + 1 >= argc) usage_error("a value is required for '-o <OUTPUT>' but none was supplied");
            output = argv[++i];
        }
        else if (arg.size() > 2 && arg[0] == '-' && arg[1] == 'o') output = arg.substr(2);
        else if (arg.size() > 1 && arg[0] == '-') usage_error("unexpected argument '" + arg + "' found");
        else dbs.push_back(arg);
    }
    if (dbs.size() < 2) usage_error(std::string("the following required arguments were not provided:\n  ") + (dbs.empty() ? "<DB1>\n  <DB2>" : "<DB2>"));
    if (dbs.size() > 2) usage_error("unexpected argument '" + dbs[2] + "' found");
    if (!output) usage_error("the following required arguments were not provided:\n  -o <OUTPUT>");
    db_merge(dbs[0], dbs[1], *output);
    return 0;
}

int run_delete(int argc, char **argv, int first)
{
    g_usage = "sketchlib delete <DB> <SAMPLES> <OUTPUT_FILE>";
    std::vector<std::string> pos;
    for (int i = first; i < argc; ++i) {
        const std::string arg = argv[i];
        if (arg == "-h" || arg == "--help") {
            std::cout << "Delete genome(s) from a database (input: one id per line)\n\nUsage: " << g_usage << "\n\n"
                         "Arguments:\n  <DB>           Sketching database\n  <SAMPLES>      Input file with IDs to delete (one ID per line)\n"
                         "  <OUTPUT_FILE>  Output prefix of the database without them\n\nOptions:\n  -h, --help  Print help\n";
            std::exit(0);
        }
        else if (arg == "-v" || arg == "--verbose" || arg == "--quiet") continue;
        else if (arg.size() > 1 && arg[0] == '-') usage_error("unexpected argument '" + arg + "' found");
        else pos.push_back(arg);
    }
    static const char *const names[] = {"<DB>", "<SAMPLES>", "<OUTPUT_FILE>"};
    if (pos.size() < 3) {
        std::string msg = "the following required arguments were not provided:";
        for (size_t i = pos.size(); i < 3; ++i) msg += std::string("\n  ") + names[i];
        usage_error(msg);
    }
    if (pos.size() > 3) usage_error("unexpected argument '" + pos[3] + "' found");
    db_delete(pos[0], pos[1], pos[2]);
    return 0;
}

int run_info(int argc, char **argv, int first)
{
    g_usage = "sketchlib info [OPTIONS] <SKM_FILE>";
    std::optional<std::string> file;
    bool sample_info = false;
    for (int i = first; i < argc; ++i) {
        const std::string arg = argv[i];
        if (arg == "-h" || arg == "--help") {
            std::cout << "Print information about a .skm or .ski file\n\nUsage: " << g_usage << "\n\n"
                         "Arguments:\n  <SKM_FILE>  Sketch metadata file (.skm) or inverted index (.ski) to describe\n\n"
                         "Options:\n      --sample-info  Write out the information for every sample contained\n  -h, --help         Print help\n";
            std::exit(0);
        }
        else if (arg == "-v" || arg == "--verbose" || arg == "--quiet") continue;
        else if (arg == "--sample-info") sample_info = true;
        else if (arg.size() > 1 && arg[0] == '-') usage_error("unexpected argument '" + arg + "' found");
        else if (!file) file = arg;
        else usage_error("unexpected argument '" + arg + "' found");
    }
    if (!file) usage_error("the following required arguments were not provided:\n  <SKM_FILE>");
    db_info(*file, sample_info, std::cout);
    std::cout.flush();
    return 0;
}

// `append`: the new samples are sketched the way the database was (its k-mer lengths, sketch size and sequence type; the
// `sketch` code path, on the host or with --gpu on the device) into <out>, the database's blocks follow them, and the
// metadata is the new samples' with the database's merged in behind (lib.rs:857-875).
int run_append(int argc, char **argv, int first, bool verbose, bool quiet)
{
    g_usage = "sketchlib append [OPTIONS] -o <OUTPUT> <DB> <SEQ_FILES|-f <FILE_LIST>>";
    std::optional<std::string> db, file_list, output;
    std::vector<std::string> seq_files;
    bool single_strand = false, concat_fasta = false;
    uint16_t min_count = 5;   // DEFAULT_MINCOUNT / DEFAULT_MINQUAL, cli.rs:12-15 (read sets only)
    uint8_t min_qual = 20;
    size_t threads = 1;
    int gpu = -1;
    std::optional<int> level;
    for (int i = first; i < argc; ++i) {
        const std::string arg = argv[i];
        auto value = [&](const std::string &flag) -> std::string {
            if (i + 1 >= argc) usage_error("a value is required for '" + flag + "' but none was supplied");
            return argv[++i];
        };
        if (arg == "-h" || arg == "--help") {
            std::cout <<
                "Append new genomes to be sketched to an existing sketch database\n\nUsage: " << g_usage << "\n\n"
                "The new samples come FIRST in the output, the samples of <DB> after them.\n\n"
                "Options:\n"
                "  -f <FILE_LIST>               File listing sample names and their files (name<TAB>file[<TAB>file])\n"
                "  -o <OUTPUT>                  Output prefix (.skm / .skd); must differ from <DB>\n"
                "      --single-strand          Ignore the reverse complement\n"
                "      --min-count <MIN_COUNT>  Read sets: minimum k-mer count [default: 5]\n"
                "      --min-qual <MIN_QUAL>    Read sets: minimum quality byte of a base [default: 20]\n"
                "      --concat-fasta           aa: every FASTA record is a sample of its own\n"
                "      --level <LEVEL>          aa: must be the database's aaHash level [default: the database's]\n"
                "      --threads <THREADS>      Number of CPU threads [default: 1]\n"
                "      --gpu                    Hash on the GPU (device 0)\n"
                "      --device <D>             The same on device D\n"
                "  -h, --help                   Print help\n";
            std::exit(0);
        }
        else if (arg == "-v" || arg == "--verbose") verbose = true;
        else if (arg == "--quiet") quiet = true;
        else if (arg == "-f") file_list = value("-f <FILE_LIST>");
        else if (arg == "-o") output = value("-o <OUTPUT>");
        else if (arg == "--single-strand") single_strand = true;
        else if (arg == "--concat-fasta") concat_fasta = true;
        else if (arg == "--min-count") min_count = (uint16_t)parse_bounded("--min-count <MIN_COUNT>", value(arg), 0xFFFF);
        else if (arg == "--min-qual") min_qual = (uint8_t)parse_bounded("--min-qual <MIN_QUAL>", value(arg), 0xFF);
        else if (arg == "--threads") threads = std::max<size_t>(1, parse_usize("--threads <THREADS>", value(arg)));
        else if (arg == "--gpu") gpu = 0;
        else if (arg == "--device") gpu = (int)parse_usize("--device <D>", value(arg));
        else if (arg == "--level") {
            const std::string v = value(arg);
            if (v != "level1" && v != "level2" && v != "level3") usage_error("invalid value '" + v + "' for '--level <LEVEL>'\n  [possible values: level1, level2, level3]");
            level = v.back() - '0';
        }
        else if (arg.size() > 1 && arg[0] == '-') usage_error("unexpected argument '" + arg + "' found");
        else if (!db) db = arg;
        else seq_files.push_back(arg);
    }
    if (!db) usage_error("the following required arguments were not provided:\n  <DB>");
    if (!output) usage_error("the following required arguments were not provided:\n  -o <OUTPUT>");
    if (seq_files.empty() == !file_list.has_value()) {
        usage_error("exactly one of <SEQ_FILES>... or -f <FILE_LIST> must be given");
    }
    const Logger log{verbose && !quiet, !quiet};
    const std::string db_name = strip_sketch_extension(*db);
    if (strip_sketch_extension(*output) == db_name) {
        throw std::runtime_error("the output " + *output + " is the database itself: append writes a new database");
    }
    log.info("Getting input files");
    const std::vector<InputFastx> inputs = file_list ? read_rfile(*file_list) : read_input_fastas(seq_files);
    log.info("Parsed " + std::to_string(inputs.size()) + " samples in input list");
    MultiSketch db_metadata = MultiSketch::load_metadata(db_name);   // `?` in the reference: Error, exit 1
    {   // append_compatibility, multisketch.rs:229-244: before anything is sketched
        std::vector<std::string> duplicates;
        for (const auto &in : inputs) {
            if (db_metadata.has_sample(in.first)) duplicates.push_back(in.first);
        }
        if (!duplicates.empty()) {
            std::cout << "Duplicates found: " << rust_debug(duplicates) << std::endl;
            throw Panic("Databases are not compatible for merging.");
        }
    }
    log.info("Passed concat check");
    SeqType seq;
    const std::string &hash_type = db_metadata.hash_type();
    if (hash_type.rfind("AA:Level", 0) == 0 && hash_type.size() == 9 && hash_type[8] >= '1' && hash_type[8] <= '3') {
        seq.aa = true;
        seq.level = hash_type[8] - '0';
        if (level && *level != seq.level) {
            throw std::runtime_error("--level level" + std::to_string(*level) + " is not the level of the database (" +
                                     hash_type_debug(hash_type) + "): its samples and the new ones would not be comparable");
        }
    } else if (hash_type != "DNA") {
        std::cerr << "error: this build sketches dna and aa (" << db_name << ".skm has sequence type " << hash_type_debug(hash_type) << ")\n";
        return 2;
    }
    if (concat_fasta && !seq.aa) throw Panic("--concat-fasta currently only supported with --seq-type aa");   // lib.rs:825-827
    seq.concat_fasta = concat_fasta;
    const std::vector<size_t> &kmers = db_metadata.kmer_lengths();
    log.info("Running sketching: sketch_size:" + std::to_string(db_metadata.sketch_size) + " threads:" + std::to_string(threads));
    MultiSketch fresh;
    try {
        if (gpu >= 0) {
            log.info("Hashing on GPU " + std::to_string(gpu));
            Device dev(gpu);   // (no device: an error, never the host loop)
            fresh = sketch_files_gpu(dev, *output, inputs, kmers, db_metadata.sketch_size, !single_strand, threads, min_count, min_qual, seq);
        } else {
            fresh = sketch_files(*output, inputs, kmers, db_metadata.sketch_size, !single_strand, threads, min_count, min_qual, seq);
        }
    } catch (const std::exception &e) {
        throw Panic(e.what());   // the reference panics on unreadable / empty input
    }
    log.info("Merging and saving sketch data to " + *output + ".skd");
    append_file(db_name + ".skd", *output + ".skd", false);
    try {
        fresh.merge_sketches(db_metadata);
    } catch (const std::exception &e) {
        throw Panic(e.what());
    }
    try {
        fresh.save_metadata(*output);
    } catch (const std::exception &) {
        throw Panic("Could not save metadata to " + *output);
    }
    return 0;
}

// ---- `sketchlib inverted query` (src/cli.rs:380-412, src/lib.rs:605-680) ----
// Queries (assemblies or read sets, --min-count / --min-qual as in `sketch`) are sketched the way the index was built
// (Inverted::sketch_queries, inverted.rs:118-140) -- on host threads, or with --gpu on the device --device names
// (sketch_inverted_gpu) -- then matched against every indexed sample on the GPU (skl_inverted_query, csrc/inv_query.hip), one band of
// queries at a time: band i + 1 computes while band i is formatted on --threads threads and written.  Rows come in
// input order (the reference's come in whatever order its threads finish).
// --top N (match-count only): the N best hits of every query instead of every count -- the reference's identification
// query (SketchlibData::query / get_probs, src/lib.rs:1019-1109), selected on the device (skl_inverted_query_top,
// csrc/inv_top.hip) -- in long form, one line per hit with d / (2 S - d) and the index's label and metadata.
int run_inverted_query(int argc, char **argv, int first, bool verbose, bool quiet)
{
    g_usage = "sketchlib inverted query [OPTIONS] <SKI> <SEQ_FILES|-f <FILE_LIST>>";
    std::optional<std::string> ski, file_list, output;
    std::vector<std::string> seq_files;
    int mode = SKL_INVQ_MATCH_COUNT;
    std::string mode_name = "match-count";
    size_t threads = 1;
    int device = 0;
    bool gpu_sketch = false;
    uint16_t min_count = 5;   // DEFAULT_MINCOUNT / DEFAULT_MINQUAL, cli.rs:12-15 (read sets only)
    uint8_t min_qual = 20;
    size_t top = 0;           // --top N: 0 = every count (the default)
    bool query_type_given = false;
    for (int i = first; i < argc; ++i) {
        const std::string arg = argv[i];
        auto value = [&](const std::string &flag) -> std::string {
            if (i + 1 >= argc) usage_error("a value is required for '" + flag + "' but none was supplied");
            return argv[++i];
        };
        if (arg == "-v" || arg == "--verbose") verbose = true;
        else if (arg == "--quiet") quiet = true;
        else if (arg == "-f") file_list = value("-f <FILE_LIST>");
        else if (arg == "-o") output = value("-o <OUTPUT>");
        else if (arg == "--top") {
            const std::string v = value("--top <N>");
            top = parse_usize("--top <N>", v);
            if (top == 0 || top > SKL_INVQ_TOP_MAX || v.size() > 20) {   // the hits of a query are held in the kernel's LDS list
                usage_error("invalid value '" + v + "' for '--top <N>': " + v + " is not in 1..=" + std::to_string(SKL_INVQ_TOP_MAX));
            }
        }
        else if (arg == "--query-type") {
            query_type_given = true;
            mode_name = value("--query-type <QUERY_TYPE>");
            if (mode_name == "match-count") mode = SKL_INVQ_MATCH_COUNT;
            else if (mode_name == "all-bins") mode = SKL_INVQ_ALL_BINS;
            else if (mode_name == "any-bins") mode = SKL_INVQ_ANY_BINS;
            else usage_error("invalid value '" + mode_name + "' for '--query-type <QUERY_TYPE>'\n  [possible values: match-count, all-bins, any-bins]");
        }
        else if (arg == "--threads") threads = std::max<size_t>(1, parse_usize("--threads <THREADS>", value(arg)));
        else if (arg == "--min-count") min_count = (uint16_t)parse_bounded("--min-count <MIN_COUNT>", value(arg), 0xFFFF);
        else if (arg == "--min-qual") min_qual = (uint8_t)parse_bounded("--min-qual <MIN_QUAL>", value(arg), 0xFF);
        else if (arg == "--gpu") gpu_sketch = true;   // sketch the queries on the device too (the one --device names)
        else if (arg == "--device") device = (int)parse_usize("--device <D>", value(arg));
        else if (arg.size() > 1 && arg[0] == '-') usage_error("unexpected argument '" + arg + "' found");
        else if (!ski) ski = arg;
        else seq_files.push_back(arg);
    }
    if (top && query_type_given && mode != SKL_INVQ_MATCH_COUNT) {
        usage_error("the argument '--top <N>' cannot be used with '--query-type <QUERY_TYPE>'");
    }
    if (!ski) usage_error("the following required arguments were not provided:\n  <SKI>");
    if (seq_files.empty() == !file_list.has_value()) {
        usage_error("exactly one of <SEQ_FILES>... or -f <FILE_LIST> must be given");
    }
    const Logger log{verbose && !quiet, !quiet};
    const bool timing = std::getenv("SKL_CLI_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto since_start = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    // (as in `precluster`: the device comes up while the .ski is read; a device that failed to come up is only reported
    // where it is first needed, after every error of the .ski and of the inputs)
    std::future<std::unique_ptr<Device>> dev_starting =
        std::async(std::launch::async, [device] { return std::make_unique<Device>(device); });
    const std::string prefix = strip_sketch_extension(*ski);
    const Inverted inv = Inverted::load(prefix);   // `?` in the reference: Error, exit 1
    log.info("Read inverted index: " + std::to_string(inv.sample_names.size()) + " samples, k=" +
             std::to_string(inv.kmer_size) + ", sketch size " + std::to_string(inv.sketch_size()));
    if (inv.hash_type != "DNA") {
        std::cerr << "error: this build queries DNA indices only (" << prefix << ".ski has hash_type " << inv.hash_type << ")\n";
        return 2;
    }
    const size_t n = inv.sample_names.size(), S = inv.sketch_size();
    const std::vector<uint16_t> index_bins = inv.dense_bins(prefix + ".ski");
    const double t_load = since_start();

    log.info("Getting input queries");
    const std::vector<InputFastx> inputs = file_list ? read_rfile(*file_list) : read_input_fastas(seq_files);
    log.info("Parsed " + std::to_string(inputs.size()) + " samples in input query list");
    log.info("Sketching input queries");
    const size_t nq = inputs.size();
    std::vector<uint16_t> query_bins(nq * S);
    std::unique_ptr<Device> dev_owner;
    try {
        if (gpu_sketch) {
            dev_owner = dev_starting.get();   // ("no CPU path" without a device: no fallback to the host loop)
            const std::vector<std::vector<uint16_t>> rows =
                sketch_inverted_gpu(*dev_owner, inputs, inv.kmer_size, S, inv.rc, threads, min_count, min_qual);
            for (size_t i = 0; i < nq; ++i) std::copy(rows[i].begin(), rows[i].end(), query_bins.begin() + i * S);
        }
        std::atomic<size_t> next{gpu_sketch ? nq : 0};   // (nothing left for the host loop then)
        std::exception_ptr err;
        std::mutex mu;
        auto work = [&] {
            try {
                for (;;) {
                    const size_t i = next.fetch_add(1);
                    if (i >= nq) break;
                    const std::vector<uint16_t> q = sketch_sample_inverted(inputs[i], inv.kmer_size, S, inv.rc, min_count, min_qual);
                    std::copy(q.begin(), q.end(), query_bins.begin() + i * S);
                }
            } catch (...) {
                std::lock_guard<std::mutex> lk(mu);
                err = std::current_exception();
            }
        };
        std::vector<std::thread> pool;
        for (size_t t = 1; t < std::min(threads, nq); ++t) pool.emplace_back(work);
        work();
        for (auto &t : pool) t.join();
        if (err) std::rethrow_exception(err);
    } catch (const std::exception &e) {
        throw Panic(e.what());   // the reference panics on unreadable / empty input
    }
    const double t_sketch = since_start();

    std::unique_ptr<TextSink> sink;
    if (output) {
        try {
            sink = std::make_unique<FileSink>(*output);
        } catch (const std::exception &e) {
            throw Panic(e.what());
        }
    } else {
        sink = std::make_unique<StreamSink>(std::cout);
    }
    auto write = [&](const std::string &text) {
        if (!text.empty()) sink->finish(sink->begin(text.data(), text.size()), text.data(), text.size());
    };

    if (!dev_owner) dev_owner = dev_starting.get();
    Device &dev = *dev_owner;
    skl_inverted *ix = nullptr;
    if (skl_inverted_create(dev.ctx(), index_bins.data(), n, S, &ix) != SKL_OK) throw std::runtime_error(skl_last_error());
    std::unique_ptr<skl_inverted, int (*)(skl_inverted *)> ix_owner(ix, skl_inverted_destroy);
    const double t_device = since_start();

    log.info("Running queries in mode: " + mode_name);
    {
        std::string header = "Query";
        if (top) {
            header += "\tSample\tMatches\tJaccard\tLabel\tMetadata";
        } else if (mode == SKL_INVQ_MATCH_COUNT) {
            for (const auto &name : inv.sample_names) header += "\t" + name;
        } else {
            header += "\tMatches";
        }
        write(header + "\n");
    }
    // bands of queries: 256 MB of results on the host at a time (at least one query)
    const size_t words64 = (n + 63) / 64;
    // (--top: a band's ids [rows][top], then its counts [rows][top])
    const size_t row_bytes = std::max<size_t>(1, top ? top * 2 * sizeof(uint32_t) : mode == SKL_INVQ_MATCH_COUNT ? n * sizeof(uint32_t) : words64 * sizeof(uint64_t));
    const size_t band = std::max<size_t>(1, std::min<size_t>(nq, (256ull << 20) / row_bytes));
    auto compute = [&](size_t q0) {
        const size_t rows = std::min(band, nq - q0);
        std::vector<uint64_t> buf((rows * row_bytes + 7) / 8);
        uint32_t *hits = reinterpret_cast<uint32_t *>(buf.data());
        const int rc = top ? skl_inverted_query_top(dev.ctx(), ix, query_bins.data() + q0 * S, rows, top, hits, hits + rows * top)
                           : skl_inverted_query(dev.ctx(), ix, query_bins.data() + q0 * S, rows, mode, buf.data());
        if (rc != SKL_OK) throw std::runtime_error(skl_last_error());
        return buf;
    };
    double t_query = 0, t_write = 0;
    std::future<std::vector<uint64_t>> pending;
    if (nq) pending = std::async(std::launch::async, compute, (size_t)0);
    for (size_t q0 = 0; q0 < nq; q0 += band) {
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<uint64_t> buf = pending.get();
        if (q0 + band < nq) pending = std::async(std::launch::async, compute, q0 + band);
        const auto t1 = std::chrono::steady_clock::now();
        const size_t rows = std::min(band, nq - q0);
        // format the band's rows on `threads` threads, in contiguous pieces, then write the pieces in order
        const size_t n_pieces = std::min(rows, threads);
        std::vector<std::string> pieces(n_pieces);
        auto format = [&](size_t piece) {
            std::string &o = pieces[piece];
            char num[16];
            for (size_t r = rows * piece / n_pieces; r < rows * (piece + 1) / n_pieces; ++r) {
                if (top) {   // one line per hit, best first; fewer than `top` lines when the index is smaller
                    const uint32_t *ids = reinterpret_cast<const uint32_t *>(buf.data()) + r * top, *cnt = ids + rows * top;
                    char jac[40];
                    for (size_t h = 0; h < std::min(top, n); ++h) {
                        const uint32_t s = ids[h], c = cnt[h];
                        o += inputs[q0 + r].first;
                        o += '\t';
                        o += inv.sample_names[s];
                        num[0] = '\t';
                        o.append(num, std::to_chars(num + 1, num + sizeof num, c).ptr);
                        o += '\t';
                        // lib.rs:1049: d / (2 S - d) in f64, shortest digits that read back as the same value
                        const double j = (double)c / (2.0 * (double)S - (double)c);
                        o.append(jac, std::to_chars(jac, jac + sizeof jac, j, std::chars_format::fixed).ptr);
                        o += '\t';
                        if (inv.labels) o += (*inv.labels)[s];
                        o += '\t';
                        if (inv.metadata) o += (*inv.metadata)[s];
                        o += '\n';
                    }
                    continue;
                }
                o += inputs[q0 + r].first;
                if (mode == SKL_INVQ_MATCH_COUNT) {
                    const uint32_t *c = reinterpret_cast<const uint32_t *>(buf.data()) + r * n;
                    for (size_t s = 0; s < n; ++s) {
                        num[0] = '\t';
                        const auto res = std::to_chars(num + 1, num + sizeof num, c[s]);
                        o.append(num, res.ptr);
                    }
                } else {
                    const uint64_t *bits = buf.data() + r * words64;
                    char sep = '\t';
                    for (size_t w = 0; w < words64; ++w) {
                        for (uint64_t b = bits[w]; b; b &= b - 1) {   // ascending .ski index (RoaringBitmap order)
                            o += sep;
                            o += inv.sample_names[w * 64 + (size_t)__builtin_ctzll(b)];
                            sep = ',';
                        }
                    }
                }
                o += '\n';
            }
        };
        std::vector<std::thread> pool;
        for (size_t t = 1; t < n_pieces; ++t) pool.emplace_back(format, t);
        format(0);
        for (auto &t : pool) t.join();
        for (const auto &piece : pieces) write(piece);
        const auto t2 = std::chrono::steady_clock::now();
        t_query += std::chrono::duration<double>(t1 - t0).count();
        t_write += std::chrono::duration<double>(t2 - t1).count();
    }
    std::cout.flush();
    if (timing) {
        std::fprintf(stderr, "TIMING inverted query: load=%.3fs sketch=%.3fs device=%.3fs query=%.3fs write=%.3fs\n",
                     t_load, t_sketch - t_load, t_device - t_sketch, t_query, t_write);
    }
    g_listing_complete = true;
    return 0;
}

// ---- `sketchlib inverted build|query|precluster` (src/cli.rs:329-461, src/lib.rs:485-789) ----
int run_inverted(int argc, char **argv, int first, bool verbose, bool quiet)
{
    if (first >= argc) usage_error("'sketchlib inverted' requires a subcommand: build | query | precluster");
    const std::string sub = argv[first];
    if (sub == "query") return run_inverted_query(argc, argv, first + 1, verbose, quiet);
    auto next_value = [&](int &i, const std::string &flag) -> std::string {
        if (i + 1 >= argc) usage_error("a value is required for '" + flag + "' but none was supplied");
        return argv[++i];
    };
    if (sub == "build") {
        g_usage = "sketchlib inverted build [OPTIONS] -o <OUTPUT> <SEQ_FILES|-f <FILE_LIST>>";
        std::vector<std::string> seq_files;
        std::optional<std::string> file_list, output, species_names, metadata_file;
        bool write_skq_flag = false, single_strand = false;
        uint64_t sketch_size = 1000;   // DEFAULT_SKETCHSIZE, cli.rs:17
        size_t kmer = 21, threads = 1; // DEFAULT_KMER, cli.rs:13
        int gpu = -1;                  // --gpu / --device D: sketch on that device (sketch_inverted_gpu)
        uint16_t min_count = 5;        // DEFAULT_MINCOUNT / DEFAULT_MINQUAL, cli.rs:12-15 (read sets only)
        uint8_t min_qual = 20;
        for (int i = first + 1; i < argc; ++i) {
            const std::string arg = argv[i];
            if (arg == "-v" || arg == "--verbose") verbose = true;
            else if (arg == "--quiet") quiet = true;
            else if (arg == "-f") file_list = next_value(i, "-f <FILE_LIST>");
            else if (arg == "-o") output = next_value(i, "-o <OUTPUT>");
            else if (arg == "--write-skq") write_skq_flag = true;
            else if (arg == "--species-names") species_names = next_value(i, arg);
            else if (arg == "--metadata") metadata_file = next_value(i, arg);
            else if (arg == "-s" || arg == "--sketch-size") sketch_size = parse_usize("--sketch-size <SKETCH_SIZE>", next_value(i, arg));
            else if (arg == "-k" || arg == "--kmer-length") kmer = parse_usize("--kmer-length <KMER_LENGTH>", next_value(i, arg));
            else if (arg == "--single-strand") single_strand = true;
            else if (arg == "--threads") threads = std::max<size_t>(1, parse_usize("--threads <THREADS>", next_value(i, arg)));
            else if (arg == "--min-count") min_count = (uint16_t)parse_bounded("--min-count <MIN_COUNT>", next_value(i, arg), 0xFFFF);
            else if (arg == "--min-qual") min_qual = (uint8_t)parse_bounded("--min-qual <MIN_QUAL>", next_value(i, arg), 0xFF);
            else if (arg == "--gpu") gpu = 0;
            else if (arg == "--device") gpu = (int)parse_usize("--device <D>", next_value(i, arg));
            else if (arg.size() > 1 && arg[0] == '-') usage_error("unexpected argument '" + arg + "' found");
            else seq_files.push_back(arg);
        }
        if (!output) usage_error("the following required arguments were not provided:\n  -o <OUTPUT>");
        if (seq_files.empty() == !file_list.has_value()) {
            usage_error("exactly one of <SEQ_FILES>... or -f <FILE_LIST> must be given");
        }
        const Logger log{verbose && !quiet, !quiet};
        log.info("Getting input files");
        const std::vector<InputFastx> inputs = file_list ? read_rfile(*file_list) : read_input_fastas(seq_files);
        log.info("Parsed " + std::to_string(inputs.size()) + " samples in input list");
        {
            std::vector<std::string> names;
            for (const auto &in : inputs) names.push_back(in.first);
            std::sort(names.begin(), names.end());
            if (std::adjacent_find(names.begin(), names.end()) != names.end()) {
                std::cerr << "error: samples listed more than once (multi-entry samples) are not part of this build\n";
                return 2;
            }
        }
        const bool timing = std::getenv("SKL_CLI_TIMING") != nullptr;
        const auto t_start = std::chrono::steady_clock::now();
        auto since_start = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
        double t_parse = 0, t_pack = 0, t_device = 0;   // (the CPU path parses and hashes sample by sample: all of it under parse)
        std::optional<std::vector<std::string>> labels;
        std::vector<size_t> order(inputs.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = i;
        try {
            if (species_names) {
                log.info("Reordering samples using labels in " + *species_names);
                order = reorder_by_labels(inputs, *species_names, &labels);
            }
            log.info("Creating sketches");
            std::vector<std::vector<uint16_t>> sketches(inputs.size());
            std::vector<std::string> names(inputs.size());
            const double t_sketch0 = since_start();
            if (gpu >= 0) {
                log.info("Sketching on GPU " + std::to_string(gpu));
                Device dev(gpu);   // ("no CPU path" without a device: no fallback to the host loop)
                std::vector<std::vector<uint16_t>> rows =
                    sketch_inverted_gpu(dev, inputs, kmer, sketch_size, !single_strand, threads, min_count, min_qual, &t_parse, &t_pack, &t_device);
                for (size_t i = 0; i < inputs.size(); ++i) {
                    sketches[order[i]] = std::move(rows[i]);
                    names[order[i]] = inputs[i].first;
                }
            } else {
                std::atomic<size_t> next{0};
                std::exception_ptr err;
                std::mutex mu;
                auto work = [&] {
                    try {
                        for (;;) {
                            const size_t i = next.fetch_add(1);
                            if (i >= inputs.size()) break;
                            sketches[order[i]] = sketch_sample_inverted(inputs[i], kmer, sketch_size, !single_strand, min_count, min_qual);
                            names[order[i]] = inputs[i].first;
                        }
                    } catch (...) {
                        std::lock_guard<std::mutex> lk(mu);
                        err = std::current_exception();
                    }
                };
                std::vector<std::thread> pool;
                for (size_t t = 1; t < threads; ++t) pool.emplace_back(work);
                work();
                for (auto &t : pool) t.join();
                if (err) std::rethrow_exception(err);
                t_parse = since_start() - t_sketch0;
            }
            const double t_sketched = since_start();
            double t_write = 0;
            if (write_skq_flag) {
                log.info("Writing bins for use with precluster as " + *output + ".skq");
                write_skq(*output + ".skq", sketches);
                t_write = since_start() - t_sketched;
            }
            log.info("Inverting sketch order");
            const double t_invert0 = since_start();
            Inverted inv = Inverted::from_sketches(sketches, names, kmer, !single_strand);
            const double t_invert = since_start() - t_invert0;
            inv.labels = labels;
            if (metadata_file) {   // parse_metadata_info, src/io.rs:118-137; lib.rs:557-568
                std::ifstream mf(*metadata_file);
                if (!mf) throw std::runtime_error("Unable to open species name file " + *metadata_file);
                std::map<std::string, std::string> dict;
                std::string line;
                while (std::getline(mf, line)) {
                    const size_t tab = line.find('\t');
                    const std::string key = line.substr(0, tab);
                    std::string val = tab == std::string::npos ? "" : line.substr(tab + 1);
                    const size_t tab2 = val.find('\t');
                    if (tab2 != std::string::npos) val.resize(tab2);
                    if (!dict.emplace(key, val).second) throw std::runtime_error("Some entry in metadata is duplicated");
                }
                log.info("Got metadata for " + std::to_string(dict.size()) + " labels");
                std::vector<std::string> md(inputs.size());
                for (size_t i = 0; i < inputs.size(); ++i) {
                    const auto it = dict.find(inputs[i].first);
                    if (it == dict.end()) throw std::runtime_error("no metadata for sample " + inputs[i].first);
                    md[order[i]] = it->second;
                }
                inv.metadata = md;
            }
            const double t_save0 = since_start();
            inv.save(*output);
            t_write += since_start() - t_save0;
            if (timing) {
                std::fprintf(stderr, "TIMING inverted build: parse=%.3fs pack=%.3fs device=%.3fs invert=%.3fs write=%.3fs total=%.3fs\n",
                             t_parse, t_pack, t_device, t_invert, t_write, since_start());
            }
        } catch (const std::exception &e) {
            throw Panic(e.what());
        }
        return 0;
    }
    if (sub != "precluster") {
        std::cerr << "error: unrecognized subcommand 'inverted " << sub << "' (this build provides `inverted build`, `inverted query` and `inverted precluster`)\n";
        return 2;
    }
    g_usage = "sketchlib inverted precluster [OPTIONS] <SKI> <--skd <SKD>|--count>";
    std::optional<std::string> ski, skd, output, completeness_file, retain;
    bool count = false, ani = false, host_candidates = false;
    int knn_ties = SKL_KNN_TIES_REFERENCE;
    size_t knn = 50, threads = 1;   // DEFAULT_KNN, cli.rs
    double cutoff = 0.64;
    int device = 0;
    for (int i = first + 1; i < argc; ++i) {
        const std::string arg = argv[i];
        if (arg == "-v" || arg == "--verbose") verbose = true;
        else if (arg == "--quiet") quiet = true;
        else if (arg == "--skd") skd = next_value(i, "--skd <SKD>");
        else if (arg == "-o") output = next_value(i, "-o <OUTPUT>");
        else if (arg == "--count") count = true;
        else if (arg == "--knn") knn = parse_usize("--knn <KNN>", next_value(i, arg));
        else if (arg == "--ani") ani = true;
        else if (arg == "--threads") threads = std::max<size_t>(1, parse_usize("--threads <THREADS>", next_value(i, arg)));
        else if (arg == "--ref-completeness-file") completeness_file = next_value(i, arg);
        else if (arg == "--completeness-cutoff") cutoff = std::strtod(next_value(i, arg).c_str(), nullptr);
        else if (arg == "--retain-unmatched") retain = next_value(i, arg);
        else if (arg == "--device") device = (int)parse_usize("--device <D>", next_value(i, arg));
        else if (arg == "--host-candidates") host_candidates = true;   // candidate lists from the .ski on host threads
        else if (arg == "--knn-ties") {   // as `dist --knn-ties`: reference (default) | canonical
            const std::string v = next_value(i, "--knn-ties <RULE>");
            if (v == "canonical") knn_ties = SKL_KNN_TIES_CANONICAL;
            else if (v == "reference") knn_ties = SKL_KNN_TIES_REFERENCE;
            else usage_error("invalid value '" + v + "' for '--knn-ties <RULE>': possible values: canonical, reference");
        }
        else if (arg.size() > 1 && arg[0] == '-') usage_error("unexpected argument '" + arg + "' found");
        else if (!ski) ski = arg;
        else usage_error("unexpected argument '" + arg + "' found");
    }
    if (!ski) usage_error("the following required arguments were not provided:\n  <SKI>");
    if (count && skd) usage_error("the argument '--skd <SKD>' cannot be used with '--count'");
    using distances::RetainUnmatched;
    RetainUnmatched retain_mode = RetainUnmatched::None;
    if (retain) {
        if (*retain == "singleton") retain_mode = RetainUnmatched::Singleton;
        else if (*retain == "bruteforce") retain_mode = RetainUnmatched::Bruteforce;
        else usage_error("invalid value '" + *retain + "' for '--retain-unmatched <RETAIN_UNMATCHED>'\n  [possible values: singleton, bruteforce]");
    }
    const Logger log{verbose && !quiet, !quiet};
    log.info("Using " + std::to_string(threads) + " threads");
    const bool timing = std::getenv("SKL_CLI_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto since_start = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    const std::string input_prefix = strip_sketch_extension(*ski);
    // (as in `dist`: the device context comes up while the .ski, the .skq and the .skd are read)
    std::future<std::unique_ptr<Device>> dev_starting;
    if (skd && !count) dev_starting = std::async(std::launch::async, [device] { return std::make_unique<Device>(device); });
    // The bitmaps of the index are only needed for --count and for the host candidate search;
    // by default the candidates are found on the device from the .skq alone.
    Inverted inv = Inverted::load(input_prefix, count || host_candidates);   // `?` in the reference: Error, exit 1
    if (!inv.has_index() && inv.sample_names.size() > skl_shared_bins_max_samples()) {
        log.info("More samples than the on-device candidate search takes: using the index on the host");
        inv = Inverted::load(input_prefix, true);
    }
    const double t_ski = since_start();
    if (count) {
        const size_t ns = inv.sample_names.size();
        std::cout << "Identified " << inv.any_shared_bin_pairs(threads) << " prefilter pairs from a max of "
                  << ns * (ns - 1) / 2 << "\n";
        return 0;
    }
    if (!skd) return 0;   // neither mode: the reference does nothing (lib.rs:713)
    std::ostream *os = &std::cout;
    std::unique_ptr<TextSink> sink;
    if (output) {
        try {
            sink = std::make_unique<FileSink>(*output);
        } catch (const std::exception &e) {
            throw Panic(e.what());
        }
    } else {
        sink = std::make_unique<StreamSink>(*os);
    }
    const std::string skq_filename = input_prefix + ".skq";
    log.info("Loading queries from " + skq_filename);
    std::vector<uint16_t> skq_bins;
    try {
        skq_bins = read_skq(skq_filename, inv.sample_names.size(), inv.sketch_size());
    } catch (const std::exception &e) {
        throw Panic(e.what());
    }
    const std::string ref_db_name = strip_sketch_extension(*skd);
    MultiSketch references;
    try {
        references = MultiSketch::load_metadata(ref_db_name);
    } catch (const std::exception &) {
        throw Panic("Could not read sketch metadata from " + ref_db_name + ".skm");
    }
    if (references.kmer_lengths().size() > 1 && references.get_k_idx(inv.kmer_size)) {
        references.select_kmer(*references.get_k_idx(inv.kmer_size));   // (as in `dist -k`: the one slice the distances read)
    }
    log.info("Loading sketch data from " + ref_db_name + ".skd");
    references.read_sketch_data(ref_db_name);
    const size_t n = references.number_samples_loaded();
    if (knn_ties == SKL_KNN_TIES_REFERENCE && !inv.has_index() && !distances::ski_order_is_skd_order(references, inv)) {
        // the reference pushes a row's candidates in ascending .ski index (mod.rs:459-487); lists built on the device are
        // ascending in .skd order, so with a .ski that orders the samples differently they come from the index, on the host
        log.info("The .ski orders the samples differently from the .skd: candidate lists from the index on the host "
                 "(--knn-ties canonical keeps them on the device)");
        inv = Inverted::load(input_prefix, true);
    }
    if (knn >= n) {   // lib.rs:737-740
        log.warn("knn=" + std::to_string(knn) + " is higher than number of samples=" + std::to_string(n));
        knn = n - 1;
    }
    if (knn == 0) throw Panic("chunk size must be non-zero");
    DistType dist_type;
    try {
        dist_type = distances::set_k(references, inv.kmer_size, ani);
    } catch (const std::exception &e) {
        throw Panic("K-mer size " + std::to_string(inv.kmer_size) + " used for .ski not found in .skd: " + e.what());
    }
    std::optional<std::vector<double>> comp;
    if (completeness_file) {
        std::vector<std::string> warnings;
        comp = read_completeness_file(*completeness_file, references, &warnings);
        for (const auto &w : warnings) log.warn(w);
    }
    log.info("Calculating sparse ref vs ref distances with " + std::to_string(knn) + " nearest neighbours");
    log.info("Preclustering with k=" + std::to_string(inv.kmer_size) + " and s=" + std::to_string(inv.sketch_size()));
    if (retain) log.info("Retain unmatched mode: " + *retain);
    const double t_loaded = since_start();
    const std::unique_ptr<Device> dev_owner = dev_starting.get();
    Device &dev = *dev_owner;
    const double t_device = since_start();
    if (comp && (skl_ctx_flags(dev.ctx()) & SKL_CTX_FLAG_LOG_UNMATCHED)) log.warn(LOG_UNMATCHED_WARNING);
    const SparseDistanceMatrix d = distances::self_dists_knn_precluster(
        dev, references, inv, skq_bins, inv.sketch_size(), n, knn, dist_type, comp ? &*comp : nullptr, cutoff,
        retain_mode, threads, knn_ties);
    const double t_dist = since_start();
    log.info("Writing out in sparse matrix form");
    d.write(*sink, threads);
    os->flush();
    if (timing) {
        std::fprintf(stderr, "TIMING precluster: load_ski=%.3fs load_skq+skd=%.3fs device_wait=%.3fs candidates+distances=%.3fs write=%.3fs\n",
                     t_ski, t_loaded - t_ski, t_device - t_loaded, t_dist - t_device, since_start() - t_dist);
    }
    g_listing_complete = true;
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    const auto start = std::chrono::steady_clock::now();
    // global flags may precede the subcommand
    int sub = 1;
    while (sub < argc && (strcmp(argv[sub], "-v") == 0 || strcmp(argv[sub], "--verbose") == 0 ||
                          strcmp(argv[sub], "--quiet") == 0)) {
        ++sub;
    }
    if (sub >= argc || strcmp(argv[sub], "-h") == 0 || strcmp(argv[sub], "--help") == 0) {
        std::cout << "Usage: sketchlib [OPTIONS] <COMMAND>\n\nCommands:\n"
                     "  sketch  Create sketches from input data (DNA assemblies and read sets, amino-acid sequences; CPU, or GPU with --gpu)\n"
                     "  dist    Calculate pairwise distances using sketches (GPU)\n"
                     "  inverted build|query|precluster  Inverted index of single-k sketches of DNA assemblies and read sets (CPU, or GPU\n"
                     "                                   with --gpu); match queries against it (GPU; --gpu sketches the queries there too);\n"
                     "                                   kNN restricted to its candidates (GPU)\n"
                     "  merge   Merge two sketch databases (.skm and .skd pair) into a new one (files only)\n"
                     "  append  Sketch new samples the way a database was sketched and write both as a new database, the new\n"
                     "          samples first (CPU, or GPU with --gpu)\n"
                     "  delete  Write a database without the samples listed in a file (files only)\n"
                     "  info    Print information about a .skm or .ski file (files only)\n";
        return sub >= argc ? 2 : 0;
    }
    if (strcmp(argv[sub], "sketch") == 0) {
        bool verbose = false, quiet = false;
        for (int i = 1; i < sub; ++i) {
            if (strcmp(argv[i], "--quiet") == 0) quiet = true;
            else verbose = true;
        }
        try {
            return run_sketch(argc, argv, sub + 1, verbose, quiet);
        } catch (const Panic &p) {
            std::cerr << "thread 'main' panicked:\n" << p.what() << "\n";
            return 101;
        } catch (const std::exception &e) {
            std::cerr << "Error: " << e.what() << "\n";
            return 1;
        }
    }
    if (strcmp(argv[sub], "inverted") == 0) {
        bool verbose = false, quiet = false;
        for (int i = 1; i < sub; ++i) {
            if (strcmp(argv[i], "--quiet") == 0) quiet = true;
            else verbose = true;
        }
        try {
            const int rc = run_inverted(argc, argv, sub + 1, verbose, quiet);
            if (verbose && !quiet) {
                const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
                std::cerr << "INFO  [sketchlib] Complete in " << s << "s\n";  // lib.rs:949-957
            }
            return leave_after_success(rc);
        } catch (const Panic &p) {
            std::cerr << "thread 'main' panicked:\n" << p.what() << "\n";
            return 101;
        } catch (const std::exception &e) {
            std::cerr << "Error: " << e.what() << "\n";
            return 1;
        }
    }
    const bool is_merge = strcmp(argv[sub], "merge") == 0, is_append = strcmp(argv[sub], "append") == 0;
    const bool is_delete = strcmp(argv[sub], "delete") == 0, is_info = strcmp(argv[sub], "info") == 0;
    if (is_merge || is_append || is_delete || is_info) {
        bool verbose = false, quiet = false;
        for (int i = 1; i < sub; ++i) {
            if (strcmp(argv[i], "--quiet") == 0) quiet = true;
            else verbose = true;
        }
        try {
            if (is_merge) return run_merge(argc, argv, sub + 1);
            if (is_delete) return run_delete(argc, argv, sub + 1);
            if (is_info) return run_info(argc, argv, sub + 1);
            return run_append(argc, argv, sub + 1, verbose, quiet);
        } catch (const Panic &p) {
            std::cout.flush();
            std::cerr << "thread 'main' panicked:\n" << p.what() << "\n";
            return 101;
        } catch (const std::exception &e) {
            std::cerr << "Error: " << e.what() << "\n";
            return 1;
        }
    }
    if (strcmp(argv[sub], "dist") != 0) {
        std::cerr << "error: unrecognized subcommand '" << argv[sub]
                  << "' (this build provides `sketch` (DNA assemblies and read sets), `dist` (GPU) and `inverted build|query|precluster`"
                     ", and the database commands `merge`, `append`, `delete` and `info`)\n";
        return 2;
    }
    DistArgs args = parse_dist(argc, argv, sub + 1);
    for (int i = 1; i < sub; ++i) {
        if (strcmp(argv[i], "--quiet") == 0) args.quiet = true;
        else args.verbose = true;
    }
    try {
        const int rc = run_dist(args);
        if (args.verbose && !args.quiet) {
            const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
            std::cerr << "INFO  [sketchlib] Complete in " << s << "s\n";  // lib.rs:949-957
        }
        return leave_after_success(rc);
    } catch (const Panic &p) {
        std::cerr << "thread 'main' panicked:\n" << p.what() << "\n";
        return 101;
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << "\n";
        return 1;
    }
}
