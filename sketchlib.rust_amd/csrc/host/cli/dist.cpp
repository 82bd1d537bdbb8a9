// dist.cpp -- `sketchlib dist`, the reference's command line for this path (src/cli.rs:185-231, src/lib.rs:303-453) on
// top of the gfx950 engine.
//
// Same positional arguments, flags, defaults, stdout format and exit behaviour (panic -> 101, error -> 1, usage -> 2).
// `--threads` (default 1, as in the reference) sets the host threads that format the dense text output; the distances
// themselves run on the GPU.  `--device` is the one addition.
#include <algorithm>
#include <cstdio>

#include "common.hpp"
#include "sketchlib_dist.h"

namespace skl_cli {
namespace {

// clap's syntax in full: --flag=value, -k21, -oFILE
const Syntax DIST_SYNTAX{/* --flag=value */ true, /* attached values */ "ok"};

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

DistArgs parse_dist(int argc, char **argv, int first, Verbosity &verbosity)
{
    DistArgs a;
    std::vector<std::string> positional;
    ArgReader r(argc, argv, first, DIST_SYNTAX);
    while (r.next()) {
        if (r.is_help()) { print_help(); throw HelpRequested{}; }
        else if (verbosity.accept(r)) continue;
        else if (r.is("-o")) a.output = r.value("-o <OUTPUT>");
        else if (r.is("--knn")) a.knn = usize("--knn <KNN>", r.value("--knn <KNN>"));
        else if (r.is("--knn-ties")) a.knn_ties = knn_ties_canonical(r) ? SKL_KNN_TIES_CANONICAL : SKL_KNN_TIES_REFERENCE;
        else if (r.is("--subset")) a.subset = r.value("--subset <SUBSET>");
        else if (r.is("--pairs")) a.pairs = r.value("--pairs <FILE>");
        else if (r.is("-k")) a.kmer = usize("-k <KMER>", r.value("-k <KMER>"));
        else if (r.is("--ani")) a.ani = true;
        else if (r.is("--threads")) a.threads = threads_strict("--threads <THREADS>", r.value("--threads <THREADS>"));
        else if (r.is("--ref-completeness-file")) a.ref_completeness_file = r.value(r.arg());
        else if (r.is("--query-completeness-file")) a.query_completeness_file = r.value(r.arg());
        else if (r.is("--completeness-cutoff")) a.completeness_cutoff = float_strict("--completeness-cutoff <COMPLETENESS_CUTOFF>", r.value(r.arg()));
        else if (r.is("--device")) a.devices = {(int)usize("--device <D>", r.value(r.arg()))};
        else if (r.is("--npy")) a.npy = true;
        else if (r.is("--band-mb")) a.band_bytes = std::max<size_t>(1, usize("--band-mb <MB>", r.value(r.arg()))) << 20;
        else if (r.is("--gpus")) {
            const size_t ngpu = usize("--gpus <N>", r.value(r.arg()));
            a.multi_device_flag = "--gpus <N>";
            if (ngpu < 1) throw UsageError{"invalid value for '--gpus <N>': must be one or higher"};
            a.devices.clear();
            for (size_t d = 0; d < ngpu; ++d) a.devices.push_back((int)d);
        }
        else if (r.is("--devices")) {
            a.multi_device_flag = "--devices <LIST>";
            a.devices.clear();
            for (const size_t d : list("--devices <LIST>", r.value(r.arg()))) a.devices.push_back((int)d);
        }
        else if (r.is_option()) r.unexpected();
        else positional.push_back(r.arg());
    }
    require({{!positional.empty(), "<REF_DB>"}});
    if (positional.size() > 2) unexpected(positional[2]);
    a.ref_db = positional[0];
    if (positional.size() == 2) a.query_db = positional[1];
    if (a.ani) require({{a.kmer.has_value(), "-k <KMER>"}});   // #[arg(long, requires("kmer"))]
    if (a.pairs) {   // a list of pairs is neither a neighbour search nor a subset, and runs on one device as text
        const char *other = a.knn ? "--knn <KNN>" : a.subset ? "--subset <SUBSET>" : a.npy ? "--npy" : nullptr;
        if (other) conflict("--pairs <FILE>", other);
        if (a.multi_device_flag) conflict("--pairs <FILE>", *a.multi_device_flag);
    }
    if (a.npy && (!a.output || a.knn)) throw UsageError{"--npy needs -o <file> and a dense (no --knn) output"};
    return a;
}

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

}  // namespace

int run_dist(int argc, char **argv, int first, Verbosity &verbosity, const char *)
{
    const DistArgs a = parse_dist(argc, argv, first, verbosity);   // (-v here also asks for main()'s "Complete in" line)
    const bool quiet = verbosity.quiet;
    const Stopwatch watch;
    double t_loaded = 0, t_device = 0;
    const Logger log(verbosity);
    log.info("Using " + std::to_string(a.threads) + " threads");   // cli.rs:75-86 (host threads unused)
    if (a.threads > 2 * host_cpu_budget()) {
        log.info("This process may use " + std::to_string(host_cpu_budget()) + " CPUs (affinity / cgroup quota): the output is formatted by " +
                 std::to_string(2 * host_cpu_budget()) + " threads");
    }
    std::future<std::unique_ptr<DeviceSet>> dev_starting = start_devices(a.devices);
    const std::unique_ptr<TextSink> sink = open_sink(a.output);

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

    t_loaded = watch.seconds();
    const std::unique_ptr<DeviceSet> dev_owner = dev_starting.get();
    DeviceSet &dev = *dev_owner;
    t_device = watch.seconds();
    if (a.devices.size() > 1) log.info("Using " + std::to_string(a.devices.size()) + " GPU contexts (row-band partition)");
    for (size_t d = 0; d < dev.size(); ++d) {
        if (skl_ctx_set_knn_ties(dev[d].ctx(), a.knn_ties) != SKL_OK) throw std::runtime_error(skl_last_error());
    }
    if (ref_comp || query_comp) warn_if_log_unmatched(log, dev[0].ctx());
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
                const DistanceMatrix d = distances::self_dists_all(dev, references, n, dist_type, quiet, rc,
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
            const SparseDistanceMatrix d = distances::self_dists_knn(dev, references, n, nn, dist_type, quiet,
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
                                                                      dist_type, quiet, rc, qc,
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
                                                                    quiet, rc, qc, a.completeness_cutoff);
                log.info("Writing out in long matrix form");
                write_whole(d, *sink, n, a);
            }
        }
    }
    std::cout.flush();
    if (watch.report) {
        const OutputTiming &t = output_timing();
        std::fprintf(stderr, "TIMING load=%.3fs device_wait=%.3fs dist+output=%.3fs (gpu_wait=%.3fs format=%.3fs sink=%.3fs)\n",
                     t_loaded, t_device - t_loaded, watch.seconds() - t_device, t.wait_s, t.format_s, t.sink_s);
    }
    g_listing_complete = true;
    return 0;
}

}  // namespace skl_cli
