// inverted.cpp -- `sketchlib inverted build | query | precluster` (src/cli.rs:329-461, src/lib.rs:485-789)
#include "../inverted.hpp"

#include <algorithm>
#include <charconv>
#include <cstdio>
#include <fstream>
#include <map>

#include "../sketch.hpp"
#include "common.hpp"
#include "sketchlib_dist.h"

namespace skl_cli {

int run_inverted_build(int argc, char **argv, int first, Verbosity &global, const char *)
{
    Verbosity verbosity = global;   // (-v here: INFO lines, not main()'s "Complete in")
    SketchInputArgs in(/* --single-strand */ true);
    std::optional<std::string> output, species_names, metadata_file;
    bool write_skq_flag = false;
    uint64_t sketch_size = 1000;   // DEFAULT_SKETCHSIZE, cli.rs:17
    size_t kmer = 21;              // DEFAULT_KMER, cli.rs:13
    ArgReader r(argc, argv, first);
    while (r.next()) {
        if (verbosity.accept(r) || in.accept(r)) continue;
        else if (r.is("-o")) output = r.value("-o <OUTPUT>");
        else if (r.is("--write-skq")) write_skq_flag = true;
        else if (r.is("--species-names")) species_names = r.value(r.arg());
        else if (r.is("--metadata")) metadata_file = r.value(r.arg());
        else if (r.is("-s", "--sketch-size")) sketch_size = usize("--sketch-size <SKETCH_SIZE>", r.value(r.arg()));
        else if (r.is("-k", "--kmer-length")) kmer = usize("--kmer-length <KMER_LENGTH>", r.value(r.arg()));
        else if (r.is_option()) r.unexpected();
        else in.seq_files.push_back(r.arg());
    }
    require({{output.has_value(), "-o <OUTPUT>"}});
    in.check();
    const Logger log(verbosity);
    log.info("Getting input files");
    const std::vector<InputFastx> inputs = in.file_list ? read_rfile(*in.file_list) : read_input_fastas(in.seq_files);
    log.info("Parsed " + std::to_string(inputs.size()) + " samples in input list");
    {
        std::vector<std::string> names;
        for (const auto &input : inputs) names.push_back(input.first);
        std::sort(names.begin(), names.end());
        if (std::adjacent_find(names.begin(), names.end()) != names.end()) {
            std::cerr << "error: samples listed more than once (multi-entry samples) are not part of this build\n";
            return 2;
        }
    }
    const Stopwatch watch;
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
        const double t_sketch0 = watch.seconds();
        if (in.sketch_device >= 0) {
            log.info("Sketching on GPU " + std::to_string(in.sketch_device));
            Device dev(in.sketch_device);   // ("no CPU path" without a device: no fallback to the host loop)
            std::vector<std::vector<uint16_t>> rows = sketch_inverted_gpu(dev, inputs, kmer, sketch_size, !in.single_strand, in.threads,
                                                                         in.min_count, in.min_qual, &t_parse, &t_pack, &t_device);
            for (size_t i = 0; i < inputs.size(); ++i) {
                sketches[order[i]] = std::move(rows[i]);
                names[order[i]] = inputs[i].first;
            }
        } else {
            parallel_for_index(inputs.size(), in.threads, [&](size_t i) {
                sketches[order[i]] = sketch_sample_inverted(inputs[i], kmer, sketch_size, !in.single_strand, in.min_count, in.min_qual);
                names[order[i]] = inputs[i].first;
            });
            t_parse = watch.seconds() - t_sketch0;
        }
        const double t_sketched = watch.seconds();
        double t_write = 0;
        if (write_skq_flag) {
            log.info("Writing bins for use with precluster as " + *output + ".skq");
            write_skq(*output + ".skq", sketches);
            t_write = watch.seconds() - t_sketched;
        }
        log.info("Inverting sketch order");
        const double t_invert0 = watch.seconds();
        Inverted inv = Inverted::from_sketches(sketches, names, kmer, !in.single_strand);
        const double t_invert = watch.seconds() - t_invert0;
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
        const double t_save0 = watch.seconds();
        inv.save(*output);
        t_write += watch.seconds() - t_save0;
        if (watch.report) {
            std::fprintf(stderr, "TIMING inverted build: parse=%.3fs pack=%.3fs device=%.3fs invert=%.3fs write=%.3fs total=%.3fs\n",
                         t_parse, t_pack, t_device, t_invert, t_write, watch.seconds());
        }
    } catch (const std::exception &e) {
        throw Panic(e.what());
    }
    return 0;
}

namespace {

// One band of `inverted query` results as text.
struct QueryBand {
    const Inverted &inv;
    const std::vector<InputFastx> &inputs;
    int mode;      // SKL_INVQ_*
    size_t top;    // --top N, 0 = every count
    size_t q0, rows;             // the band's queries: inputs[q0 .. q0 + rows)
    const uint64_t *buf;         // top: ids [rows][top] then counts [rows][top], u32; match-count: [rows][n] u32; else [rows][words64] bits

    void format_row(size_t r, std::string &o) const
    {
        const size_t n = inv.sample_names.size(), S = inv.sketch_size(), words64 = (n + 63) / 64;
        char num[16];
        if (top) {   // one line per hit, best first; fewer than `top` lines when the index is smaller
            const uint32_t *ids = reinterpret_cast<const uint32_t *>(buf) + r * top, *cnt = ids + rows * top;
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
            return;
        }
        o += inputs[q0 + r].first;
        if (mode == SKL_INVQ_MATCH_COUNT) {
            const uint32_t *c = reinterpret_cast<const uint32_t *>(buf) + r * n;
            for (size_t s = 0; s < n; ++s) {
                num[0] = '\t';
                o.append(num, std::to_chars(num + 1, num + sizeof num, c[s]).ptr);
            }
        } else {
            const uint64_t *bits = buf + r * words64;
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

    // the band's rows on `threads` threads, in contiguous pieces to be written in order
    std::vector<std::string> format(size_t threads) const
    {
        const size_t n_pieces = std::min(rows, threads);
        std::vector<std::string> pieces(n_pieces);
        parallel_for_index(n_pieces, n_pieces, [&](size_t piece) {
            for (size_t r = rows * piece / n_pieces; r < rows * (piece + 1) / n_pieces; ++r) format_row(r, pieces[piece]);
        });
        return pieces;
    }
};

}  // namespace

// Queries (assemblies or read sets, --min-count / --min-qual as in `sketch`) are sketched the way the index was built
// (Inverted::sketch_queries, inverted.rs:118-140) -- on host threads, or with --gpu on the device --device names
// (sketch_inverted_gpu) -- then matched against every indexed sample on the GPU (skl_inverted_query, csrc/inv_query.hip), one band of
// queries at a time: band i + 1 computes while band i is formatted on --threads threads and written.  Rows come in
// input order (the reference's come in whatever order its threads finish).
// --top N (match-count only): the N best hits of every query instead of every count -- the reference's identification
// query (SketchlibData::query / get_probs, src/lib.rs:1019-1109), selected on the device (skl_inverted_query_top,
// csrc/inv_top.hip) -- in long form, one line per hit with d / (2 S - d) and the index's label and metadata.
int run_inverted_query(int argc, char **argv, int first, Verbosity &global, const char *)
{
    Verbosity verbosity = global;
    SketchInputArgs in(/* --single-strand */ false);
    std::optional<std::string> ski, output;
    int mode = SKL_INVQ_MATCH_COUNT;
    std::string mode_name = "match-count";
    size_t top = 0;           // --top N: 0 = every count (the default)
    bool query_type_given = false;
    ArgReader r(argc, argv, first);
    while (r.next()) {
        if (verbosity.accept(r) || in.accept(r)) continue;
        else if (r.is("-o")) output = r.value("-o <OUTPUT>");
        else if (r.is("--top")) top = bounded("--top <N>", r.value("--top <N>"), 1, SKL_INVQ_TOP_MAX);   // the hits of a query are held in the kernel's LDS list
        else if (r.is("--query-type")) {
            query_type_given = true;
            mode_name = r.value("--query-type <QUERY_TYPE>");
            static const int modes[] = {SKL_INVQ_MATCH_COUNT, SKL_INVQ_ALL_BINS, SKL_INVQ_ANY_BINS};
            mode = modes[choice("--query-type <QUERY_TYPE>", mode_name, {"match-count", "all-bins", "any-bins"}, ChoiceStyle::Block)];
        }
        else if (r.is_option()) r.unexpected();
        else if (!ski) ski = r.arg();
        else in.seq_files.push_back(r.arg());
    }
    if (top && query_type_given && mode != SKL_INVQ_MATCH_COUNT) conflict("--top <N>", "--query-type <QUERY_TYPE>");
    require({{ski.has_value(), "<SKI>"}});
    in.check();
    const Logger log(verbosity);
    const Stopwatch watch;
    // (as in `precluster`: the device comes up while the .ski is read; a device that failed to come up is only reported
    // where it is first needed, after every error of the .ski and of the inputs)
    std::future<std::unique_ptr<Device>> dev_starting = start_device(in.device);
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
    const double t_load = watch.seconds();

    log.info("Getting input queries");
    const std::vector<InputFastx> inputs = in.file_list ? read_rfile(*in.file_list) : read_input_fastas(in.seq_files);
    log.info("Parsed " + std::to_string(inputs.size()) + " samples in input query list");
    log.info("Sketching input queries");
    const size_t nq = inputs.size();
    std::vector<uint16_t> query_bins(nq * S);
    std::unique_ptr<Device> dev_owner;
    try {
        if (in.gpu) {
            dev_owner = dev_starting.get();   // ("no CPU path" without a device: no fallback to the host loop)
            const std::vector<std::vector<uint16_t>> rows =
                sketch_inverted_gpu(*dev_owner, inputs, inv.kmer_size, S, inv.rc, in.threads, in.min_count, in.min_qual);
            for (size_t i = 0; i < nq; ++i) std::copy(rows[i].begin(), rows[i].end(), query_bins.begin() + i * S);
        } else {
            parallel_for_index(nq, std::min(in.threads, nq), [&](size_t i) {
                const std::vector<uint16_t> q = sketch_sample_inverted(inputs[i], inv.kmer_size, S, inv.rc, in.min_count, in.min_qual);
                std::copy(q.begin(), q.end(), query_bins.begin() + i * S);
            });
        }
    } catch (const std::exception &e) {
        throw Panic(e.what());   // the reference panics on unreadable / empty input
    }
    const double t_sketch = watch.seconds();

    const std::unique_ptr<TextSink> sink = open_sink(output);
    auto write = [&](const std::string &text) {
        if (!text.empty()) sink->finish(sink->begin(text.data(), text.size()), text.data(), text.size());
    };

    if (!dev_owner) dev_owner = dev_starting.get();
    Device &dev = *dev_owner;
    skl_inverted *ix = nullptr;
    if (skl_inverted_create(dev.ctx(), index_bins.data(), n, S, &ix) != SKL_OK) throw std::runtime_error(skl_last_error());
    std::unique_ptr<skl_inverted, int (*)(skl_inverted *)> ix_owner(ix, skl_inverted_destroy);
    const double t_device = watch.seconds();

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
    // (--top: a band's ids [rows][top], then its counts [rows][top])
    const size_t row_bytes = std::max<size_t>(1, top ? top * 2 * sizeof(uint32_t) : mode == SKL_INVQ_MATCH_COUNT ? n * sizeof(uint32_t) : (n + 63) / 64 * sizeof(uint64_t));
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
        const double t0 = watch.seconds();
        const std::vector<uint64_t> buf = pending.get();
        if (q0 + band < nq) pending = std::async(std::launch::async, compute, q0 + band);
        const double t1 = watch.seconds();
        const QueryBand rows{inv, inputs, mode, top, q0, std::min(band, nq - q0), buf.data()};
        for (const auto &piece : rows.format(in.threads)) write(piece);
        t_query += t1 - t0;
        t_write += watch.seconds() - t1;
    }
    std::cout.flush();
    if (watch.report) {
        std::fprintf(stderr, "TIMING inverted query: load=%.3fs sketch=%.3fs device=%.3fs query=%.3fs write=%.3fs\n",
                     t_load, t_sketch - t_load, t_device - t_sketch, t_query, t_write);
    }
    g_listing_complete = true;
    return 0;
}

int run_inverted_precluster(int argc, char **argv, int first, Verbosity &global, const char *)
{
    Verbosity verbosity = global;
    std::optional<std::string> ski, skd, output, completeness_file, retain;
    bool count = false, ani = false, host_candidates = false;
    int knn_ties = SKL_KNN_TIES_REFERENCE;
    size_t knn = 50, threads = 1;   // DEFAULT_KNN, cli.rs
    double cutoff = 0.64;
    int device = 0;
    ArgReader r(argc, argv, first);
    while (r.next()) {
        if (verbosity.accept(r)) continue;
        else if (r.is("--skd")) skd = r.value("--skd <SKD>");
        else if (r.is("-o")) output = r.value("-o <OUTPUT>");
        else if (r.is("--count")) count = true;
        else if (r.is("--knn")) knn = usize("--knn <KNN>", r.value(r.arg()));
        else if (r.is("--ani")) ani = true;
        else if (r.is("--threads")) threads = threads_lenient("--threads <THREADS>", r.value(r.arg()));
        else if (r.is("--ref-completeness-file")) completeness_file = r.value(r.arg());
        else if (r.is("--completeness-cutoff")) cutoff = std::strtod(r.value(r.arg()).c_str(), nullptr);   // (a word reads as 0)
        else if (r.is("--retain-unmatched")) retain = r.value(r.arg());
        else if (r.is("--device")) device = (int)usize("--device <D>", r.value(r.arg()));
        else if (r.is("--host-candidates")) host_candidates = true;   // candidate lists from the .ski on host threads
        else if (r.is("--knn-ties")) knn_ties = knn_ties_canonical(r) ? SKL_KNN_TIES_CANONICAL : SKL_KNN_TIES_REFERENCE;   // as `dist --knn-ties`
        else if (r.is_option() || ski) r.unexpected();
        else ski = r.arg();
    }
    require({{ski.has_value(), "<SKI>"}});
    if (count && skd) conflict("--skd <SKD>", "--count");
    using distances::RetainUnmatched;
    RetainUnmatched retain_mode = RetainUnmatched::None;
    if (retain) {
        static const RetainUnmatched modes[] = {RetainUnmatched::Singleton, RetainUnmatched::Bruteforce};
        retain_mode = modes[choice("--retain-unmatched <RETAIN_UNMATCHED>", *retain, {"singleton", "bruteforce"}, ChoiceStyle::Block)];
    }
    const Logger log(verbosity);
    log.info("Using " + std::to_string(threads) + " threads");
    const Stopwatch watch;
    const std::string input_prefix = strip_sketch_extension(*ski);
    // (as in `dist`: the device context comes up while the .ski, the .skq and the .skd are read)
    std::future<std::unique_ptr<Device>> dev_starting;
    if (skd && !count) dev_starting = start_device(device);
    // The bitmaps of the index are only needed for --count and for the host candidate search;
    // by default the candidates are found on the device from the .skq alone.
    Inverted inv = Inverted::load(input_prefix, count || host_candidates);   // `?` in the reference: Error, exit 1
    if (!inv.has_index() && inv.sample_names.size() > skl_shared_bins_max_samples()) {
        log.info("More samples than the on-device candidate search takes: using the index on the host");
        inv = Inverted::load(input_prefix, true);
    }
    const double t_ski = watch.seconds();
    if (count) {
        const size_t ns = inv.sample_names.size();
        std::cout << "Identified " << inv.any_shared_bin_pairs(threads) << " prefilter pairs from a max of "
                  << ns * (ns - 1) / 2 << "\n";
        return 0;
    }
    if (!skd) return 0;   // neither mode: the reference does nothing (lib.rs:713)
    const std::unique_ptr<TextSink> sink = open_sink(output);
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
    const double t_loaded = watch.seconds();
    const std::unique_ptr<Device> dev_owner = dev_starting.get();
    Device &dev = *dev_owner;
    const double t_device = watch.seconds();
    if (comp) warn_if_log_unmatched(log, dev.ctx());
    const SparseDistanceMatrix d = distances::self_dists_knn_precluster(
        dev, references, inv, skq_bins, inv.sketch_size(), n, knn, dist_type, comp ? &*comp : nullptr, cutoff,
        retain_mode, threads, knn_ties);
    const double t_dist = watch.seconds();
    log.info("Writing out in sparse matrix form");
    d.write(*sink, threads);
    std::cout.flush();
    if (watch.report) {
        std::fprintf(stderr, "TIMING precluster: load_ski=%.3fs load_skq+skd=%.3fs device_wait=%.3fs candidates+distances=%.3fs write=%.3fs\n",
                     t_ski, t_loaded - t_ski, t_device - t_loaded, t_dist - t_device, watch.seconds() - t_dist);
    }
    g_listing_complete = true;
    return 0;
}

}  // namespace skl_cli
