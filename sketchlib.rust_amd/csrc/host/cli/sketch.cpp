// sketch.cpp -- `sketchlib sketch` (src/cli.rs:121-183, src/lib.rs:242-301: DNA assemblies and read sets, amino-acid
// sequences) and `sketchlib append` (src/cli.rs:240-322, src/lib.rs:793-875), which sketches new samples the way a
// database was sketched: one path from the inputs to the .skd, on the host or with --gpu on the device.
#include "../sketch.hpp"

#include "../dbmaint.hpp"
#include "common.hpp"

namespace skl_cli {
namespace {

void check_concat_fasta(const SeqType &seq)   // lib.rs:258-260, 825-827
{
    if (seq.concat_fasta && !seq.aa) throw Panic("--concat-fasta currently only supported with --seq-type aa");
}

// Writes <output>.skd and returns its metadata.  A device that is asked for and missing is an error, never the host loop.
MultiSketch sketch_inputs(const Logger &log, const SketchInputArgs &in, const std::string &output, const std::vector<InputFastx> &inputs,
                          const std::vector<size_t> &kmers, uint64_t sketch_size, const SeqType &seq)
{
    try {
        if (in.sketch_device >= 0) {
            log.info("Hashing on GPU " + std::to_string(in.sketch_device));
            Device dev(in.sketch_device);
            return sketch_files_gpu(dev, output, inputs, kmers, sketch_size, !in.single_strand, in.threads, in.min_count, in.min_qual, seq);
        }
        return sketch_files(output, inputs, kmers, sketch_size, !in.single_strand, in.threads, in.min_count, in.min_qual, seq);
    } catch (const std::exception &e) {
        throw Panic(e.what());   // the reference panics on unreadable / empty input
    }
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

}  // namespace

int run_sketch(int argc, char **argv, int first, Verbosity &global, const char *)
{
    Verbosity verbosity = global;
    SketchInputArgs in(/* --single-strand */ true);
    std::optional<std::string> output;
    std::vector<size_t> k_vals, k_seq;
    uint64_t sketch_size = 1000;   // DEFAULT_SKETCHSIZE, cli.rs:17
    SeqType seq;
    ArgReader r(argc, argv, first);
    while (r.next()) {
        if (r.is_help()) { print_sketch_help(); throw HelpRequested{}; }
        else if (verbosity.accept(r) || in.accept(r)) continue;
        else if (r.is("-o")) output = r.value("-o <OUTPUT>");
        else if (r.is("-k", "--k-vals")) k_vals = list("--k-vals <K_VALS>", r.value(r.arg()));
        else if (r.is("--k-seq")) k_seq = list("--k-seq <K_SEQ>", r.value(r.arg()));
        else if (r.is("-s", "--sketch-size")) sketch_size = usize("--sketch-size <SKETCH_SIZE>", r.value(r.arg()));
        else if (r.is("--seq-type")) {
            const size_t type = choice("--seq-type <SEQ_TYPE>", r.value(r.arg()), {"dna", "aa", "pdb"}, ChoiceStyle::Block);
            if (type == 2) { std::cerr << "error: structures are not part of this build (--seq-type pdb); it sketches dna and aa\n"; return 2; }
            seq.aa = type == 1;
        }
        else if (r.is("--level")) seq.level = aa_level(r);
        else if (r.is("--concat-fasta")) seq.concat_fasta = true;
        else if (r.is_option()) r.unexpected();
        else in.seq_files.push_back(r.arg());
    }
    require({{output.has_value(), "-o <OUTPUT>"}});
    in.check();
    if (k_vals.empty() == k_seq.empty()) throw UsageError{"exactly one of --k-vals or --k-seq must be given"};
    check_concat_fasta(seq);
    if (!seq.aa) seq.level = 1;   // (--level is read with aa only)
    const Logger log(verbosity);
    const std::vector<InputFastx> inputs = in.file_list ? read_rfile(*in.file_list) : read_input_fastas(in.seq_files);
    log.info("Parsed " + std::to_string(inputs.size()) + " samples in input list");
    const std::vector<size_t> kmers = parse_kmers(k_vals, k_seq);
    const uint64_t bins = (sketch_size + 63) / 64 * 64;
    log.info("Running sketching: sketch_size:" + std::to_string(bins) + " threads:" + std::to_string(in.threads));
    sketch_inputs(log, in, *output, inputs, kmers, sketch_size, seq);
    return 0;
}

// `append`: the new samples are sketched the way the database was (its k-mer lengths, sketch size and sequence type) into
// <out>, the database's blocks follow them, and the metadata is the new samples' with the database's merged in behind
// (lib.rs:857-875).
int run_append(int argc, char **argv, int first, Verbosity &global, const char *usage)
{
    Verbosity verbosity = global;
    SketchInputArgs in(/* --single-strand */ true);
    std::optional<std::string> db, output;
    bool concat_fasta = false;
    std::optional<int> level;
    ArgReader r(argc, argv, first);
    while (r.next()) {
        if (r.is_help()) {
            std::cout <<
                "Append new genomes to be sketched to an existing sketch database\n\nUsage: " << usage << "\n\n"
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
            throw HelpRequested{};
        }
        else if (verbosity.accept(r) || in.accept(r)) continue;
        else if (r.is("-o")) output = r.value("-o <OUTPUT>");
        else if (r.is("--concat-fasta")) concat_fasta = true;
        else if (r.is("--level")) level = aa_level(r);
        else if (r.is_option()) r.unexpected();
        else if (!db) db = r.arg();
        else in.seq_files.push_back(r.arg());
    }
    require({{db.has_value(), "<DB>"}});
    require({{output.has_value(), "-o <OUTPUT>"}});
    in.check();
    const Logger log(verbosity);
    const std::string db_name = strip_sketch_extension(*db);
    if (strip_sketch_extension(*output) == db_name) {
        throw std::runtime_error("the output " + *output + " is the database itself: append writes a new database");
    }
    log.info("Getting input files");
    const std::vector<InputFastx> inputs = in.file_list ? read_rfile(*in.file_list) : read_input_fastas(in.seq_files);
    log.info("Parsed " + std::to_string(inputs.size()) + " samples in input list");
    MultiSketch db_metadata = MultiSketch::load_metadata(db_name);   // `?` in the reference: Error, exit 1
    {   // append_compatibility, multisketch.rs:229-244: before anything is sketched
        std::vector<std::string> duplicates;
        for (const auto &input : inputs) {
            if (db_metadata.has_sample(input.first)) duplicates.push_back(input.first);
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
    seq.concat_fasta = concat_fasta;
    check_concat_fasta(seq);
    log.info("Running sketching: sketch_size:" + std::to_string(db_metadata.sketch_size) + " threads:" + std::to_string(in.threads));
    MultiSketch fresh = sketch_inputs(log, in, *output, inputs, db_metadata.kmer_lengths(), db_metadata.sketch_size, seq);
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

}  // namespace skl_cli
