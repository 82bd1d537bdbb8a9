// sketch.hpp -- CPU assembly sketcher: gz/plain FASTA -> canonical ntHash -> bin minima ->
// densify -> 14-plane transpose, i.e. the producer of the `.skm/.skd` files the distance
// path consumes.  Mirrors the reference's `sketch` command for DNA
// assemblies and read sets (src/sketch/mod.rs:74-258,283-391, src/hashing/nthash_iterator.rs; reads: FASTQ + k-mer count
// filter, read_filter.hpp).  Amino-acid sequences (`--seq-type aa`, SeqType below) take the aaHash path of aahash.hpp and share
// the bin minimum, densification, transpose and writers here; the structure alphabet (`pdb`) is not part of this build.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../nthash.hpp"
#include "multisketch.hpp"

namespace skl_host {

using skl::SIGN_MOD;   // src/sketch/mod.rs:36 (nthash.hpp)

// (sample name, sequence files), one entry per sample (src/io.rs:20-40, rfile parsing)
using InputFastx = std::pair<std::string, std::vector<std::string>>;

// What is hashed (HashType, src/hashing/mod.rs:29-39; `sketch --seq-type / --level / --concat-fasta`, src/lib.rs:242-302)
struct SeqType {
    bool aa = false;             // amino acids (aaHash, forward only) instead of DNA (canonical ntHash)
    int level = 1;               // aaHash grouping level 1 / 2 / 3 (aa only)
    bool concat_fasta = false;   // every FASTA record a sample of its own, named <name>_<n> (aa only)
    std::string hash_type() const { return aa ? "AA:Level" + std::to_string(level) : "DNA"; }   // as MultiSketch holds it
};

std::string read_maybe_gz(const std::string &path);   // a whole gz or plain file

std::vector<InputFastx> read_input_fastas(const std::vector<std::string> &seq_files);  // io.rs:20-40
std::vector<InputFastx> read_rfile(const std::string &file_list);                      // name<TAB>file[<TAB>file]
std::vector<size_t> parse_kmers(const std::vector<size_t> &k_vals, const std::vector<size_t> &k_seq);  // io.rs:140-159

// NtHashIterator::add_dna_seq (nthash_iterator.rs:205-251): valid bases as 2-bit codes, plus
// the valid-base coordinates of every N and record end.
struct Sequence {
    std::vector<uint8_t> codes;
    std::vector<size_t> offsets;
    uint64_t acgt[4] = {0, 0, 0, 0};
    uint64_t non_acgt = 0;
    bool reads = false;   // FASTQ input: codes / offsets in the padded two-file layout of load_sample
};
void add_fasta(const std::string &path, Sequence &s);
// A sample's files (NtHashIterator::new, nthash_iterator.rs:94-141).  FASTA: add_fasta per file (concatenated
// without padding).  Reads (the first record of the first file is FASTQ; more than two files is an error): bases
// kept iff valid and quality byte >= min_qual, each file starting on a multiple of 4 positions (the 0-3 bases
// between are code 0), codes cut at the number of valid bases and offsets past it dropped.
void load_sample(const InputFastx &input, uint8_t min_qual, Sequence &s);
// A read set's k-mer length gave no window at all, or no k-mer passed the count filter: the error to raise.
void check_read_signs(bool any_window, const std::vector<uint64_t> &signs, const std::string &name, size_t k,
                      uint16_t min_count);
bool densify_bin(std::vector<uint64_t> &signs);                     // sketch/mod.rs:237-258
void fill_usigs(uint64_t *usigs, const std::vector<uint64_t> &signs);  // sketch/mod.rs:215-223

struct SketchResult {
    SketchMeta meta;
    std::vector<uint64_t> usigs;  // [k][chunk][plane]
};

// Sketch::new (src/sketch/mod.rs:74-129) for one sample.  min_count / min_qual apply to read sets only
// (defaults 5 / 20, cli.rs:12-15).
SketchResult sketch_sample(const InputFastx &input, const std::vector<size_t> &kmers, uint64_t sketch_size,
                           bool rc, uint16_t min_count = 5, uint8_t min_qual = 20);

// sketch_files (src/sketch/mod.rs:283-391): writes <output_prefix>.skd and .skm; samples
// keep their input order (what the reference yields with --threads 1).
MultiSketch sketch_files(const std::string &output_prefix, const std::vector<InputFastx> &inputs,
                         const std::vector<size_t> &kmers, uint64_t sketch_size, bool rc, size_t threads,
                         uint16_t min_count = 5, uint8_t min_qual = 20, const SeqType &st = SeqType());

class Device;
// The same with the hashing / bin-minimum loop on the GPU (SURVEY 8f row f4,
// skl_sketch_signs): FASTA parsing, densification, transpose and the file writers stay on the
// host.  Amino acids: skl_sketch_signs_aa.  Output files are byte-identical to sketch_files'.
MultiSketch sketch_files_gpu(Device &dev, const std::string &output_prefix, const std::vector<InputFastx> &inputs,
                             const std::vector<size_t> &kmers, uint64_t sketch_size, bool rc, size_t threads,
                             uint16_t min_count = 5, uint8_t min_qual = 20, const SeqType &st = SeqType());

}  // namespace skl_host
