// aahash.hpp -- amino-acid sketching on the CPU: FASTA -> residues with separators -> forward aaHash of every window of k valid
// residues -> `% SIGN_MOD` -> bin minima -> the densify / transpose / writers of sketch.hpp.  Restates the reference's
// AaHashIterator (src/hashing/aahash_iterator.rs), the HashType::AA parts of src/hashing/mod.rs and src/sketch/mod.rs:283-391,
// and `sketch --seq-type aa` of src/lib.rs:242-302.  The seeds are the published aaHash constants
// (doi:10.1093/bioadv/vbad162); the roll values are derived from them at start-up (aa_roll_values), not tabulated.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "sketch.hpp"

namespace skl_host {

// A residue as the sketcher stores it: 0 = separator (an invalid residue or a record end; the reference's SEQSEP), 1..20 = the
// letters ACDEFGHIKLMNPQRSTVWY in that order, either case (valid_aa, aahash_iterator.rs:11-13).  The grouping level is not in
// the code: it is in the seed table the code indexes.
constexpr int AA_CODES = 21;
uint8_t aa_code(uint8_t byte);
// seed of each residue code at level 1 / 2 / 3 ([0] = 0: a separator adds nothing to a hash)
const uint64_t *aa_seeds(int level);
// srol^k of each seed: what a residue contributes when it leaves a window of k (aa_roll_table, aahash_tables.rs:18-35; its split
// 31 / 33-bit tables indexed by k % 31 | k % 33 hold exactly these values)
void aa_roll_values(int level, size_t k, uint64_t out[AA_CODES]);

// AaHashIterator::new (aahash_iterator.rs:84-124): one entry per sample -- the whole list of files, or with concat_fasta every
// record (named <name>_<n>, n from 1 across the files).  Without concat_fasta a separator follows every record.
struct AaSample {
    std::string name;
    std::vector<uint8_t> codes;   // stored length = seq_length of the metadata, separators included
    uint64_t invalid = 0;         // invalid residues (non_acgt of the metadata)
};
std::vector<AaSample> load_aa_samples(const InputFastx &input, bool concat_fasta);

// Bin minima of the signs of every window the reference's iterator yields at k (next / new_iterator, aahash_iterator.rs:138-210):
// a window is hashed iff its k residues are valid, and -- the iterator seeds only where start < len - k -- the window at exactly
// len - k only when it is reached by rolling, i.e. when the residue before it is valid too (`end_rule`; a sequence that ends in
// a separator never shows it).  signs[num_bins] is lowered in place.  Returns whether any window was hashed.
bool aa_bin_minima(const uint8_t *codes, size_t len, size_t k, int level, bool end_rule, uint64_t *signs, uint64_t num_bins);

// Sketch::new for every sample of one input (sketch_files, sketch/mod.rs:330-375), the samples on `threads` threads
std::vector<SketchResult> sketch_input_aa(const InputFastx &input, const std::vector<size_t> &kmers, uint64_t sketch_size,
                                          bool rc, const SeqType &st, size_t threads = 1);

}  // namespace skl_host
