// pairs_file.hpp -- the list of sample pairs `sketchlib dist --pairs <FILE>` takes (no reference counterpart).
//
// One pair per line, `name1<TAB>name2`; further tab-separated columns are ignored, so the listing of an earlier
// `dist --knn` run is a valid pairs file.  Blank lines are skipped; a line end of CR LF is taken as LF.  name1 is looked
// up among `first_names`, name2 among `second_names` (the same list for ref-vs-ref; reference and query samples
// otherwise); of samples that share a name the first one is meant.  Anything else -- a line without a second column, an
// empty name, a name that is not in its list -- is an error naming the file, the line and, where there is one, the sample.
// Plain host code without a device dependency: tests/native/pairs_file_check.cpp builds it as it is.
#pragma once

#include <cstdint>
#include <iosfwd>
#include <string>
#include <vector>

namespace skl_host {

struct PairsFile {
    std::vector<uint32_t> first, second;   // sample indices, one entry per non-blank line, in file order
    size_t size() const { return first.size(); }
};

// `label`: what the error messages call the input (the file's path); `second_what`: "reference" or "query"
PairsFile parse_pairs(std::istream &in, const std::string &label, const std::vector<std::string> &first_names,
                      const std::vector<std::string> &second_names, const char *second_what = "reference");
// throws std::runtime_error("Unable to open <path>") when the file cannot be read
PairsFile read_pairs_file(const std::string &path, const std::vector<std::string> &first_names,
                          const std::vector<std::string> &second_names, const char *second_what = "reference");

}  // namespace skl_host
