// dbmaint.hpp -- database maintenance on disk: the reference's `merge`, `delete` and `info` commands and the file side of
// `append` (src/lib.rs:454-483, 793-947; src/sketch/multisketch.rs:222-363; src/utils.rs:17-40).  File operations only:
// nothing here touches a device.  Where the reference panics these throw Panic (exit code 101 in the CLI); where it returns
// an anyhow error they throw std::runtime_error ("Error: ..." and exit code 1).
#pragma once

#include <iosfwd>
#include <string>
#include <vector>

#include "multisketch.hpp"

namespace skl_host {

// Rust's `{:?}` of a str / of a Vec of them: "name", ["a", "b"]
std::string rust_debug(const std::string &s);
std::string rust_debug(const std::vector<std::string> &v);
// Rust's `{:?}` of a HashType as MultiSketch / Inverted hold it here: DNA, AA(Level1)
std::string hash_type_debug(const std::string &hash_type);

// bytes [offset, offset + bytes) of `src` appended to the open file `out_fd`, through a bounded buffer
void copy_file_range_buffered(int src_fd, int out_fd, uint64_t offset, uint64_t bytes, const std::string &what);
// all of src_path at the end of dst_path (truncate: dst_path is created / emptied first)
void append_file(const std::string &src_path, const std::string &dst_path, bool truncate);

// `merge <db1> <db2> -o <out>`: <out>.skm = db1's metadata with db2's samples after them, <out>.skd = db1's bytes, then db2's
void db_merge(const std::string &db1, const std::string &db2, const std::string &output);
// `delete <db> <samples.txt> <out>`: <out>.skm / .skd without the samples listed, blocks in file order, indices renumbered
void db_delete(const std::string &db, const std::string &samples_file, const std::string &output);
// `info <file> [--sample-info]`: the reference's Debug / Display text of a .skm (or .skd / bare prefix) or a .ski
void db_info(const std::string &file, bool sample_info, std::ostream &os);

}  // namespace skl_host
