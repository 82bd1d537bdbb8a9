#include "dbmaint.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <charconv>
#include <cstring>
#include <fstream>
#include <ostream>
#include <stdexcept>

#include "distances.hpp"   // Panic
#include "inverted.hpp"
#include "io.hpp"

namespace skl_host {

namespace {

constexpr size_t COPY_BUFFER_BYTES = 8u << 20;   // what a copy holds in memory, whatever the database's size

struct Fd {
    int fd = -1;
    explicit Fd(int f) : fd(f) {}
    Fd(const Fd &) = delete;
    Fd &operator=(const Fd &) = delete;
    ~Fd() { if (fd >= 0) ::close(fd); }
};

int open_read(const std::string &path)
{
    const int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd < 0) throw std::runtime_error("cannot open " + path + ": " + std::strerror(errno));
    return fd;
}

int open_write(const std::string &path, bool truncate)
{
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_CLOEXEC | (truncate ? O_TRUNC : O_APPEND), 0644);
    if (fd < 0) throw std::runtime_error("cannot create " + path + ": " + std::strerror(errno));
    return fd;
}

uint64_t file_size(int fd, const std::string &path)
{
    struct stat st;
    if (::fstat(fd, &st) != 0) throw std::runtime_error("cannot stat " + path);
    return (uint64_t)st.st_size;
}

MultiSketch load_or_panic(const std::string &prefix)
{
    try {
        return MultiSketch::load_metadata(prefix);
    } catch (const std::exception &) {
        throw Panic("Could not read sketch metadata from " + prefix + ".skm");
    }
}

// Rust's `{}` of an f64: the shortest digits that read back the same, never an exponent, 4.0 as "4"
std::string rust_display(double v)
{
    char buf[512];
    const auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}

}  // namespace

std::string rust_debug(const std::string &s)
{
    std::string o = "\"";
    for (const char c : s) {
        switch (c) {
        case '"': o += "\\\""; break;
        case '\\': o += "\\\\"; break;
        case '\n': o += "\\n"; break;
        case '\r': o += "\\r"; break;
        case '\t': o += "\\t"; break;
        default: o += c;
        }
    }
    return o + "\"";
}

std::string rust_debug(const std::vector<std::string> &v)
{
    std::string o = "[";
    for (size_t i = 0; i < v.size(); ++i) o += (i ? ", " : "") + rust_debug(v[i]);
    return o + "]";
}

std::string hash_type_debug(const std::string &h)
{
    const size_t colon = h.find(':');   // MultiSketch holds AA:Level1, Inverted AA(Level1)
    return colon == std::string::npos ? h : h.substr(0, colon) + "(" + h.substr(colon + 1) + ")";
}

void copy_file_range_buffered(int src_fd, int out_fd, uint64_t offset, uint64_t bytes, const std::string &what)
{
    std::vector<char> buf((size_t)std::min<uint64_t>(std::max<uint64_t>(bytes, 1), COPY_BUFFER_BYTES));
    while (bytes) {
        const size_t want = (size_t)std::min<uint64_t>(bytes, buf.size());
        const ssize_t got = ::pread(src_fd, buf.data(), want, (off_t)offset);
        if (got <= 0) throw std::runtime_error(what + " is shorter than its metadata says");
        for (ssize_t done = 0; done < got;) {
            const ssize_t w = ::write(out_fd, buf.data() + done, (size_t)(got - done));
            if (w <= 0) throw std::runtime_error("error writing the sketch data: " + std::string(std::strerror(errno)));
            done += w;
        }
        offset += (uint64_t)got;
        bytes -= (uint64_t)got;
    }
}

void append_file(const std::string &src_path, const std::string &dst_path, bool truncate)
{
    const Fd src(open_read(src_path));
    const Fd dst(open_write(dst_path, truncate));
    copy_file_range_buffered(src.fd, dst.fd, 0, file_size(src.fd, src_path), src_path);
}

void db_merge(const std::string &db1, const std::string &db2, const std::string &output)
{
    const std::string name1 = strip_sketch_extension(db1), name2 = strip_sketch_extension(db2);
    if (output == name1 || output == name2) throw std::runtime_error("the output " + output + " is one of the inputs");
    MultiSketch sketches1 = load_or_panic(name1);
    const MultiSketch sketches2 = load_or_panic(name2);
    if (!sketches1.is_compatible_with(sketches2)) throw Panic("Databases are not compatible for merging.");
    try {
        sketches1.merge_sketches(sketches2);
    } catch (const std::exception &e) {
        throw Panic(e.what());
    }
    try {
        sketches1.save_metadata(output);
    } catch (const std::exception &) {
        throw Panic("Couldn't save metadata to " + output);
    }
    // utils.rs:17-33: the two .skd streamed one after the other (an error here is the reference's `?`)
    append_file(name1 + ".skd", output + ".skd", true);
    append_file(name2 + ".skd", output + ".skd", false);
}

void db_delete(const std::string &db, const std::string &samples_file, const std::string &output)
{
    const std::string ref_db = strip_sketch_extension(db);
    std::vector<std::string> ids;   // BufReader::lines(): the final newline ends the last id, a blank line is the id ""
    {
        std::ifstream f(samples_file);
        if (!f) throw std::runtime_error("No such file or directory (os error 2)");
        std::string line;
        while (std::getline(f, line)) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            ids.push_back(line);
        }
    }
    if (output == ref_db) throw std::runtime_error("the output " + output + " is the input database");
    MultiSketch sketches = load_or_panic(ref_db);
    const size_t block_bytes = sketches.sample_stride() * sizeof(uint64_t);
    std::vector<std::string> missing;
    const std::vector<size_t> kept = sketches.remove_samples(ids, &missing);
    if (!missing.empty()) {
        throw std::runtime_error("The following samples have not been found in the database: " + rust_debug(missing));
    }
    const std::string in_path = ref_db + ".skd";
    const Fd src(open_read(in_path));
    sketches.save_metadata(output);
    const Fd dst(open_write(output + ".skd", true));
    for (size_t i = 0; i < kept.size();) {   // runs of blocks that follow each other in the file: one copy each
        size_t j = i + 1;
        while (j < kept.size() && kept[j] == kept[j - 1] + 1) ++j;
        copy_file_range_buffered(src.fd, dst.fd, (uint64_t)kept[i] * block_bytes, (uint64_t)(j - i) * block_bytes, in_path);
        i = j;
    }
}

void db_info(const std::string &file, bool sample_info, std::ostream &os)
{
    auto ends = [&](const char *e) { return file.size() >= 4 && file.compare(file.size() - 4, 4, e) == 0; };
    if (ends(".ski")) {
        const std::string prefix = file.substr(0, file.size() - 4);
        Inverted inv;
        try {
            inv = Inverted::load(prefix);
        } catch (const std::exception &e) {
            os << "Read error: " << e.what() << "\n";
            os.flush();
            throw Panic("Could not read inverted index from " + prefix + ".ski");
        }
        if (sample_info) {   // Display, inverted.rs:543-551
            os << "Name\n";
            for (const auto &name : inv.sample_names) os << name << "\n";
            os << "\n";
            return;
        }
        // Debug, inverted.rs:517-541
        if (inv.index.empty()) throw Panic("called `Option::unwrap()` on a `None` value");   // (max of no bins)
        size_t max = 0, min = (size_t)-1, sum = 0;
        for (const auto &bin : inv.index) {
            max = std::max(max, bin.size());
            min = std::min(min, bin.size());
            sum += bin.size();
        }
        os << "sketch_version=" << inv.sketch_version << "\nsequence_type=" << hash_type_debug(inv.hash_type)
           << "\nsketch_size=" << inv.index.size() << "\nn_samples=" << inv.sample_names.size() << "\nkmer=" << inv.kmer_size
           << "\nrc=" << (inv.rc ? "true" : "false") << "\ninverted=true\n"
           << "max_hashes_per_bin=" << max << "\nmin_hashes_per_bin=" << min
           << "\navg_hashes_per_bin=" << rust_display((double)sum / (double)inv.index.size()) << "\n";
        return;
    }
    const std::string prefix = ends(".skm") || ends(".skd") ? file.substr(0, file.size() - 4) : file;
    const MultiSketch m = load_or_panic(prefix);
    if (sample_info) {   // Display, multisketch.rs:365-373 over sketch/mod.rs:261-278 (note acgt[3] before acgt[2])
        os << "Name\tSequence length\tBase frequencies\tMissing/ambig bases\tFrom reads\tSingle strand\tDensified\n";
        for (const auto &s : m.metadata()) {
            os << s.name << "\t" << s.seq_length << "\t[" << s.acgt[0] << ", " << s.acgt[1] << ", " << s.acgt[3] << ", " << s.acgt[2]
               << "]\t" << s.non_acgt << "\t" << (s.reads ? "true" : "false") << "\t" << (!s.rc ? "true" : "false") << "\t"
               << (s.densified ? "true" : "false") << "\n";
        }
        os << "\n";
        return;
    }
    // Debug, multisketch.rs:351-363
    os << "sketch_version=" << m.version() << "\nsequence_type=" << hash_type_debug(m.hash_type()) << "\nsketch_size=" << m.sketch_size
       << "\nn_samples=" << m.metadata().size() << "\nkmers=[";
    for (size_t i = 0; i < m.kmer_lengths().size(); ++i) os << (i ? ", " : "") << m.kmer_lengths()[i];
    os << "]\ninverted=false\n";
}

}  // namespace skl_host
