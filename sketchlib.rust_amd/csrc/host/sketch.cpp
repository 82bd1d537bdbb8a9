#include "sketch.hpp"
#include "aahash.hpp"
#include "inverted.hpp"
#include "read_filter.hpp"

#include <zlib.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstring>
#include <fstream>
#include <memory>
#include <mutex>
#include <string_view>
#include <stdexcept>
#include <thread>

namespace skl_host {

namespace {

using skl::srol;   // the split rotation ntHash rolls with (nthash_iterator.rs:368-370) and its inverse: nthash.hpp
using skl::sror;
// src/hashing/nthash_tables.rs:4-16, as tables for the loops below
const uint64_t HASH_LOOKUP[4] = {skl::hash_fwd(0), skl::hash_fwd(1), skl::hash_fwd(2), skl::hash_fwd(3)};
const uint64_t RC_HASH_LOOKUP[4] = {skl::hash_rc(0), skl::hash_rc(1), skl::hash_rc(2), skl::hash_rc(3)};

inline bool valid_base(uint8_t b)
{
    b |= 0x20;
    return b == 'a' || b == 'c' || b == 'g' || b == 't' || b == 'u';  // hashing/mod.rs:93-97
}
inline uint8_t encode_base(uint8_t b) { return (b >> 1) & 0x3; }  // hashing/mod.rs:82-85

}  // namespace

std::string read_maybe_gz(const std::string &path)
{
    gzFile f = gzopen(path.c_str(), "rb");  // transparently reads plain files too
    if (!f) throw std::runtime_error("Invalid path/file: " + path);
    gzbuffer(f, 1 << 20);
    std::string data;
    {
        std::ifstream probe(path, std::ios::binary | std::ios::ate);
        if (probe) data.reserve((size_t)probe.tellg() * (gzdirect(f) ? 1 : 4) + 16);
    }
    std::vector<char> buf(1 << 20);
    int n;
    while ((n = gzread(f, buf.data(), (unsigned)buf.size())) > 0) data.append(buf.data(), (size_t)n);
    gzclose(f);
    if (n < 0) throw std::runtime_error("Invalid FASTA/Q record in " + path);
    return data;
}

void add_fasta(const std::string &path, Sequence &s)
{
    const std::string data = read_maybe_gz(path);
    if (!data.empty() && data[0] == '@') {
        throw std::runtime_error(path + ": FASTQ input (reads) is not supported by this build");
    }
    // byte classes: 0-3 = base code, 4 = line break (skipped), 5 = anything else inside a record
    // (an invalid base: recorded as a break)
    static const auto table = [] {
        std::array<uint8_t, 256> t;
        t.fill(5);
        t[(uint8_t)'\n'] = 4;
        t[(uint8_t)'\r'] = 4;
        for (int c = 0; c < 256; ++c) {
            if (valid_base((uint8_t)c)) t[c] = encode_base((uint8_t)c);
        }
        return t;
    }();
    const size_t n = data.size();
    const size_t base0 = s.codes.size();
    s.codes.resize(base0 + n);          // upper bound; trimmed below (one allocation, no per-base growth)
    uint8_t *out = s.codes.data() + base0;
    size_t n_out = 0;
    uint64_t counts[6] = {0, 0, 0, 0, 0, 0};
    size_t i = 0;
    bool in_record = false;
    while (i < n) {
        if (data[i] == '>') {
            if (in_record) s.offsets.push_back(base0 + n_out);  // record boundary
            in_record = true;
            const void *nl = std::memchr(data.data() + i, '\n', n - i);   // skip header line
            i = nl ? (size_t)((const char *)nl - data.data()) : n;
            continue;
        }
        if (!in_record) {
            ++i;
            continue;
        }
        // sequence bytes up to the next header
        const void *gt = std::memchr(data.data() + i, '>', n - i);
        const size_t end = gt ? (size_t)((const char *)gt - data.data()) : n;
        for (; i < end; ++i) {
            const uint8_t cls = table[(uint8_t)data[i]];
            if (cls < 4) {
                out[n_out++] = cls;
                ++counts[cls];
            } else if (cls == 5) {
                ++counts[5];
                s.offsets.push_back(base0 + n_out);
            }
        }
    }
    if (in_record) s.offsets.push_back(base0 + n_out);
    s.codes.resize(base0 + n_out);
    for (int b = 0; b < 4; ++b) s.acgt[b] += counts[b];
    s.non_acgt += counts[5];
}

namespace {

// needletail's format peek (nthash_iterator.rs:94-108): the first record of a file decides FASTA / FASTQ
bool first_record_is_fastq(const std::string &path)
{
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("Invalid path/file: " + path);
    char buf[4096];
    const int n = gzread(f, buf, sizeof buf);
    gzclose(f);
    for (int i = 0; i < n; ++i) {
        if (buf[i] == '\n' || buf[i] == '\r' || buf[i] == ' ' || buf[i] == '\t') continue;
        return buf[i] == '@';
    }
    return false;
}

// One FASTQ file into `s` (add_dna_seq, nthash_iterator.rs:205-251), four-line records: a base is kept
// iff valid_base(b) && q[i] >= min_qual on the RAW quality byte (no -33 offset); a rejected base counts
// as non-ACGT and pushes an offset, and so does every record end.  Positions continue from
// s.codes.size().
void add_fastq(const std::string &path, uint8_t min_qual, Sequence &s)
{
    const std::string data = read_maybe_gz(path);
    const size_t n = data.size();
    size_t i = 0;
    auto next_line = [&](std::string_view &out) -> bool {
        if (i >= n) return false;
        const void *nl = std::memchr(data.data() + i, '\n', n - i);
        const size_t e = nl ? (size_t)((const char *)nl - data.data()) : n;
        out = std::string_view(data.data() + i, e - i);
        if (!out.empty() && out.back() == '\r') out.remove_suffix(1);
        i = e < n ? e + 1 : n;
        return true;
    };
    auto bad = [&](const char *what) {
        return std::runtime_error("Invalid FASTA/Q record in " + path + ": " + what);
    };
    s.codes.reserve(s.codes.size() + n / 2);
    uint64_t counts[5] = {0, 0, 0, 0, 0};
    std::string_view head, seq, plus, qual;
    for (;;) {
        bool more;
        while ((more = next_line(head)) && head.empty()) {
        }
        if (!more) break;
        if (head[0] != '@') throw bad("a record must start with '@'");
        if (!next_line(seq) || !next_line(plus) || !next_line(qual)) throw bad("truncated record");
        if (plus.empty() || plus[0] != '+') throw bad("the third line of a record must start with '+'");
        if (qual.size() != seq.size()) throw bad("quality and sequence lengths differ");
        for (size_t b = 0; b < seq.size(); ++b) {
            const uint8_t base = (uint8_t)seq[b];
            if (valid_base(base) && (uint8_t)qual[b] >= min_qual) {
                const uint8_t code = encode_base(base);
                s.codes.push_back(code);
                ++counts[code];
            } else {
                ++counts[4];
                s.offsets.push_back(s.codes.size());
            }
        }
        s.offsets.push_back(s.codes.size());
    }
    for (int b = 0; b < 4; ++b) s.acgt[b] += counts[b];
    s.non_acgt += counts[4];
}

}  // namespace

void load_sample(const InputFastx &input, uint8_t min_qual, Sequence &s)
{
    const auto &files = input.second;
    if (files.empty() || !first_record_is_fastq(files[0])) {
        for (const auto &file : files) add_fasta(file, s);
        return;
    }
    if (files.size() > 2) throw std::runtime_error("Input files are reads, but there are more than two input files");
    s.reads = true;
    for (const auto &file : files) {
        // each file's last partial byte is left-aligned (nthash_iterator.rs:245-250): the next file starts on a whole
        // byte, 0-3 bases of code 0 after the last base of this one
        s.codes.resize((s.codes.size() + 3) / 4 * 4, 0);
        if (first_record_is_fastq(file)) add_fastq(file, min_qual, s);
        else add_fasta(file, s);
    }
    // the iterator stops at seq_len() = the number of valid bases (nthash_iterator.rs:74-76), in the padded
    // coordinates: what lies past it is never hashed, and breaks past it cut no window
    uint64_t total = 0;
    for (uint64_t c : s.acgt) total += c;
    s.codes.resize((size_t)total);
    while (!s.offsets.empty() && s.offsets.back() > total) s.offsets.pop_back();
}

namespace {

// Every valid k-mer's sign (hash % SIGN_MOD), in the order NtHashIterator yields them
// (nthash_iterator.rs:470-520): f(start, sign) for each window start in ascending order; canonical
// hash = min(forward, reverse-complement) when rc (nthash_iterator.rs:62-68).  A window [s, s+k) is
// valid iff s + k <= codes.size() and no offset o satisfies s < o < s+k (next_iterator, :325-346).
// Returns whether there was any valid window.
template <class F>
bool for_each_window(const Sequence &seq, size_t k, bool rc, F &&f)
{
    const size_t n = seq.codes.size();
    // srol^(k-1) of each seed: the weight of the oldest base (forward) / newest base (reverse)
    uint64_t top_f[4], top_r[4];
    skl::nthash_top_tables(k, top_f, top_r);
    size_t off_idx = 0;
    size_t start = 0;
    bool any = false;
    while (start + k <= n) {
        // skip windows containing an offset strictly inside
        while (off_idx < seq.offsets.size() && seq.offsets[off_idx] <= start) ++off_idx;
        if (off_idx < seq.offsets.size() && seq.offsets[off_idx] < start + k) {
            start = seq.offsets[off_idx];  // restart right after the N / boundary
            continue;
        }
        // run of valid windows: from `start` until the next offset
        const size_t run_end = off_idx < seq.offsets.size() ? seq.offsets[off_idx] : n;  // exclusive base bound
        uint64_t fh = 0, rh = 0;
        for (size_t i = 0; i < k; ++i) {
            fh = srol(fh) ^ HASH_LOOKUP[seq.codes[start + i]];
        }
        if (rc) {
            for (size_t i = k; i-- > 0;) rh = srol(rh) ^ RC_HASH_LOOKUP[seq.codes[start + i]];
        }
        size_t s = start;
        for (;;) {
            const uint64_t h = rc ? std::min(fh, rh) : fh;
            f(s, h % SIGN_MOD);
            any = true;
            if (s + k >= run_end) break;
            const uint8_t old_b = seq.codes[s], new_b = seq.codes[s + k];
            fh = srol(fh ^ top_f[old_b]) ^ HASH_LOOKUP[new_b];
            if (rc) rh = sror(rh ^ RC_HASH_LOOKUP[old_b]) ^ top_r[new_b];
            ++s;
        }
        start = run_end;
    }
    return any;
}

// Bin minima of the signs of every valid k-mer (get_signs, sketch/mod.rs:132-153).
void bin_minima(const Sequence &seq, size_t k, bool rc, std::vector<uint64_t> &signs)
{
    const uint64_t num_bins = signs.size();
    const uint64_t bin_size = skl::bin_size_of(num_bins);
    if (seq.codes.size() < k) throw std::runtime_error("K-mer larger than smallest valid sequence");
    const bool any = for_each_window(seq, k, rc, [&](size_t, uint64_t sign) {
        uint64_t &slot = signs[sign / bin_size];
        if (sign < slot) slot = sign;
    });
    if (!any) throw std::runtime_error("K-mer larger than smallest valid sequence");
}

// sketch/mod.rs:225-231
inline uint64_t universal_hash(uint64_t s, uint64_t t)
{
    const uint64_t x = s * 1009ull + t * (1000ull * 1000ull + 3ull);
    return (x * 48271ull + 11ull) % ((1ull << 31) - 1);
}

}  // namespace

// densify_bin, sketch/mod.rs:237-258
bool densify_bin(std::vector<uint64_t> &signs)
{
    uint64_t maxval = 0;
    for (uint64_t s : signs) maxval = std::max(maxval, s);
    if (maxval != UINT64_MAX) return false;
    for (size_t i = 0; i < signs.size(); ++i) {
        size_t j = i;
        uint64_t attempts = 0;
        while (signs[j] == UINT64_MAX) {
            j = (size_t)(universal_hash(i, attempts) % signs.size());
            ++attempts;
        }
        signs[i] = signs[j];
    }
    return true;
}

// fill_usigs, sketch/mod.rs:215-223
void fill_usigs(uint64_t *usigs, const std::vector<uint64_t> &signs)
{
    for (size_t idx = 0; idx < signs.size(); ++idx) {
        const size_t leftshift = idx % 64;
        for (uint64_t p = 0; p < BBITS; ++p) {
            usigs[idx / 64 * BBITS + p] |= ((signs[idx] >> p) & 1ull) << leftshift;
        }
    }
}

std::vector<InputFastx> read_input_fastas(const std::vector<std::string> &seq_files)
{
    // the reference strips the directory when the extension is a known FASTA/FASTQ one
    static const char *exts[] = {".fa", ".fasta", ".fa.gz", ".fasta.gz", ".fastq", ".fastq.gz", ".fq", ".fq.gz"};
    std::vector<InputFastx> out;
    for (const auto &file : seq_files) {
        std::string name = file;
        bool known = false;
        for (const char *e : exts) {
            const size_t el = strlen(e);
            if (file.size() > el && file.compare(file.size() - el, el, e) == 0) known = true;
        }
        const size_t slash = file.rfind('/');
        if (known && slash != std::string::npos) name = file.substr(slash + 1);
        out.push_back({name, {file}});
    }
    return out;
}

std::vector<InputFastx> read_rfile(const std::string &file_list)
{
    std::ifstream f(file_list);
    if (!f) throw std::runtime_error("Unable to open file_list " + file_list);
    std::vector<InputFastx> out;
    std::string line;
    while (std::getline(f, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        std::vector<std::string> fields;
        size_t pos = 0;
        for (;;) {
            const size_t tab = line.find_first_of("\t ", pos);
            fields.push_back(line.substr(pos, tab == std::string::npos ? std::string::npos : tab - pos));
            if (tab == std::string::npos) break;
            pos = tab + 1;
        }
        if (fields.size() < 2) throw std::runtime_error("Unable to parse line in file_list: " + line);
        out.push_back({fields[0], std::vector<std::string>(fields.begin() + 1, fields.end())});
    }
    return out;
}

std::vector<size_t> parse_kmers(const std::vector<size_t> &k_vals, const std::vector<size_t> &k_seq)
{
    std::vector<size_t> kmers;
    if (!k_vals.empty()) {
        kmers = k_vals;
    } else if (k_seq.size() == 3 && k_seq[2] > 0) {
        for (size_t k = k_seq[0]; k <= k_seq[1]; k += k_seq[2]) kmers.push_back(k);
    } else {
        throw std::runtime_error("Must specify --k-vals or --k-seq");
    }
    std::sort(kmers.begin(), kmers.end());
    for (size_t k : kmers) {
        if (k < 3) throw std::runtime_error("K-mers must be >=3");
    }
    return kmers;
}

SketchResult sketch_sample(const InputFastx &input, const std::vector<size_t> &kmers, uint64_t sketch_size,
                           bool rc, uint16_t min_count, uint8_t min_qual)
{
    Sequence seq;
    load_sample(input, min_qual, seq);
    uint64_t total = 0;
    for (uint64_t c : seq.acgt) total += c;
    if (total == 0) throw std::runtime_error(input.first + " has no valid sequence");
    const uint64_t ss64 = (sketch_size + 63) / 64;  // num_bins, sketch/mod.rs:49-54
    const uint64_t num_bins = ss64 * 64;
    const uint64_t bin_size = skl::bin_size_of(num_bins);
    SketchResult out;
    out.usigs.assign((size_t)(ss64 * BBITS * kmers.size()), 0);
    bool densified = false;
    std::vector<uint64_t> first_signs;   // signs[0] per k, for a read set's length estimate
    std::unique_ptr<KmerFilter> filter;
    if (seq.reads) filter.reset(new KmerFilter(min_count));
    for (size_t ki = 0; ki < kmers.size(); ++ki) {
        std::vector<uint64_t> signs((size_t)num_bins, UINT64_MAX);
        if (filter) {   // every window through the count filter, in stream order (get_signs, sketch/mod.rs:132-153)
            filter->clear();
            const bool any = for_each_window(seq, kmers[ki], rc, [&](size_t, uint64_t sign) {
                offer_sign(signs.data(), bin_size, *filter, sign);
            });
            check_read_signs(any, signs, input.first, kmers[ki], min_count);
        } else {
            bin_minima(seq, kmers[ki], rc, signs);
        }
        densified |= densify_bin(signs);
        first_signs.push_back(signs[0]);
        fill_usigs(out.usigs.data() + ki * ss64 * BBITS, signs);
    }
    out.meta.name = input.first;
    out.meta.rc = rc;
    out.meta.reads = seq.reads;
    out.meta.seq_length = seq.reads ? reads_seq_length(first_signs) : total;
    out.meta.densified = densified;
    for (int b = 0; b < 4; ++b) out.meta.acgt[b] = seq.acgt[b];
    out.meta.non_acgt = seq.non_acgt;
    return out;
}

void check_read_signs(bool any_window, const std::vector<uint64_t> &signs, const std::string &name, size_t k,
                      uint16_t min_count)
{
    if (!any_window) throw std::runtime_error("K-mer larger than smallest valid sequence");
    // (the reference's densify_bin never returns on an all-empty sketch)
    if (std::all_of(signs.begin(), signs.end(), [](uint64_t v) { return v == UINT64_MAX; })) {
        throw std::runtime_error("no k-mer of " + name + " reached --min-count " + std::to_string(min_count) + " at k=" +
                                 std::to_string(k) + ": every bin is empty");
    }
}

std::vector<uint16_t> sketch_sample_inverted(const InputFastx &input, size_t k, uint64_t sketch_size, bool rc,
                                             uint16_t min_count, uint8_t min_qual)
{
    Sequence seq;
    load_sample(input, min_qual, seq);
    uint64_t total = 0;
    for (uint64_t c : seq.acgt) total += c;
    if (total == 0) throw std::runtime_error(input.first + " has no valid sequence");
    std::vector<uint64_t> signs((size_t)sketch_size, UINT64_MAX);   // exactly sketch_size bins, inverted.rs:352-357
    if (seq.reads) {   // every window through the count filter, in stream order (inverted.rs:348-361, as sketch_sample)
        const uint64_t bin_size = skl::bin_size_of(sketch_size);
        KmerFilter filter(min_count);
        const bool any = for_each_window(seq, k, rc, [&](size_t, uint64_t sign) { offer_sign(signs.data(), bin_size, filter, sign); });
        check_read_signs(any, signs, input.first, k, min_count);
    } else {
        bin_minima(seq, k, rc, signs);
    }
    densify_bin(signs);
    std::vector<uint16_t> out(signs.size());
    for (size_t i = 0; i < signs.size(); ++i) out[i] = (uint16_t)signs[i];   // `*h as u16`, inverted.rs:380
    return out;
}

MultiSketch sketch_files(const std::string &output_prefix, const std::vector<InputFastx> &inputs,
                         const std::vector<size_t> &kmers, uint64_t sketch_size, bool rc, size_t threads,
                         uint16_t min_count, uint8_t min_qual, const SeqType &st)
{
    const uint64_t ss64 = (sketch_size + 63) / 64;
    const size_t sample_words = (size_t)(ss64 * BBITS * kmers.size());
    std::vector<std::vector<SketchResult>> results(inputs.size());   // (amino acids with --concat-fasta: a sample per record)
    std::atomic<size_t> next{0};
    std::string error;
    // (fewer inputs than threads -- one FASTA of many proteins under --concat-fasta: the rest go to the samples inside an input)
    const size_t inner_threads = std::max<size_t>(1, threads / std::max<size_t>(1, inputs.size()));
    auto worker = [&]() {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= inputs.size()) break;
            try {
                if (st.aa) {
                    results[i] = sketch_input_aa(inputs[i], kmers, sketch_size, rc, st, inner_threads);
                } else {
                    results[i].resize(1);
                    results[i][0] = sketch_sample(inputs[i], kmers, sketch_size, rc, min_count, min_qual);
                }
            } catch (const std::exception &e) {
                results[i].clear();
                static std::mutex m;
                std::lock_guard<std::mutex> lock(m);
                if (error.empty()) error = e.what();
            }
        }
    };
    threads = std::max<size_t>(1, std::min(threads, inputs.size()));
    std::vector<std::thread> pool;
    for (size_t t = 1; t < threads; ++t) pool.emplace_back(worker);
    worker();
    for (auto &t : pool) t.join();
    if (!error.empty()) throw std::runtime_error(error);

    size_t n_samples = 0;
    for (const auto &r : results) n_samples += r.size();
    std::vector<uint64_t> bins(sample_words * n_samples);
    std::vector<SketchMeta> meta;
    for (auto &per_input : results) {
        for (auto &r : per_input) {
            std::copy(r.usigs.begin(), r.usigs.end(), bins.begin() + meta.size() * sample_words);
            r.meta.index = meta.size();
            meta.push_back(r.meta);
        }
    }
    MultiSketch::write_sketch_data(output_prefix, bins.data(), bins.size());
    MultiSketch m(std::move(meta), ss64 * 64, kmers);
    m.set_hash_type(st.hash_type());
    m.save_metadata(output_prefix);
    m.set_bins(std::move(bins));
    return m;
}

}  // namespace skl_host
