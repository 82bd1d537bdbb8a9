#include "aahash.hpp"

#include "../aa_seeds.hpp"

#include <algorithm>
#include <array>
#include <atomic>
#include <cstring>
#include <stdexcept>
#include <thread>

namespace skl_host {

namespace {

using skl::srol;   // the split rotation (nthash.hpp)

const std::array<uint8_t, 256> &code_table()
{
    static const auto table = [] {
        std::array<uint8_t, 256> t;
        t.fill(0);
        const char *letters = "ACDEFGHIKLMNPQRSTVWY";
        for (int i = 0; i < 20; ++i) {
            t[(uint8_t)letters[i]] = (uint8_t)(i + 1);
            t[(uint8_t)(letters[i] | 0x20)] = (uint8_t)(i + 1);
        }
        return t;
    }();
    return table;
}

}  // namespace

uint8_t aa_code(uint8_t byte) { return code_table()[byte]; }

const uint64_t *aa_seeds(int level)
{
    const uint64_t *seeds = skl::aa_seed_table(level);
    if (!seeds) throw std::runtime_error("aaHash level must be 1, 2 or 3");
    return seeds;
}

void aa_roll_values(int level, size_t k, uint64_t out[AA_CODES]) { skl::aa_roll_table(aa_seeds(level), k, out); }

std::vector<AaSample> load_aa_samples(const InputFastx &input, bool concat_fasta)
{
    const auto &table = code_table();
    std::vector<AaSample> out;
    AaSample cur;
    size_t n_records = 0;
    auto name_of = [&](size_t n) { return concat_fasta ? input.first + "_" + std::to_string(n) : input.first; };
    for (const auto &file : input.second) {
        const std::string data = read_maybe_gz(file);
        const size_t n = data.size();
        size_t i = 0;
        while (i < n && (data[i] == '\n' || data[i] == '\r' || data[i] == ' ' || data[i] == '\t')) ++i;
        if (i < n && data[i] == '@') {
            throw std::runtime_error("Unexpected quality information with AA sequences in " + file +
                                     ". Correct sequence type set?");
        }
        bool in_record = false;
        auto end_record = [&] {
            ++n_records;
            if (concat_fasta) {
                cur.name = name_of(n_records);
                out.push_back(std::move(cur));
                cur = AaSample();
            } else {
                cur.codes.push_back(0);
            }
        };
        while (i < n) {   // line by line: a '>' line opens a record, every other byte of a record's lines but CR / LF is a residue
            const void *nl = std::memchr(data.data() + i, '\n', n - i);
            const size_t end = nl ? (size_t)((const char *)nl - data.data()) : n;
            if (data[i] == '>') {
                if (in_record) end_record();
                in_record = true;
            } else if (in_record) {
                for (size_t x = i; x < end; ++x) {
                    if (data[x] == '\r') continue;
                    const uint8_t c = table[(uint8_t)data[x]];
                    cur.invalid += c == 0;
                    cur.codes.push_back(c);
                }
            } else if (end > i && data[i] != '\r') {
                throw std::runtime_error("Invalid FASTA/Q record in " + file);
            }
            i = end < n ? end + 1 : n;
        }
        if (in_record) end_record();
    }
    if (!concat_fasta) {
        cur.name = name_of(0);
        out.push_back(std::move(cur));
    }
    return out;
}

bool aa_bin_minima(const uint8_t *codes, size_t len, size_t k, int level, bool end_rule, uint64_t *signs, uint64_t num_bins)
{
    if (k == 0 || len < k) return false;
    const uint64_t *seeds = aa_seeds(level);
    uint64_t roll[AA_CODES];
    aa_roll_values(level, k, roll);
    const uint64_t bin_size = skl::bin_size_of(num_bins);
    // A separator has seed 0 and roll value 0, so the hash rolled straight through one is still the XOR of srol^distance(seed)
    // over the window's valid residues: exact for every window of k valid residues, and nothing is re-seeded.
    uint64_t fh = 0;
    size_t run = 0;   // valid residues since the last separator
    bool any = false;
    for (size_t e = 0; e < len; ++e) {
        const uint8_t c = codes[e];
        fh = srol(fh) ^ seeds[c];
        if (e >= k) fh ^= roll[codes[e - k]];
        run = c ? run + 1 : 0;
        if (run < k) continue;
        // the window [e + 1 - k, e]; the last one only if the iterator rolled into it (the residue before it is valid)
        if (end_rule && e + 1 == len && run < k + 1) continue;
        const uint64_t sign = fh % SIGN_MOD;
        uint64_t &slot = signs[sign / bin_size];
        if (sign < slot) slot = sign;
        any = true;
    }
    return any;
}

std::vector<SketchResult> sketch_input_aa(const InputFastx &input, const std::vector<size_t> &kmers, uint64_t sketch_size,
                                          bool rc, const SeqType &st, size_t threads)
{
    const std::vector<AaSample> samples = load_aa_samples(input, st.concat_fasta);
    const uint64_t ss64 = (sketch_size + 63) / 64;
    const uint64_t num_bins = ss64 * 64;
    std::vector<SketchResult> out(samples.size());
    std::vector<std::string> error(samples.size());
    auto sketch_one = [&](size_t s) {
        const AaSample &a = samples[s];
        if (a.codes.empty()) {
            error[s] = a.name + " has no valid sequence";
            return;
        }
        SketchResult &r = out[s];
        r.usigs.assign((size_t)(ss64 * BBITS * kmers.size()), 0);
        bool densified = false;
        std::vector<uint64_t> signs;
        for (size_t ki = 0; ki < kmers.size(); ++ki) {
            signs.assign((size_t)num_bins, UINT64_MAX);
            if (!aa_bin_minima(a.codes.data(), a.codes.size(), kmers[ki], st.level, true, signs.data(), num_bins)) {
                error[s] = "K-mer larger than smallest valid sequence";
                return;
            }
            densified |= densify_bin(signs);
            fill_usigs(r.usigs.data() + ki * ss64 * BBITS, signs);
        }
        r.meta.name = a.name;
        r.meta.rc = rc;   // (the hash is forward only: the flag is stored, nothing else)
        r.meta.reads = false;
        r.meta.seq_length = a.codes.size();
        r.meta.densified = densified;
        r.meta.non_acgt = a.invalid;
    };
    // the samples of one input (--concat-fasta: a record each) on this input's share of the threads
    std::atomic<size_t> next{0};
    auto worker = [&] {
        for (size_t s; (s = next.fetch_add(1)) < samples.size();) sketch_one(s);
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < std::max<size_t>(1, std::min(threads, samples.size())); ++t) pool.emplace_back(worker);
    worker();
    for (auto &t : pool) t.join();
    for (const auto &e : error) {   // the first sample in input order that fails
        if (!e.empty()) throw std::runtime_error(e);
    }
    return out;
}

}  // namespace skl_host
