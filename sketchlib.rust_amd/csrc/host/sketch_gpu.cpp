// sketch_gpu.cpp -- `sketchlib sketch --gpu`: FASTA / FASTQ parsing on host threads; hashing, bin minima,
// densification and the 14-plane transpose on the device (skl_sketch_usigs_packed), whose words
// land in the `.skd` image as they come back; file writers on the host.  Read sets
// with a count filter (min_count >= 2) hash on the device too (skl_reads_survivors), in chunks of window
// starts, and the host replays the survivors through the filter and finishes their signs itself.
// `inverted build --gpu` / `inverted query --gpu` (sketch_inverted_gpu, at the end): the same parsing, packing and batches for
// an index's rows -- one k-mer length, exactly sketch_size bins, u16 -- through skl_sketch_bins_u16_packed, and read sets under
// a count filter through the survivors path above with skl_sketch_finish_u16 behind it.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <stdexcept>
#include <thread>

#include "../sketch_plan.hpp"
#include "aahash.hpp"
#include "distances.hpp"
#include "inverted.hpp"
#include "read_filter.hpp"
#include "sketch.hpp"
#include "sketchlib_dist.h"

namespace skl_host {

namespace {
template <class F>
void parallel_for(size_t n, size_t threads, F f)
{
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n) break;
            f(i);
        }
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < std::max<size_t>(1, std::min(threads, n)); ++t) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
}

// f(i) for every i < n on host threads; the message of what f(i) threw is kept per i ("": nothing)
template <class F>
std::vector<std::string> try_each(size_t n, size_t threads, F f)
{
    std::vector<std::string> error(n);
    parallel_for(n, threads, [&](size_t i) {
        try {
            f(i);
        } catch (const std::exception &e) {
            error[i] = e.what();
            if (error[i].empty()) error[i] = "unreadable input";
        }
    });
    return error;
}

// the first error in input order: what the CPU path reports on one thread
void raise_first(const std::vector<std::string> &error)
{
    for (const auto &e : error) {
        if (!e.empty()) throw std::runtime_error(e);
    }
}

uint64_t valid_bases(const Sequence &s) { return s.acgt[0] + s.acgt[1] + s.acgt[2] + s.acgt[3]; }

// 1. parse (threads): every input into seqs, every input's error kept
std::vector<std::string> parse_inputs(const std::vector<InputFastx> &inputs, uint8_t min_qual, size_t threads, std::vector<Sequence> &seqs)
{
    seqs.assign(inputs.size(), Sequence());
    return try_each(inputs.size(), threads, [&](size_t i) {
        load_sample(inputs[i], min_qual, seqs[i]);
        if (valid_bases(seqs[i]) == 0) throw std::runtime_error(inputs[i].first + " has no valid sequence");
    });
}

// The batches [b0, b1) of items 0 .. n - 1 that sketch_plan.hpp cut_before cuts under `caps` (none for n = 0).
template <class SizeOf>
std::vector<std::pair<size_t, size_t>> batches(size_t n, SizeOf size_of, const skl::CutCaps &caps)
{
    std::vector<std::pair<size_t, size_t>> out;
    const std::vector<size_t> cuts = skl::cut_before(n, size_of, caps);
    for (size_t b = 0; n && b + 1 < cuts.size(); ++b) out.push_back({cuts[b], cuts[b + 1]});
    return out;
}

// The samples seqs[idx[0 .. nb)] as the input of one library call: the bases at 2 bits each, 16 per word, every sample on a word
// boundary (skl_sketch_signs_packed) -- a quarter of the bytes to gather here and to send over PCIe -- packed on host threads.
struct PackedBatch {
    std::vector<uint64_t> code_begin, word_begin, offset_begin, offsets;
    std::unique_ptr<uint32_t[]> packed;   // not zero-filled
};
PackedBatch gather_and_pack(const std::vector<Sequence> &seqs, const size_t *idx, size_t nb, size_t threads)
{
    PackedBatch p;
    p.code_begin.assign(nb + 1, 0);
    p.word_begin.assign(nb + 1, 0);
    p.offset_begin.assign(nb + 1, 0);
    for (size_t i = 0; i < nb; ++i) {
        const Sequence &s = seqs[idx[i]];
        p.code_begin[i + 1] = p.code_begin[i] + s.codes.size();
        p.word_begin[i + 1] = p.word_begin[i] + (s.codes.size() + 15) / 16;
        p.offsets.insert(p.offsets.end(), s.offsets.begin(), s.offsets.end());
        p.offset_begin[i + 1] = p.offsets.size();
    }
    p.packed.reset(new uint32_t[std::max<uint64_t>(p.word_begin[nb], 1)]);
    parallel_for(nb, threads, [&](size_t i) {
        const std::vector<uint8_t> &c = seqs[idx[i]].codes;
        skl::pack_codes(c.data(), c.size(), p.packed.get() + p.word_begin[i]);
    });
    return p;
}

SketchMeta make_meta(const std::string &name, size_t at, bool rc, bool reads, uint64_t seq_length, bool densified, const uint64_t *acgt,
                     uint64_t non_acgt)
{
    SketchMeta m;
    m.name = name;
    m.rc = rc;
    m.reads = reads;
    m.seq_length = seq_length;
    m.densified = densified;
    for (int x = 0; acgt && x < 4; ++x) m.acgt[x] = acgt[x];
    m.non_acgt = non_acgt;
    m.index = at;
    return m;
}
// ... of a DNA sample, from the densified signs[0] of each of its k-mer lengths
SketchMeta dna_meta(const std::string &name, size_t at, const Sequence &s, bool rc, bool densified, const std::vector<uint64_t> &first_signs)
{
    return make_meta(name, at, rc, s.reads, s.reads ? reads_seq_length(first_signs) : valid_bases(s), densified, s.acgt, s.non_acgt);
}

struct ReadsTiming {
    double gpu = 0, replay_wait = 0;
    uint64_t chunks = 0, window_starts = 0, survivors = 0;
};

// Bin minima after the count filter for the read sets `idx`.  Chunk j covers window starts
// [pos_j, pos_j + len_j) of every sample and stream; its survivors are taken under the bins the replay had reached
// before chunk j - 1's replay, so the kernel of chunk j runs while the host replays chunk j - 1.  The first chunk
// (every bin empty: everything survives) is short and the chunks double up to the cap (SKL_READS_CHUNK_WINDOWS).
// signs: [idx.size()][nk][num_bins]; any_window: [idx.size()][nk], whether the stream had a valid window at all.
void reads_signs_gpu(Device &dev, const std::vector<Sequence> &seqs, const std::vector<size_t> &idx,
                     const std::vector<size_t> &kmers, uint64_t num_bins, bool rc, uint16_t min_count, size_t threads,
                     std::vector<uint64_t> &signs, std::vector<char> &any_window, ReadsTiming &tm)
{
    const size_t nk = kmers.size(), streams = idx.size() * nk;
    const uint64_t bin_size = skl::bin_size_of(num_bins);
    const bool log_chunks = std::getenv("SKL_CLI_TIMING") != nullptr;
    uint64_t cap_len = 1ull << 20;
    if (const char *e = std::getenv("SKL_READS_CHUNK_WINDOWS")) cap_len = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    signs.assign(streams * num_bins, UINT64_MAX);
    any_window.assign(streams, 0);
    const PackedBatch in = gather_and_pack(seqs, idx.data(), idx.size(), threads);
    const std::vector<uint64_t> &code_begin = in.code_begin;
    uint64_t max_len = 0;
    for (size_t i = 0; i < idx.size(); ++i) max_len = std::max(max_len, code_begin[i + 1] - code_begin[i]);
    skl_reads *h = nullptr;
    if (skl_reads_create(dev.ctx(), in.packed.get(), code_begin.data(), in.offsets.data(), in.offset_begin.data(), idx.size(),
                         kmers.data(), nk, num_bins, rc ? 1 : 0, &h) != SKL_OK) {
        throw std::runtime_error(skl_last_error());
    }
    struct Release {
        skl_reads *h;
        ~Release() { skl_reads_destroy(h); }
    } release{h};
    std::vector<std::unique_ptr<KmerFilter>> filters(streams);
    for (auto &f : filters) f.reset(new KmerFilter(min_count));
    // survivors of one chunk: records [streams][capacity][2] and counts
    struct Chunk {
        std::vector<uint64_t> recs, counts;
        uint64_t capacity = 0;
        bool live = false;
    };
    auto replay = [&](Chunk &c) {
        if (!c.live) return;
        parallel_for(streams, threads, [&](size_t st) {
            const uint64_t m = c.counts[st];
            if (m == 0) return;
            any_window[st] = 1;   // (under all-empty bins every valid window survives)
            const uint64_t *rec = c.recs.data() + st * c.capacity * 2;
            std::vector<std::pair<uint64_t, uint64_t>> order(m);   // (window start, sign)
            for (uint64_t x = 0; x < m; ++x) order[x] = {rec[2 * x], rec[2 * x + 1]};
            std::sort(order.begin(), order.end());   // stream order: by window start
            uint64_t *bins = signs.data() + st * num_bins;
            for (const auto &o : order) offer_sign(bins, bin_size, *filters[st], o.second);
        });
        c.live = false;
    };
    const auto t0 = std::chrono::steady_clock::now();
    auto secs = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    Chunk chunk[2];
    uint64_t len = std::min<uint64_t>(cap_len, 1ull << 14), capacity = len;
    std::vector<uint64_t> win_begin(idx.size()), win_end(idx.size());
    size_t cur = 0;
    for (uint64_t pos = 0; pos < max_len; pos += len, len = std::min(cap_len, 2 * len)) {
        std::fill(win_begin.begin(), win_begin.end(), pos);
        std::fill(win_end.begin(), win_end.end(), pos + len);
        const std::vector<uint64_t> thresholds = signs;   // the replay's state before the previous chunk is replayed
        Chunk &prev = chunk[cur ^ 1], &c = chunk[cur];
        std::exception_ptr replay_error;
        std::thread replayer([&] {
            try {
                replay(prev);
            } catch (...) {
                replay_error = std::current_exception();
            }
        });
        const double g0 = secs();
        capacity = std::min(capacity, len);
        for (;;) {   // a stream with more survivors than room: the same call again with room for all of them
            c.capacity = capacity;
            c.recs.resize(streams * capacity * 2);
            c.counts.assign(streams, 0);
            const int rc_ = skl_reads_survivors(h, win_begin.data(), win_end.data(), thresholds.data(), capacity, c.recs.data(),
                                                c.counts.data());
            if (rc_ != SKL_OK) {
                replayer.join();
                throw std::runtime_error(skl_last_error());
            }
            const uint64_t most = *std::max_element(c.counts.begin(), c.counts.end());
            if (most <= capacity) break;
            capacity = most;
        }
        const double g1 = secs();
        replayer.join();
        if (replay_error) std::rethrow_exception(replay_error);
        tm.gpu += g1 - g0;
        tm.replay_wait += secs() - g1;
        c.live = true;
        uint64_t found = 0, most = 0, starts = 0;
        for (uint64_t x : c.counts) {
            found += x;
            most = std::max(most, x);
        }
        for (size_t i = 0; i < idx.size(); ++i) {
            const uint64_t n_i = code_begin[i + 1] - code_begin[i];
            starts += pos < n_i ? std::min(len, n_i - pos) * nk : 0;
        }
        if (log_chunks) {
            std::fprintf(stderr, "READS chunk %llu: window starts [%llu, %llu) x %zu streams, survivors %llu of %llu (%.3g)\n",
                         (unsigned long long)tm.chunks, (unsigned long long)pos, (unsigned long long)(pos + len), streams,
                         (unsigned long long)found, (unsigned long long)starts, starts ? (double)found / (double)starts : 0.0);
        }
        tm.chunks += 1;
        tm.window_starts += starts;
        tm.survivors += found;
        capacity = std::max<uint64_t>(4096, 2 * most);   // next chunk's first guess
        cur ^= 1;
    }
    const double r0 = secs();
    replay(chunk[cur ^ 1]);
    tm.replay_wait += secs() - r0;
}
}  // namespace

namespace {
// `sketch --gpu --seq-type aa`: protein FASTA parsed into residue codes on host threads (load_aa_samples), aaHash and bin
// minima on the device and densify / transpose behind them (skl_sketch_usigs_aa, §4.7): the finished words
// come back straight into the `.skd` image, 1 792 B per protein and k-mer length at 1 024 bins.  One call takes samples up to
// 1 Gi residues and 1 GiB of signs ON THE DEVICE -- at 1 024 bins and one k-mer length a protein's signs are 8 KiB, so a
// million proteins take eight calls -- and the library cuts a call into device batches of 256 MiB of signs.
MultiSketch sketch_files_gpu_aa(Device &dev, const std::string &output_prefix, const std::vector<InputFastx> &inputs,
                                const std::vector<size_t> &kmers, uint64_t sketch_size, bool rc, size_t threads, const SeqType &st)
{
    const size_t nk = kmers.size();
    const uint64_t ss64 = (sketch_size + 63) / 64;
    const uint64_t num_bins = ss64 * 64;
    const size_t sample_words = (size_t)(ss64 * BBITS * nk);
    const bool timing = std::getenv("SKL_CLI_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };

    std::vector<std::vector<AaSample>> per_input(inputs.size());
    raise_first(try_each(inputs.size(), threads, [&](size_t i) { per_input[i] = load_aa_samples(inputs[i], st.concat_fasta); }));
    std::vector<AaSample> samples;
    for (auto &v : per_input) {
        for (auto &a : v) samples.push_back(std::move(a));
    }
    per_input.clear();
    const size_t n = samples.size();
    const double t_parse = since();
    double t_gpu = 0, t_finish = 0;

    std::vector<uint64_t> bins(sample_words * n, 0);
    std::vector<SketchMeta> meta(n);
    std::vector<std::string> sample_error(n);
    std::vector<uint8_t> flags;
    for (const auto &[b0, b1] : batches(n, [&](size_t i) { return samples[i].codes.size(); }, skl::caps_aa_call(nk, num_bins))) {
        const size_t nb = b1 - b0;
        std::vector<uint64_t> res_begin(nb + 1, 0);
        for (size_t i = 0; i < nb; ++i) res_begin[i + 1] = res_begin[i] + samples[b0 + i].codes.size();
        std::unique_ptr<uint8_t[]> residues(new uint8_t[std::max<uint64_t>(res_begin[nb], 1)]);
        parallel_for(nb, threads, [&](size_t i) {
            const auto &c = samples[b0 + i].codes;
            if (!c.empty()) memcpy(residues.get() + res_begin[i], c.data(), c.size());
        });
        flags.assign(nb * nk, 0);
        const double t0 = since();
        // the finished words of samples [b0, b1) are exactly their part of the `.skd` image
        if (skl_sketch_usigs_aa(dev.ctx(), residues.get(), res_begin.data(), nb, kmers.data(), nk, num_bins, st.level,
                                st.concat_fasta ? 1 : 0, bins.data() + b0 * sample_words, nullptr, flags.data()) != SKL_OK) {
            throw std::runtime_error(skl_last_error());
        }
        const double t1 = since();
        t_gpu += t1 - t0;
        for (size_t i = 0; i < nb; ++i) {
            const size_t at = b0 + i;
            const AaSample &a = samples[at];
            if (a.codes.empty()) {
                sample_error[at] = a.name + " has no valid sequence";
                continue;
            }
            bool densified = false, empty = false;
            for (size_t ki = 0; ki < nk; ++ki) {
                densified |= (flags[i * nk + ki] & SKL_FINISH_DENSIFIED) != 0;
                empty |= (flags[i * nk + ki] & SKL_FINISH_EMPTY) != 0;
            }
            if (empty) {
                sample_error[at] = "K-mer larger than smallest valid sequence";   // as the CPU path
                continue;
            }
            meta[at] = make_meta(a.name, at, rc, false, a.codes.size(), densified, nullptr, a.invalid);
        }
        for (size_t at = b0; at < b1; ++at) {   // the first sample in input order that fails, as the CPU path on one thread
            if (!sample_error[at].empty()) throw std::runtime_error(sample_error[at]);
            std::vector<uint8_t>().swap(samples[at].codes);
        }
        t_finish += since() - t1;
    }
    const double t_before_write = since();
    MultiSketch::write_sketch_data(output_prefix, bins.data(), bins.size());
    MultiSketch m(std::move(meta), ss64 * 64, kmers);
    m.set_hash_type(st.hash_type());
    m.save_metadata(output_prefix);
    m.set_bins(std::move(bins));
    if (timing) {
        std::fprintf(stderr, "TIMING sketch --gpu --seq-type aa: parse=%.3fs gather+upload+kernel+download=%.3fs densify+transpose=%.3fs write=%.3fs\n",
                     t_parse, t_gpu, t_finish, since() - t_before_write);
    }
    return m;
}
}  // namespace

MultiSketch sketch_files_gpu(Device &dev, const std::string &output_prefix, const std::vector<InputFastx> &inputs,
                             const std::vector<size_t> &kmers, uint64_t sketch_size, bool rc, size_t threads,
                             uint16_t min_count, uint8_t min_qual, const SeqType &st)
{
    if (st.aa) return sketch_files_gpu_aa(dev, output_prefix, inputs, kmers, sketch_size, rc, threads, st);
    const size_t n = inputs.size(), nk = kmers.size();
    const uint64_t ss64 = (sketch_size + 63) / 64;   // num_bins, sketch/mod.rs:49-54
    const uint64_t num_bins = ss64 * 64;
    const size_t sample_words = (size_t)(ss64 * BBITS * nk);

    const bool timing = std::getenv("SKL_CLI_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    double t_parse = 0, t_pack = 0, t_gpu = 0, t_finish = 0;

    std::vector<Sequence> seqs;
    raise_first(parse_inputs(inputs, min_qual, threads, seqs));

    t_parse = since();
    std::vector<uint64_t> bins(sample_words * n, 0);
    std::vector<SketchMeta> meta(n);
    // densify + transpose + metadata of sample `at` from its [nk][num_bins] signs on host threads: read sets under a count
    // filter, whose signs are produced on the host
    auto finish = [&](size_t at, const uint64_t *sample_signs, const char *any_window) {
        bool densified = false;
        std::vector<uint64_t> first_signs;
        for (size_t ki = 0; ki < nk; ++ki) {
            const uint64_t *src = sample_signs + ki * num_bins;
            std::vector<uint64_t> sg(src, src + num_bins);
            check_read_signs(any_window[ki] != 0, sg, inputs[at].first, kmers[ki], min_count);
            densified |= densify_bin(sg);
            first_signs.push_back(sg[0]);
            fill_usigs(bins.data() + at * sample_words + ki * ss64 * BBITS, sg);
        }
        meta[at] = dna_meta(inputs[at].first, at, seqs[at], rc, densified, first_signs);
    };
    // read sets under a count filter go their own way; assemblies (and read sets without one) take the bin-minimum kernel and
    // the finish kernel behind it
    std::vector<size_t> plain, filtered;
    for (size_t i = 0; i < n; ++i) (seqs[i].reads && min_count >= 2 ? filtered : plain).push_back(i);

    // 2. hash + bin minima + densify + transpose on the device, in batches of at most ~4 G bases
    for (const auto &[b0, b1] : batches(plain.size(), [&](size_t i) { return seqs[plain[i]].codes.size(); }, skl::caps_dna_call())) {
        const size_t nb = b1 - b0;
        const PackedBatch in = gather_and_pack(seqs, plain.data() + b0, nb, threads);
        // Hash, bin minima, densify and transpose on the device.  A batch's finished words are its samples' part of the `.skd`
        // image when the samples are consecutive in input order (always, unless read sets under a count filter lie between them).
        const bool in_place = plain[b1 - 1] - plain[b0] == nb - 1;
        std::vector<uint64_t> staged_words(in_place ? 0 : nb * sample_words), first_signs(nb * nk);
        std::vector<uint8_t> flags(nb * nk, 0);
        uint64_t *words = in_place ? bins.data() + plain[b0] * sample_words : staged_words.data();
        const double t0 = since();
        t_pack += t0 - (t_parse + t_pack + t_gpu + t_finish);
        const int rc_ = skl_sketch_usigs_packed(dev.ctx(), in.packed.get(), in.code_begin.data(), in.offsets.data(), in.offset_begin.data(),
                                                nb, kmers.data(), nk, num_bins, rc ? 1 : 0, words, first_signs.data(), flags.data());
        if (rc_ != SKL_OK) throw std::runtime_error(skl_last_error());
        t_gpu += since() - t0;
        // 3. metadata from the flags and first signs
        for (size_t i = 0; i < nb; ++i) {
            const size_t at = plain[b0 + i];
            bool densified = false;
            for (size_t ki = 0; ki < nk; ++ki) {
                if (flags[i * nk + ki] & SKL_FINISH_EMPTY) throw std::runtime_error("K-mer larger than smallest valid sequence");   // as the CPU path: the first such sample in input order
                densified |= (flags[i * nk + ki] & SKL_FINISH_DENSIFIED) != 0;
            }
            if (!in_place) memcpy(bins.data() + at * sample_words, words + i * sample_words, sample_words * sizeof(uint64_t));
            meta[at] = dna_meta(inputs[at].first, at, seqs[at], rc, densified,
                                std::vector<uint64_t>(first_signs.begin() + i * nk, first_signs.begin() + (i + 1) * nk));
        }
        for (size_t i = b0; i < b1; ++i) Sequence().codes.swap(seqs[plain[i]].codes);   // release
        t_finish = since() - t_parse - t_pack - t_gpu;
    }

    // 2'. read sets with a count filter: survivors on the device, the filter replayed on the host.  A batch holds at most
    // max(64, nk) streams (one 24 MiB filter each) and ~1 G bases.
    ReadsTiming rt;
    const double t_reads0 = since();
    for (const auto &[b0, b1] : batches(filtered.size(), [&](size_t i) { return seqs[filtered[i]].codes.size(); }, skl::caps_filtered_reads(nk))) {
        const std::vector<size_t> idx(filtered.begin() + b0, filtered.begin() + b1);
        std::vector<uint64_t> signs;
        std::vector<char> any_window;
        reads_signs_gpu(dev, seqs, idx, kmers, num_bins, rc, min_count, threads, signs, any_window, rt);
        raise_first(try_each(idx.size(), threads, [&](size_t i) {
            finish(idx[i], signs.data() + i * nk * num_bins, any_window.data() + i * nk);
        }));
        for (size_t i : idx) Sequence().codes.swap(seqs[i].codes);   // release
    }
    const double t_reads = since() - t_reads0;

    const double t_before_write = since();
    MultiSketch::write_sketch_data(output_prefix, bins.data(), bins.size());
    MultiSketch m(std::move(meta), ss64 * 64, kmers);
    m.save_metadata(output_prefix);
    m.set_bins(std::move(bins));
    if (timing) {
        std::fprintf(stderr, "TIMING sketch --gpu: parse=%.3fs pack=%.3fs upload+kernel+download=%.3fs densify+transpose=%.3fs write=%.3fs\n",
                     t_parse, t_pack, t_gpu, t_finish, since() - t_before_write);
        if (!filtered.empty()) {
            std::fprintf(stderr, "TIMING reads: total=%.3fs survivors_gpu=%.3fs replay_wait=%.3fs chunks=%llu window_starts=%llu "
                                 "survivors=%llu\n",
                         t_reads, rt.gpu, rt.replay_wait, (unsigned long long)rt.chunks, (unsigned long long)rt.window_starts,
                         (unsigned long long)rt.survivors);
        }
    }
    return m;
}

// `inverted build --gpu` / `inverted query --gpu`: the rows of an inverted index -- one k-mer length, exactly sketch_size bins,
// `sign as u16` -- with hashing, bin minima, densification and the u16 emit on the device.  Parsing and
// packing on host threads, batches as in sketch_files_gpu.  Every sample's error is kept and the first in input order is
// raised at the end, which is what the CPU path reports on one thread.
std::vector<std::vector<uint16_t>> sketch_inverted_gpu(Device &dev, const std::vector<InputFastx> &inputs, size_t k,
                                                       uint64_t sketch_size, bool rc, size_t threads, uint16_t min_count,
                                                       uint8_t min_qual, double *t_parse_out, double *t_pack_out, double *t_device_out)
{
    const size_t n = inputs.size();
    const uint64_t S = sketch_size;
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    double t_pack = 0, t_device = 0;

    std::vector<Sequence> seqs;
    std::vector<std::string> error = parse_inputs(inputs, min_qual, threads, seqs);
    const double t_parse = since();
    std::vector<std::vector<uint16_t>> out(n);
    // read sets under a count filter go their own way; assemblies (and read sets without one) take the bin-minimum kernel and
    // the u16 finish behind it
    std::vector<size_t> plain, filtered;
    for (size_t i = 0; i < n; ++i) {
        if (error[i].empty()) (seqs[i].reads && min_count >= 2 ? filtered : plain).push_back(i);
    }

    // 2. hash + bin minima + densify + u16 on the device, in batches of at most ~4 G bases and 1 GiB of signs on the device
    for (const auto &[b0, b1] : batches(plain.size(), [&](size_t i) { return seqs[plain[i]].codes.size(); }, skl::caps_u16_call(S))) {
        const double p0 = since();
        const size_t nb = b1 - b0;
        const PackedBatch in = gather_and_pack(seqs, plain.data() + b0, nb, threads);
        std::vector<uint16_t> rows(nb * S);
        std::vector<uint8_t> flags(nb, 0);
        const double d0 = since();
        t_pack += d0 - p0;
        if (skl_sketch_bins_u16_packed(dev.ctx(), in.packed.get(), in.code_begin.data(), in.offsets.data(), in.offset_begin.data(), nb, k, S,
                                       rc ? 1 : 0, rows.data(), flags.data()) != SKL_OK) {
            throw std::runtime_error(skl_last_error());
        }
        t_device += since() - d0;
        for (size_t i = 0; i < nb; ++i) {
            const size_t at = plain[b0 + i];
            if (flags[i] & SKL_FINISH_EMPTY) {
                error[at] = "K-mer larger than smallest valid sequence";   // as the CPU path
            } else {
                out[at].assign(rows.begin() + i * S, rows.begin() + (i + 1) * S);
            }
            Sequence().codes.swap(seqs[at].codes);   // release
        }
    }

    // 2'. read sets with a count filter: survivors on the device, the filter replayed on the host (one k, sketch_size bins),
    // then the u16 finish of their signs on the device.  A batch holds at most 64 streams (one 24 MiB filter each) and ~1 G bases.
    const std::vector<size_t> kmers{k};
    ReadsTiming rt;
    for (const auto &[b0, b1] : batches(filtered.size(), [&](size_t i) { return seqs[filtered[i]].codes.size(); }, skl::caps_filtered_reads(1))) {
        const double d0 = since();
        const std::vector<size_t> idx(filtered.begin() + b0, filtered.begin() + b1);
        std::vector<uint64_t> signs;
        std::vector<char> any_window;
        reads_signs_gpu(dev, seqs, idx, kmers, S, rc, min_count, threads, signs, any_window, rt);
        for (size_t i = 0; i < idx.size(); ++i) {
            try {
                check_read_signs(any_window[i] != 0, std::vector<uint64_t>(signs.begin() + i * S, signs.begin() + (i + 1) * S),
                                 inputs[idx[i]].first, k, min_count);
            } catch (const std::exception &e) {
                error[idx[i]] = e.what();
            }
        }
        std::vector<uint16_t> rows(idx.size() * S);
        std::vector<uint8_t> flags(idx.size(), 0);
        if (skl_sketch_finish_u16(dev.ctx(), signs.data(), idx.size(), S, rows.data(), flags.data()) != SKL_OK) {
            throw std::runtime_error(skl_last_error());
        }
        for (size_t i = 0; i < idx.size(); ++i) {
            if (error[idx[i]].empty()) out[idx[i]].assign(rows.begin() + i * S, rows.begin() + (i + 1) * S);
            Sequence().codes.swap(seqs[idx[i]].codes);   // release
        }
        t_device += since() - d0;
    }
    raise_first(error);
    if (t_parse_out) *t_parse_out = t_parse;
    if (t_pack_out) *t_pack_out = t_pack;
    if (t_device_out) *t_device_out = t_device;
    return out;
}

}  // namespace skl_host
