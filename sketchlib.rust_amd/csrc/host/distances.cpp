#include "distances_impl.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <exception>
#include <ostream>
#include <string>
#include <thread>

namespace skl_host {

Device::Device(int device) { detail::check(skl_ctx_create(device, &ctx_)); }
Device::~Device() { skl_ctx_destroy(ctx_); }

DeviceSet::DeviceSet(const std::vector<int> &devices)
{
    if (devices.empty()) throw std::runtime_error("no devices given");
    for (int d : devices) devs_.push_back(std::make_unique<Device>(d));
}

namespace {
// the result arrays of the C ABI: written whole by the call, never read before
template <class T>
using RawVec = std::vector<T, DefaultInitAllocator<T>>;

// records [0, n) by several threads (a million samples x 50 neighbours: 50 M records)
template <class Fill>
void fill_records(size_t n, const Fill &fill)
{
    const size_t n_threads = n >= (1u << 20) ? std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency())) : 1;
    std::vector<std::thread> pool;
    for (size_t t = 1; t < n_threads; ++t) pool.emplace_back([&, t] { fill(n * t / n_threads, n * (t + 1) / n_threads); });
    fill(0, n / n_threads);
    for (auto &th : pool) th.join();
}
}  // namespace

namespace detail {
void check(int rc)
{
    if (rc == SKL_OK) return;
    const std::string msg = skl_last_error();
    // reference panics keep their panic status (exit 101); the rest are ordinary errors
    if (rc == SKL_ERR_KMER_COUNT || rc == SKL_ERR_EMPTY_DB) throw Panic(msg);
    throw std::runtime_error(msg);
}

SparseDistanceMatrix assemble_knn(const DistType &dist_type, size_t knn, const uint64_t *idx, const float *d0, const float *d1, size_t n_records)
{
    SparseDistanceMatrix out;
    out.jaccard = dist_type;
    out.knn = knn;
    out.n_distances = n_records;
    if (dist_type.kind == DistType::CoreAcc) {
        out.coreacc_dists.resize(n_records);
        fill_records(n_records, [&](size_t a, size_t b) {
            for (size_t i = a; i < b; ++i) out.coreacc_dists[i] = {(size_t)idx[i], d0[i], d1[i]};
        });
    } else {
        out.jaccard_dists.resize(n_records);
        fill_records(n_records, [&](size_t a, size_t b) {
            for (size_t i = a; i < b; ++i) out.jaccard_dists[i] = {(size_t)idx[i], d0[i]};
        });
    }
    return out;
}

skl_dist_params to_params(const DistType &d, double cutoff)
{
    skl_dist_params p;
    p.dist_type = d.kind == DistType::CoreAcc ? SKL_DIST_COREACC : SKL_DIST_JACCARD;
    p.ani = d.ani ? 1 : 0;
    p.k_idx = d.k_idx;
    p.completeness_cutoff = cutoff;
    return p;
}

std::vector<std::string> sketch_names(const MultiSketch &m)
{
    std::vector<std::string> names;
    for (size_t i = 0; i < m.number_samples_loaded(); ++i) names.push_back(m.sketch_name(i));
    return names;
}
}  // namespace detail

namespace distances {

using namespace detail;

DistType set_k(const MultiSketch &sketches, std::optional<size_t> kmer, bool ani)
{
    DistType d;
    if (kmer) {
        const auto k_idx = sketches.get_k_idx(*kmer);
        if (!k_idx) throw std::runtime_error("K-mer size " + std::to_string(*kmer) + " not found in file");
        d.kind = DistType::Jaccard;
        d.k_idx = *k_idx;
        d.k = (double)*kmer;
        d.ani = ani;
    } else {
        d.kind = DistType::CoreAcc;
    }
    return d;
}

DistanceMatrix self_dists_all(Device &dev, const MultiSketch &sketches, size_t n, const DistType &dist_type,
                              bool /*quiet*/, const std::vector<double> *completeness_vec,
                              double completeness_cutoff)
{
    DistanceMatrix out;  // DistanceMatrix::new, distance_matrix.rs:132-158
    out.jaccard = dist_type;
    out.ref_names = sketch_names(sketches);
    out.n_distances = n * (n - 1) / 2;
    out.distances.assign(out.n_distances * dist_type.n_dist_cols(), 0.0f);
    Slab s(dev, sketches, completeness_vec);
    const skl_dist_params p = to_params(dist_type, completeness_cutoff);
    check(skl_self_dists_all(dev.ctx(), s.h, &p, out.distances.data(), 0));
    return out;
}

DistanceMatrix cross_dists_all(Device &dev, const MultiSketch &ref_sketches,
                               const MultiSketch &query_sketches, size_t n, size_t n_query,
                               const DistType &dist_type, bool /*quiet*/,
                               const std::vector<double> *ref_completeness_vec,
                               const std::vector<double> *query_completeness_vec,
                               double completeness_cutoff)
{
    DistanceMatrix out;
    out.jaccard = dist_type;
    out.ref_names = sketch_names(ref_sketches);
    out.query_names = sketch_names(query_sketches);
    out.n_distances = n * n_query;
    out.distances.assign(out.n_distances * dist_type.n_dist_cols(), 0.0f);
    Slab r(dev, ref_sketches, ref_completeness_vec);
    Slab q(dev, query_sketches, query_completeness_vec);
    const skl_dist_params p = to_params(dist_type, completeness_cutoff);
    check(skl_cross_dists_all(dev.ctx(), r.h, q.h, &p, out.distances.data(), 0));
    return out;
}

static SparseDistanceMatrix run_knn(Device &dev, skl_sketches *ref, skl_sketches *query, size_t rows,
                                    size_t knn, const DistType &dist_type, double cutoff)
{
    const size_t n_records = rows * knn;
    RawVec<uint64_t> idx(n_records);
    RawVec<float> d0(n_records), d1(n_records);
    const skl_dist_params p = to_params(dist_type, cutoff);
    if (query) {
        check(skl_cross_dists_knn(dev.ctx(), ref, query, &p, knn, idx.data(), d0.data(), d1.data(), 0));
    } else {
        check(skl_self_dists_knn(dev.ctx(), ref, &p, knn, idx.data(), d0.data(), d1.data(), 0));
    }
    return assemble_knn(dist_type, knn, idx.data(), d0.data(), d1.data(), n_records);
}

SparseDistanceMatrix self_dists_knn(Device &dev, const MultiSketch &sketches, size_t n, size_t knn,
                                    const DistType &dist_type, bool /*quiet*/,
                                    const std::vector<double> *completeness_vec,
                                    double completeness_cutoff)
{
    Slab s(dev, sketches, completeness_vec);
    SparseDistanceMatrix out = run_knn(dev, s.h, nullptr, n, knn, dist_type, completeness_cutoff);
    out.ref_names = sketch_names(sketches);
    return out;
}

SparseDistanceMatrix cross_dists_knn(Device &dev, const MultiSketch &ref_sketches,
                                     const MultiSketch &query_sketches, size_t n, size_t n_query,
                                     size_t knn, const DistType &dist_type, bool /*quiet*/,
                                     const std::vector<double> *ref_completeness_vec,
                                     const std::vector<double> *query_completeness_vec,
                                     double completeness_cutoff)
{
    if (n == 0) throw Panic("Reference database has no loaded samples");   // mod.rs:318-320
    if (n_query == 0) throw Panic("Query database has no loaded samples");  // mod.rs:321-323
    knn = std::min(knn, n);                                                 // mod.rs:325
    Slab r(dev, ref_sketches, ref_completeness_vec);
    Slab q(dev, query_sketches, query_completeness_vec);
    SparseDistanceMatrix out = run_knn(dev, r.h, q.h, n_query, knn, dist_type, completeness_cutoff);
    out.ref_names = sketch_names(ref_sketches);
    out.query_names = sketch_names(query_sketches);
    return out;
}

// ---------------------------------------------------------------------------
// pair list
// ---------------------------------------------------------------------------

void dists_pairs(Device &dev, const MultiSketch &ref_sketches, const MultiSketch *query_sketches, const PairsFile &pairs,
                 const std::vector<std::string> &first_names, const std::vector<std::string> &second_names,
                 const DistType &dist_type, const std::vector<double> *ref_completeness_vec,
                 const std::vector<double> *query_completeness_vec, double completeness_cutoff, TextSink &sink,
                 size_t threads)
{
    const size_t n_pairs = pairs.size();
    const size_t ncols = dist_type.n_dist_cols();
    const skl_dist_params p = to_params(dist_type, completeness_cutoff);
    RawVec<float> dist(n_pairs * ncols);
    if (query_sketches) {
        Slab r(dev, ref_sketches, ref_completeness_vec);
        Slab q(dev, *query_sketches, query_completeness_vec);
        check(skl_cross_dists_pairs(dev.ctx(), r.h, q.h, &p, pairs.first.data(), pairs.second.data(), n_pairs, dist.data(), 0));
    } else {
        Slab s(dev, ref_sketches, ref_completeness_vec);
        check(skl_self_dists_pairs(dev.ctx(), s.h, &p, pairs.first.data(), pairs.second.data(), n_pairs, dist.data(), 0));
    }
    write_pair_list(sink, first_names, second_names, pairs.first.data(), pairs.second.data(), n_pairs, dist.data(), ncols, threads);
}

// ---------------------------------------------------------------------------
// precluster
// ---------------------------------------------------------------------------

namespace {
// sample name -> position in the .ski
std::unordered_map<std::string, size_t> ski_positions(const Inverted &inv)
{
    std::unordered_map<std::string, size_t> pos;
    for (size_t i = 0; i < inv.sample_names.size(); ++i) pos.emplace(inv.sample_names[i], i);
    return pos;
}

// sample sets of .ski and .skm must agree; i <-> j lookups (mod.rs:412-440)
struct NameMaps {
    std::vector<size_t> ski_of_skd, skd_of_ski;
};
NameMaps map_names(const MultiSketch &sketches, const Inverted &inv, size_t n)
{
    const std::unordered_map<std::string, size_t> skq_lookup = ski_positions(inv);
    NameMaps m;
    std::string not_found;
    for (size_t i = 0; i < sketches.number_samples_loaded(); ++i) {
        const auto it = skq_lookup.find(sketches.sketch_name(i));
        if (it != skq_lookup.end()) m.ski_of_skd.push_back(it->second);
        else not_found += (not_found.empty() ? "\"" : ", \"") + sketches.sketch_name(i) + "\"";
    }
    if (!not_found.empty()) {
        throw Panic("The following samples in the .skd could not be found in the .ski:\n[" + not_found + "]");
    }
    m.skd_of_ski.assign(std::max(n, inv.sample_names.size()), 0);
    for (size_t i = 0; i < m.ski_of_skd.size(); ++i) m.skd_of_ski[m.ski_of_skd[i]] = i;
    return m;
}

// Candidate lists built on the host (inverted.rs:259-268), in .skd ids, self excluded.  Every worker appends its rows' lists to
// ONE growing buffer of its own (a few large allocations instead of one per row: 64 threads faulting in millions of small
// blocks serialise on the address-space lock) and records where each row went.
struct RowRef {
    uint32_t worker = 0;
    uint32_t len = 0;
    uint64_t begin = 0;
};
struct HostLists {
    std::vector<RowRef> rows;
    std::vector<std::vector<uint32_t>> arena;   // one per worker
};
HostLists host_candidate_lists(const Inverted &inv, const std::vector<uint16_t> &skq_bins, size_t skq_stride, size_t n,
                               const NameMaps &names, bool reference_order, size_t n_workers)
{
    HostLists lists{std::vector<RowRef>(n), std::vector<std::vector<uint32_t>>(n_workers)};
    std::atomic<size_t> next{0};
    std::exception_ptr err;
    std::mutex mu;
    auto work = [&](size_t wid) {
        try {
            std::vector<uint32_t> stamp(inv.n_samples, 0), hits;   // per-thread scratch
            std::vector<uint32_t> &buf = lists.arena[wid];
            uint32_t epoch = 0;
            for (;;) {
                const size_t i0 = next.fetch_add(256);
                if (i0 >= n) break;
                for (size_t i = i0; i < std::min(n, i0 + 256); ++i) {
                    const size_t ski_i = names.ski_of_skd[i];
                    if (++epoch == 0) {   // wrapped: start over
                        std::fill(stamp.begin(), stamp.end(), 0u);
                        epoch = 1;
                    }
                    inv.any_shared_bins(skq_bins.data() + ski_i * skq_stride, stamp, epoch, hits);
                    const size_t begin = buf.size();
                    for (uint32_t j : hits) {   // (ascending .ski index)
                        if (j != ski_i) buf.push_back((uint32_t)names.skd_of_ski[j]);   // mod.rs:458-461
                    }
                    // canonical ties: ascending .skd id (the lists are a set); the reference's tie order: the order the
                    // reference pushes them in, i.e. as any_shared_bins returned them
                    if (!reference_order) std::sort(buf.begin() + begin, buf.end());
                    lists.rows[i].worker = (uint32_t)wid;
                    lists.rows[i].begin = begin;
                    lists.rows[i].len = (uint32_t)(buf.size() - begin);
                }
            }
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu);
            err = std::current_exception();
        }
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < n_workers; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto &t : pool) t.join();
    if (err) std::rethrow_exception(err);
    return lists;
}

// the lists as one CSR, copied by n_workers threads: offsets [n + 1] and the candidates; the arenas are gone on return
std::unique_ptr<uint32_t[]> lists_to_csr(HostLists lists, size_t n_workers, std::vector<uint64_t> &offsets)
{
    const size_t n = lists.rows.size();
    offsets.assign(n + 1, 0);
    for (size_t i = 0; i < n; ++i) offsets[i + 1] = offsets[i] + lists.rows[i].len;
    std::unique_ptr<uint32_t[]> cand(new uint32_t[std::max<uint64_t>(offsets[n], 1)]);   // not zero-filled
    std::atomic<size_t> next{0};
    auto copy_work = [&] {
        for (;;) {
            const size_t i0 = next.fetch_add(1024);
            if (i0 >= n) break;
            for (size_t i = i0; i < std::min(n, i0 + 1024); ++i) {
                const uint32_t *src = lists.arena[lists.rows[i].worker].data() + lists.rows[i].begin;
                std::copy(src, src + lists.rows[i].len, cand.get() + offsets[i]);
            }
        }
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < n_workers; ++t) pool.emplace_back(copy_work);
    copy_work();
    for (auto &t : pool) t.join();
    return cand;
}

// genomes without a prefilter match (mod.rs:487-527)
void retain_unmatched_rows(Device &dev, const Slab &s, const skl_dist_params &p, size_t knn, RetainUnmatched retain,
                           const std::vector<uint8_t> &unmatched, std::vector<uint64_t> &idx, std::vector<float> &d0)
{
    if (retain == RetainUnmatched::None) return;
    std::vector<uint64_t> bi(knn);
    std::vector<float> b0(knn), b1(knn);
    for (size_t i = 0; i < unmatched.size(); ++i) {
        if (!unmatched[i]) continue;
        if (retain == RetainUnmatched::Singleton) {
            for (size_t t = 0; t < knn; ++t) {
                idx[i * knn + t] = i;
                d0[i * knn + t] = t == 0 ? 0.0f : 1.0f;
            }
        } else {
            check(skl_self_dists_knn_rows(dev.ctx(), s.h, &p, knn, i, i + 1, bi.data(), b0.data(), b1.data(), 0));
            std::copy(bi.begin(), bi.end(), idx.begin() + i * knn);
            std::copy(b0.begin(), b0.end(), d0.begin() + i * knn);
        }
    }
}
}  // namespace

SparseDistanceMatrix self_dists_knn_precluster(Device &dev, const MultiSketch &sketches, const Inverted &inv,
                                               const std::vector<uint16_t> &skq_bins, size_t skq_stride, size_t n,
                                               size_t knn, const DistType &dist_type,
                                               const std::vector<double> *completeness_vec,
                                               double completeness_cutoff, RetainUnmatched retain, size_t threads, int knn_ties)
{
    const NameMaps names = map_names(sketches, inv, n);
    if (dist_type.kind == DistType::CoreAcc) {
        throw Panic("not implemented: Prefilter only available for single k-mer distances");   // mod.rs:549-551
    }

    const bool timing = std::getenv("SKL_CLI_TIMING") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); };
    const bool reference_order = knn_ties == SKL_KNN_TIES_REFERENCE;
    check(skl_ctx_set_knn_ties(dev.ctx(), knn_ties));
    bool monotone = true;   // does ascending .skd id mean ascending .ski index?
    for (size_t i = 1; i < names.ski_of_skd.size(); ++i) monotone = monotone && names.ski_of_skd[i - 1] < names.ski_of_skd[i];
    if (reference_order && !monotone && !inv.has_index()) {
        throw std::runtime_error("the reference's tie order pushes a row's candidates in ascending .ski index, and this .ski orders the "
                                 "samples differently from the .skd: load the index (host candidate lists)");
    }
    Slab s(dev, sketches, completeness_vec);
    const skl_dist_params p = to_params(dist_type, completeness_cutoff);
    std::vector<uint64_t> idx(n * knn);
    std::vector<float> d0(n * knn), d1;
    std::vector<uint8_t> unmatched(n, 0);
    if (!inv.has_index()) {
        // candidate lists on the device: index sketches re-ordered to .skd order
        std::vector<uint16_t> skq_skd(n * skq_stride);
        for (size_t i = 0; i < n; ++i) {
            std::copy(skq_bins.begin() + names.ski_of_skd[i] * skq_stride, skq_bins.begin() + (names.ski_of_skd[i] + 1) * skq_stride,
                      skq_skd.begin() + i * skq_stride);
        }
        uint64_t total = 0;
        check(skl_self_dists_knn_shared_bins(dev.ctx(), s.h, &p, knn, skq_skd.data(), skq_stride, idx.data(), d0.data(),
                                             &total));
        // a row whose first entry is padding (itself at distance 1) had no candidate at all
        for (size_t i = 0; i < n; ++i) unmatched[i] = idx[i * knn] == i;
        if (timing) {
            std::fprintf(stderr, "TIMING precluster: %llu candidate pairs; device candidate search + distances + top-k=%.3fs\n",
                         (unsigned long long)total, since());
        }
    } else {
        const size_t n_workers = std::max<size_t>(1, threads);
        HostLists lists = host_candidate_lists(inv, skq_bins, skq_stride, n, names, reference_order, n_workers);
        const double t_lists = since();
        std::vector<uint64_t> offsets;
        const std::unique_ptr<uint32_t[]> cand = lists_to_csr(std::move(lists), n_workers, offsets);
        for (size_t i = 0; i < n; ++i) unmatched[i] = offsets[i + 1] == offsets[i];
        const double t_csr = since();

        const double t_slab = since();
        check(skl_self_dists_knn_candidates(dev.ctx(), s.h, &p, knn, offsets.data(), cand.get(), idx.data(), d0.data()));
        if (timing) {
            std::fprintf(stderr, "TIMING precluster: %llu candidate pairs; lists=%.3fs csr=%.3fs slab upload=%.3fs "
                                 "candidate upload+distances+top-k=%.3fs\n",
                         (unsigned long long)offsets[n], t_lists, t_csr - t_lists, t_slab - t_csr, since() - t_slab);
        }
    }
    retain_unmatched_rows(dev, s, p, knn, retain, unmatched, idx, d0);
    SparseDistanceMatrix out = assemble_knn(dist_type, knn, idx.data(), d0.data(), d1.data(), idx.size());
    out.ref_names = sketch_names(sketches);
    return out;
}

bool ski_order_is_skd_order(const MultiSketch &sketches, const Inverted &inv)
{
    const std::unordered_map<std::string, size_t> pos = ski_positions(inv);
    size_t last = 0;
    for (size_t i = 0; i < sketches.number_samples_loaded(); ++i) {
        const auto it = pos.find(sketches.sketch_name(i));
        if (it == pos.end()) return true;   // (reported by self_dists_knn_precluster itself)
        if (i && it->second <= last) return false;
        last = it->second;
    }
    return true;
}

// ---------------------------------------------------------------------------
// streaming dense drivers
// ---------------------------------------------------------------------------

namespace {
// Compute bands [b[i], b[i+1]) one after the other; while band i is formatted and written,
// band i+1 is already being computed (one helper thread drives the GPU call).
template <class Compute>
void stream_bands(const DistanceMatrix &shape, const std::vector<size_t> &b, size_t max_band_floats,
                  Compute compute, TextSink &sink, size_t threads, bool npy)
{
    const size_t ncols = shape.jaccard.n_dist_cols();
    const size_t n_rows = shape.ref_names.size();
    auto band_floats = [&](size_t r0, size_t r1) {
        if (shape.query_names) return (r1 - r0) * shape.query_names->size() * ncols;
        r1 = std::min(r1, n_rows ? n_rows - 1 : 0);
        if (r1 <= r0) return (size_t)0;
        auto upto = [&](size_t r) { return r * n_rows - r * (r + 1) / 2; };   // pairs with i < r
        return (upto(r1) - upto(r0)) * ncols;
    };
    if (npy) {
        const std::string h = npy_header(shape.n_distances, ncols);
        sink.finish(sink.begin(h.data(), h.size()), h.data(), h.size());
    }
    std::vector<float> buf[2];
    buf[0].resize(max_band_floats);
    buf[1].resize(max_band_floats);
    std::exception_ptr err;
    auto launch = [&](size_t i) {
        return std::thread([&, i] {
            try {
                compute(b[i], b[i + 1], buf[i & 1].data());
            } catch (...) {
                err = std::current_exception();
            }
        });
    };
    const size_t n_bands = b.size() - 1;
    if (n_bands == 0) return;
    std::thread worker = launch(0);
    for (size_t i = 0; i < n_bands; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        worker.join();
        output_timing().wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (err) std::rethrow_exception(err);
        if (i + 1 < n_bands) worker = launch(i + 1);
        if (npy) {
            const char *bytes = reinterpret_cast<const char *>(buf[i & 1].data());
            const size_t len = band_floats(b[i], b[i + 1]) * sizeof(float);
            const auto t1 = std::chrono::steady_clock::now();
            write_raw(sink, bytes, len);
            output_timing().sink_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        } else {
            shape.write_rows(sink, b[i], b[i + 1], buf[i & 1].data(), threads);
        }
    }
}

}  // namespace

std::string npy_header(size_t rows, size_t cols)
{
    std::string dict = "{'descr': '<f4', 'fortran_order': False, 'shape': (" + std::to_string(rows) + ", " +
                       std::to_string(cols) + "), }";
    // magic(6) + version(2) + header length(2) + dict + padding + '\n' must be a multiple of 64
    size_t total = 10 + dict.size() + 1;
    const size_t pad = (64 - total % 64) % 64;
    dict.append(pad, ' ');
    dict.push_back('\n');
    std::string h("\x93NUMPY", 6);
    h.push_back('\x01');
    h.push_back('\x00');
    h.push_back((char)(dict.size() & 0xFF));
    h.push_back((char)((dict.size() >> 8) & 0xFF));
    return h + dict;
}

void self_dists_all_streamed(Device &dev, const MultiSketch &sketches, size_t n, const DistType &dist_type,
                             const std::vector<double> *completeness_vec, double completeness_cutoff,
                             TextSink &sink, size_t threads, size_t band_bytes, bool npy)
{
    if (n < 2) return;
    DistanceMatrix shape;   // names + type only; no n^2 storage
    shape.jaccard = dist_type;
    shape.ref_names = sketch_names(sketches);
    shape.n_distances = n * (n - 1) / 2;
    const size_t ncols = dist_type.n_dist_cols();
    const size_t band_pairs = std::max<size_t>(n, band_bytes / (ncols * sizeof(float)));
    std::vector<size_t> b = {0};
    size_t acc = 0, max_pairs = 0;
    for (size_t i = 0; i + 1 < n; ++i) {
        const size_t row = n - 1 - i;
        if (acc && acc + row > band_pairs) {
            b.push_back(i);
            max_pairs = std::max(max_pairs, acc);
            acc = 0;
        }
        acc += row;
    }
    b.push_back(n);
    max_pairs = std::max(max_pairs, acc);
    Slab s(dev, sketches, completeness_vec);
    const skl_dist_params p = to_params(dist_type, completeness_cutoff);
    stream_bands(shape, b, max_pairs * ncols,
                 [&](size_t r0, size_t r1, float *out) { check(skl_self_dists_rows(dev.ctx(), s.h, &p, r0, r1, out, 0)); },
                 sink, threads, npy);
}

void cross_dists_all_streamed(Device &dev, const MultiSketch &ref_sketches, const MultiSketch &query_sketches,
                              size_t n, size_t n_query, const DistType &dist_type,
                              const std::vector<double> *ref_completeness_vec,
                              const std::vector<double> *query_completeness_vec, double completeness_cutoff,
                              TextSink &sink, size_t threads, size_t band_bytes, bool npy)
{
    if (n == 0 || n_query == 0) return;
    DistanceMatrix shape;
    shape.jaccard = dist_type;
    shape.ref_names = sketch_names(ref_sketches);
    shape.query_names = sketch_names(query_sketches);
    shape.n_distances = n * n_query;
    const size_t ncols = dist_type.n_dist_cols();
    const size_t rows_per_band = std::max<size_t>(1, band_bytes / (n_query * ncols * sizeof(float)));
    std::vector<size_t> b;
    for (size_t r = 0; r < n; r += rows_per_band) b.push_back(r);
    b.push_back(n);
    Slab r(dev, ref_sketches, ref_completeness_vec);
    Slab q(dev, query_sketches, query_completeness_vec);
    const skl_dist_params p = to_params(dist_type, completeness_cutoff);
    stream_bands(shape, b, std::min(rows_per_band, n) * n_query * ncols,
                 [&](size_t r0, size_t r1, float *out) {
                     check(skl_cross_dists_rows(dev.ctx(), r.h, q.h, &p, r0, r1, out, 0));
                 },
                 sink, threads, npy);
}

}  // namespace distances
}  // namespace skl_host
