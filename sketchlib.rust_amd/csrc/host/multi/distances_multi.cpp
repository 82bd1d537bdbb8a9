// distances_multi.cpp -- the DeviceSet forms of the drivers: one context and one host thread per device, every device holding
// the whole slab.  WHAT each device gets -- row shards, column windows, dealt bands, which kNN form -- is decided by
// multi_plan.hpp on the calling thread before a worker starts; the functions here carry it out over the C ABI.
//
// This file calls the GPU library, so it lies in host/multi/, apart from host/*.cpp: what builds the host layer without the library
// (skl_dbtool, the CPU check programs under tests/native/) takes host/*.cpp less distances.cpp and sketch_gpu.cpp, by name.
#include "../distances_impl.hpp"
#include "../multi_plan.hpp"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <exception>
#include <memory>
#include <mutex>
#include <optional>
#include <thread>

namespace skl_host {
namespace distances {

using namespace detail;
using namespace multi_plan;

namespace {
// run fn(device index) on one thread per device; rethrow the first failure
template <class F>
void for_each_device(DeviceSet &devs, F fn)
{
    std::vector<std::exception_ptr> errs(devs.size());
    std::vector<std::thread> pool;
    for (size_t d = 0; d < devs.size(); ++d) {
        pool.emplace_back([&, d] {
            try {
                fn(d);
            } catch (...) {
                errs[d] = std::current_exception();
            }
        });
    }
    for (auto &t : pool) t.join();
    for (auto &e : errs) {
        if (e) std::rethrow_exception(e);
    }
}
}  // namespace

DistanceMatrix self_dists_all(DeviceSet &devs, const MultiSketch &sketches, size_t n, const DistType &dist_type,
                              bool quiet, const std::vector<double> *completeness_vec,
                              double completeness_cutoff)
{
    if (devs.size() == 1) return self_dists_all(devs[0], sketches, n, dist_type, quiet, completeness_vec, completeness_cutoff);
    DistanceMatrix out;
    out.jaccard = dist_type;
    out.ref_names = sketch_names(sketches);
    out.n_distances = n * (n - 1) / 2;
    const size_t ncols = dist_type.n_dist_cols();
    out.distances.assign(out.n_distances * ncols, 0.0f);
    const skl_dist_params p = to_params(dist_type, completeness_cutoff);
    const std::vector<size_t> b = self_row_bounds(n, devs.size());
    for_each_device(devs, [&](size_t d) {
        if (b[d + 1] <= b[d]) return;
        Slab s(devs[d], sketches, completeness_vec);
        const size_t first = b[d] + 1 < n ? square_to_condensed(b[d], b[d] + 1, n) : out.n_distances;
        check(skl_self_dists_rows(devs[d].ctx(), s.h, &p, b[d], b[d + 1], out.distances.data() + first * ncols, 0));
    });
    return out;
}

DistanceMatrix cross_dists_all(DeviceSet &devs, const MultiSketch &ref_sketches,
                               const MultiSketch &query_sketches, size_t n, size_t n_query,
                               const DistType &dist_type, bool quiet,
                               const std::vector<double> *ref_completeness_vec,
                               const std::vector<double> *query_completeness_vec,
                               double completeness_cutoff)
{
    if (devs.size() == 1) {
        return cross_dists_all(devs[0], ref_sketches, query_sketches, n, n_query, dist_type, quiet,
                               ref_completeness_vec, query_completeness_vec, completeness_cutoff);
    }
    DistanceMatrix out;
    out.jaccard = dist_type;
    out.ref_names = sketch_names(ref_sketches);
    out.query_names = sketch_names(query_sketches);
    out.n_distances = n * n_query;
    const size_t ncols = dist_type.n_dist_cols();
    out.distances.assign(out.n_distances * ncols, 0.0f);
    const skl_dist_params p = to_params(dist_type, completeness_cutoff);
    const std::vector<size_t> b = even_bounds(n, devs.size());
    for_each_device(devs, [&](size_t d) {
        if (b[d + 1] <= b[d]) return;
        Slab r(devs[d], ref_sketches, ref_completeness_vec);
        Slab q(devs[d], query_sketches, query_completeness_vec);
        check(skl_cross_dists_rows(devs[d].ctx(), r.h, q.h, &p, b[d], b[d + 1],
                                   out.distances.data() + b[d] * n_query * ncols, 0));
    });
    return out;
}

// ---------------------------------------------------------------------------
// self kNN over several devices
// ---------------------------------------------------------------------------
// Row shards evaluate every pair twice.  The other three forms evaluate it once:
//   THE REFERENCE'S TIE ORDER: partial heaps of disjoint candidate sets do not merge (a BinaryHeap's state depends on the order
//   its candidates arrive in), so device d owns the column window [cut[d], cut[d + 1]) and evaluates the pairs whose column lies
//   in it band by band.  TRAVELLING heaps: each band's heaps go to device d + 1 as soon as the band is done (skl_self_dists_knn_window),
//   and the last device ends up with every row's final heap.  DECOUPLED windows (skl_self_dists_knn_window_logged): every device
//   runs its window against heaps it has cleared itself and logs what they take; no device waits for another, and each device
//   then replays the logs of its row shard in window order.  The logs pass through host memory (this layer sees only the C ABI),
//   so that form is taken while they fit (multi_plan::knn_logs_fit_host) and hands over to the travelling heaps when a log overflows.
//   CANONICAL TIES (the reference evaluates (i, j) and (j, i), mod.rs:148-171): the row bands are DEALT back and forth over the
//   devices, each device returns its partial top-k states for ALL rows, and every device merges one row shard of the stacked states.
namespace {
struct DevMem {
    skl_ctx *c;
    void *p = nullptr;
    DevMem(skl_ctx *ctx_, size_t bytes) : c(ctx_) { check(skl_device_malloc(c, bytes, &p)); }
    ~DevMem() { skl_device_free(c, p); }
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    template <class T>
    T *as() const { return static_cast<T *>(p); }
};

// a device's reference heaps of `rows` rows: the RefHeap layout of skl_knn_heaps_* (h_d1 only for core/accessory)
struct Heaps {
    skl_ctx *ctx;
    size_t rows, knn;
    bool coreacc;
    DevMem key_m, id_m, d1_m, len_m, thr_m;
    Heaps(skl_ctx *c, size_t rows_, size_t knn_, bool coreacc_)
        : ctx(c), rows(rows_), knn(knn_), coreacc(coreacc_), key_m(c, rows * knn * 4), id_m(c, rows * knn * 4),
          d1_m(c, coreacc ? rows * knn * 4 : 4), len_m(c, rows * 4), thr_m(c, rows * 4) {}
    float *h_key() const { return key_m.as<float>(); }
    uint32_t *h_id() const { return id_m.as<uint32_t>(); }
    float *h_d1() const { return coreacc ? d1_m.as<float>() : nullptr; }
    uint32_t *h_len() const { return len_m.as<uint32_t>(); }
    uint32_t *thr() const { return thr_m.as<uint32_t>(); }
    void clear() const { check(skl_knn_heaps_clear(ctx, 0, rows, h_len(), thr())); }
    // into_sorted_vec of every heap, the lists to host rows [row0, row0 + rows) of the output
    void finalize_to(int ani, size_t row0, std::vector<uint64_t> &idx, std::vector<float> &d0, std::vector<float> &d1) const
    {
        DevMem o_idx(ctx, rows * knn * 8), o_d0(ctx, rows * knn * 4), o_d1(ctx, coreacc ? rows * knn * 4 : 4);
        check(skl_knn_heaps_finalize(ctx, rows, knn, h_key(), h_id(), h_d1(), h_len(), ani, o_idx.as<uint64_t>(), o_d0.as<float>(),
                                     coreacc ? o_d1.as<float>() : nullptr));
        check(skl_device_memcpy(ctx, idx.data() + row0 * knn, o_idx.p, rows * knn * 8, 0));
        check(skl_device_memcpy(ctx, d0.data() + row0 * knn, o_d0.p, rows * knn * 4, 0));
        if (coreacc) check(skl_device_memcpy(ctx, d1.data() + row0 * knn, o_d1.p, rows * knn * 4, 0));
    }
};

// Heap rows [r0, r1) between the device and a message of (r1 - r0) * knn_heap_wire_words: keys, ids[, second values], lengths,
// thresholds, each array's rows together.
void copy_rows(const Heaps &h, size_t r0, size_t r1, uint32_t *w, int to_device)
{
    const size_t rows = r1 - r0;
    auto part = [&](const DevMem &m, size_t per_row) {
        char *dev = m.as<char>() + r0 * per_row * 4;
        check(skl_device_memcpy(h.ctx, to_device ? (void *)dev : w, to_device ? (const void *)w : dev, rows * per_row * 4, to_device));
        w += rows * per_row;
    };
    part(h.key_m, h.knn);
    part(h.id_m, h.knn);
    if (h.coreacc) part(h.d1_m, h.knn);
    part(h.len_m, 1);
    part(h.thr_m, 1);
}
std::vector<uint32_t> export_rows(const Heaps &h, size_t r0, size_t r1)
{
    std::vector<uint32_t> buf((r1 - r0) * knn_heap_wire_words(h.knn, h.coreacc));
    copy_rows(h, r0, r1, buf.data(), 0);
    return buf;
}
void import_rows(const Heaps &h, size_t r0, size_t r1, std::vector<uint32_t> &buf) { copy_rows(h, r0, r1, buf.data(), 1); }

// what the forms work from, the plan they follow and the lists they fill
struct KnnJob {
    DeviceSet &devs;
    const MultiSketch &sketches;
    const std::vector<double> *completeness_vec;
    const size_t n, knn, W;
    const skl_dist_params p;
    const bool coreacc;
    const std::vector<size_t> b;   // even row shards: the rows device d finishes
    size_t band_rows = 0, n_bands = 0;
    std::vector<size_t> cut;       // column windows (reference ties)
    std::vector<uint64_t> idx;
    std::vector<float> d0, d1;
    std::unique_ptr<Slab> first_slab = nullptr;   // device 0's, uploaded on the calling thread: the plan is made from it
};
// Device d's slab for the length of its bands: every worker uploads its own, side by side, but for device 0, whose slab is there.
std::unique_ptr<Slab> slab_of(KnnJob &job, size_t d)
{
    return d == 0 ? std::move(job.first_slab) : std::make_unique<Slab>(job.devs[d], job.sketches, job.completeness_vec);
}

std::optional<KnnGaveUp> run_decoupled(KnnJob &job)
{
    const size_t n = job.n, knn = job.knn, W = job.W, band_rows = job.band_rows;
    const bool coreacc = job.coreacc;
    const size_t rec_w = knn_log_record_width(coreacc), cap = knn_log_cap(knn);
    std::vector<std::vector<float>> log_rec(W);
    std::vector<std::vector<uint32_t>> log_id(W), log_len(W);
    std::atomic<bool> give_up{false}, overflow{false};
    for_each_device(job.devs, [&](size_t d) {
        const std::unique_ptr<Slab> s = slab_of(job, d);
        skl_ctx *ctx = job.devs[d].ctx();
        const size_t lo = job.cut[d], hi = job.cut[d + 1];
        if (hi == 0) return;
        Heaps h(ctx, n, knn, coreacc);
        DevMem l_rec(ctx, hi * cap * rec_w * 4), l_id(ctx, hi * cap * 4), l_len(ctx, hi * 4);
        h.clear();
        {
            const std::vector<uint32_t> zeros(hi, 0u);
            check(skl_device_memcpy(ctx, l_len.p, zeros.data(), hi * 4, 1));
        }
        for (size_t band = 0; band < job.n_bands && !give_up; ++band) {
            if (band * band_rows >= hi) break;
            // (the log arrays cover rows [0, hi): no row at or behind the window's end meets a pair of it)
            const int r = skl_self_dists_knn_window_logged(ctx, s->h, &job.p, knn, band_rows, band, lo, hi, h.h_key(), h.h_id(), h.h_d1(), h.h_len(),
                                                           h.thr(), l_rec.as<float>(), l_id.as<uint32_t>(), l_len.as<uint32_t>(), cap);
            if (r == SKL_ERR_INVALID_ARG && band == 0) {   // no one-evaluation form for this configuration
                give_up = true;
                return;
            }
            check(r);
        }
        log_len[d].resize(hi);
        check(skl_device_memcpy(ctx, log_len[d].data(), l_len.p, hi * 4, 0));
        for (const uint32_t v : log_len[d]) {
            if (v > cap) give_up = overflow = true;   // an overflowed log is useless
        }
        if (give_up) return;
        log_rec[d].resize(hi * cap * rec_w);
        log_id[d].resize(hi * cap);
        check(skl_device_memcpy(ctx, log_rec[d].data(), l_rec.p, hi * cap * rec_w * 4, 0));
        check(skl_device_memcpy(ctx, log_id[d].data(), l_id.p, hi * cap * 4, 0));
    });
    if (give_up) return overflow ? KnnGaveUp::LogOverflow : KnnGaveUp::NoForm;
    // every device replays the logs of ITS row shard in window order into empty heaps, and sorts them
    for_each_device(job.devs, [&](size_t d) {
        const size_t r0 = job.b[d], r1 = job.b[d + 1], rows = r1 - r0;
        if (rows == 0) return;
        skl_ctx *ctx = job.devs[d].ctx();
        Heaps h(ctx, rows, knn, coreacc);
        DevMem u_rec(ctx, rows * cap * rec_w * 4), u_id(ctx, rows * cap * 4), u_len(ctx, rows * 4);
        h.clear();
        for (size_t src = 0; src < W; ++src) {
            const size_t a = r0, e = std::min(r1, job.cut[src + 1]);
            if (e <= a) continue;   // (rows at or behind window src's end: nothing of it)
            check(skl_device_memcpy(ctx, u_rec.p, log_rec[src].data() + a * cap * rec_w, (e - a) * cap * rec_w * 4, 1));
            check(skl_device_memcpy(ctx, u_id.p, log_id[src].data() + a * cap, (e - a) * cap * 4, 1));
            check(skl_device_memcpy(ctx, u_len.p, log_len[src].data() + a, (e - a) * 4, 1));
            check(skl_knn_heaps_replay(ctx, e - a, knn, coreacc ? 1 : 0, u_rec.as<float>(), u_id.as<uint32_t>(), u_len.as<uint32_t>(), cap,
                                       h.h_key(), h.h_id(), h.h_d1(), h.h_len(), h.thr()));
        }
        h.finalize_to(job.p.ani, r0, job.idx, job.d0, job.d1);
    });
    return std::nullopt;
}

std::optional<KnnGaveUp> run_travelling(KnnJob &job)
{
    const size_t n = job.n, knn = job.knn, W = job.W, band_rows = job.band_rows;
    struct Link {   // device d -> d + 1: bands in order
        std::mutex m;
        std::condition_variable cv;
        std::deque<std::vector<uint32_t>> q;
        bool broken = false;
    };
    std::vector<Link> link(W);
    std::atomic<bool> no_form{false};
    auto break_links = [&] {
        for (auto &l : link) {
            std::lock_guard<std::mutex> g(l.m);
            l.broken = true;
            l.cv.notify_all();
        }
    };
    for_each_device(job.devs, [&](size_t d) {
        try {
            const std::unique_ptr<Slab> s = slab_of(job, d);
            skl_ctx *ctx = job.devs[d].ctx();
            const size_t lo = job.cut[d], hi = job.cut[d + 1];
            Heaps h(ctx, n, knn, job.coreacc);
            h.clear();
            for (size_t band = 0; band < job.n_bands && !no_form; ++band) {
                const size_t b0 = band * band_rows, b1 = std::min(n, b0 + band_rows);
                if (b0 >= hi) break;
                if (b0 < lo) {   // rows of an earlier window: from the device that has just finished them
                    Link &in = link[d - 1];
                    std::unique_lock<std::mutex> g(in.m);
                    in.cv.wait(g, [&] { return !in.q.empty() || in.broken; });
                    if (in.q.empty()) {
                        if (no_form) return;   // (upstream found that the configuration has no one-evaluation form)
                        throw std::runtime_error("the device upstream of this one failed");
                    }
                    std::vector<uint32_t> buf = std::move(in.q.front());
                    in.q.pop_front();
                    g.unlock();
                    import_rows(h, b0, b1, buf);
                }
                const int r = skl_self_dists_knn_window(ctx, s->h, &job.p, knn, band_rows, band, lo, hi, h.h_key(), h.h_id(), h.h_d1(), h.h_len(), h.thr());
                if (r == SKL_ERR_INVALID_ARG && band == 0) {   // no one-evaluation form for this configuration
                    no_form = true;
                    break_links();
                    return;
                }
                check(r);
                if (d + 1 < W) {
                    std::vector<uint32_t> buf = export_rows(h, b0, b1);
                    Link &out_l = link[d];
                    std::lock_guard<std::mutex> g(out_l.m);
                    out_l.q.push_back(std::move(buf));
                    out_l.cv.notify_all();
                }
            }
            // every heap has ended on the last device: into_sorted_vec, lists to the host
            if (d + 1 == W && !no_form) h.finalize_to(job.p.ani, 0, job.idx, job.d0, job.d1);
        } catch (...) {
            break_links();   // nobody waits for a band that will not come
            throw;
        }
    });
    if (no_form) return KnnGaveUp::NoForm;
    return std::nullopt;
}

std::optional<KnnGaveUp> run_dealt(KnnJob &job)
{
    const size_t n = job.n, knn = job.knn, W = job.W;
    const bool coreacc = job.coreacc;
    std::vector<std::vector<uint32_t>> deal(W), key(W), sid(W);
    std::vector<std::vector<float>> sd1(W);
    for (size_t d = 0; d < W; ++d) deal[d] = knn_band_deal(job.n_bands, W, d);
    std::atomic<bool> no_form{false};
    for_each_device(job.devs, [&](size_t d) {
        const std::unique_ptr<Slab> s = slab_of(job, d);
        key[d].resize(n * knn);
        sid[d].resize(n * knn);
        if (coreacc) sd1[d].resize(n * knn);
        const int r = skl_self_dists_knn_partial(job.devs[d].ctx(), s->h, &job.p, knn, job.band_rows, deal[d].data(), deal[d].size(),
                                                 key[d].data(), sid[d].data(), coreacc ? sd1[d].data() : nullptr, 0);
        if (r == SKL_ERR_INVALID_ARG) no_form = true;   // no one-evaluation form for this configuration
        else check(r);
    });
    if (no_form) return KnnGaveUp::NoForm;
    for_each_device(job.devs, [&](size_t d) {
        const size_t r0 = job.b[d], rows = job.b[d + 1] - r0;
        if (rows == 0) return;
        std::vector<uint32_t> k_all(W * rows * knn), i_all(W * rows * knn);
        std::vector<float> d_all(coreacc ? W * rows * knn : 0);
        for (size_t w = 0; w < W; ++w) {
            std::copy_n(key[w].data() + r0 * knn, rows * knn, k_all.data() + w * rows * knn);
            std::copy_n(sid[w].data() + r0 * knn, rows * knn, i_all.data() + w * rows * knn);
            if (coreacc) std::copy_n(sd1[w].data() + r0 * knn, rows * knn, d_all.data() + w * rows * knn);
        }
        check(skl_knn_merge_states(job.devs[d].ctx(), W, rows, knn, k_all.data(), i_all.data(), coreacc ? d_all.data() : nullptr, 0,
                                   job.p.ani, job.idx.data() + r0 * knn, job.d0.data() + r0 * knn, job.d1.data() + r0 * knn, 0));
    });
    return std::nullopt;
}

void run_row_shards(KnnJob &job)
{
    for_each_device(job.devs, [&](size_t d) {
        const size_t r0 = job.b[d], r1 = job.b[d + 1];
        if (r1 <= r0) return;
        Slab s(job.devs[d], job.sketches, job.completeness_vec);
        check(skl_self_dists_knn_rows(job.devs[d].ctx(), s.h, &job.p, job.knn, r0, r1, job.idx.data() + r0 * job.knn,
                                      job.d0.data() + r0 * job.knn, job.d1.data() + r0 * job.knn, 0));
    });
}

// One attempt at a one-evaluation form: nothing, or why it gave up.  The plan -- band height, bands, windows -- is made HERE, once,
// before a worker starts.  skl_knn_band_rows wants a slab (it is a host-side rule over the sample count and the record width, the
// same whichever device's slab is asked), so device 0's is uploaded on this thread first and handed to device 0's worker; every
// device still makes the calls it made, in their order.
std::optional<KnnGaveUp> run_one_evaluation(KnnJob &job, KnnForm form)
{
    job.first_slab = std::make_unique<Slab>(job.devs[0], job.sketches, job.completeness_vec);
    job.band_rows = skl_knn_band_rows(job.first_slab->h, &job.p, job.W);
    if (job.band_rows == 0 && form != KnnForm::Dealt) throw std::runtime_error("skl_knn_band_rows failed");
    if (job.band_rows == 0) {
        job.first_slab.reset();
        return KnnGaveUp::NoForm;
    }
    job.n_bands = (job.n + job.band_rows - 1) / job.band_rows;
    if (form == KnnForm::Dealt) return run_dealt(job);
    job.cut = knn_window_cuts(job.n, job.band_rows, job.W);
    return form == KnnForm::Decoupled ? run_decoupled(job) : run_travelling(job);
}
}  // namespace

SparseDistanceMatrix self_dists_knn(DeviceSet &devs, const MultiSketch &sketches, size_t n, size_t knn,
                                    const DistType &dist_type, bool quiet,
                                    const std::vector<double> *completeness_vec,
                                    double completeness_cutoff)
{
    if (devs.size() == 1) return self_dists_knn(devs[0], sketches, n, knn, dist_type, quiet, completeness_vec, completeness_cutoff);
    const skl_dist_params p = to_params(dist_type, completeness_cutoff);
    KnnJob job{devs, sketches, completeness_vec, n, knn, devs.size(), p, p.dist_type == SKL_DIST_COREACC, even_bounds(n, devs.size()),
               0, 0, {}, std::vector<uint64_t>(n * knn), std::vector<float>(n * knn), std::vector<float>(n * knn), nullptr};
    const char *off = std::getenv("SKL_KNN_DECOUPLED");   // (=0: the travelling heaps, for tests and A/B timing)
    const bool reference_ties = skl_ctx_get_knn_ties(devs[0].ctx()) == SKL_KNN_TIES_REFERENCE;
    // decided up front: nothing is uploaded for a form the configuration does not have
    KnnForm form = first_knn_form(reference_ties, knn, n, job.W, job.coreacc, !(off && off[0] == '0'));
    while (form != KnnForm::RowShards) {
        const std::optional<KnnGaveUp> why = run_one_evaluation(job, form);
        if (!why) break;
        form = next_knn_form(form, *why);
    }
    if (form == KnnForm::RowShards) run_row_shards(job);
    SparseDistanceMatrix out = assemble_knn(dist_type, knn, job.idx.data(), job.d0.data(), job.d1.data(), job.idx.size());
    out.ref_names = sketch_names(sketches);
    return out;
}

SparseDistanceMatrix cross_dists_knn(DeviceSet &devs, const MultiSketch &ref_sketches,
                                     const MultiSketch &query_sketches, size_t n, size_t n_query,
                                     size_t knn, const DistType &dist_type, bool quiet,
                                     const std::vector<double> *ref_completeness_vec,
                                     const std::vector<double> *query_completeness_vec,
                                     double completeness_cutoff)
{
    if (devs.size() == 1) {
        return cross_dists_knn(devs[0], ref_sketches, query_sketches, n, n_query, knn, dist_type, quiet,
                               ref_completeness_vec, query_completeness_vec, completeness_cutoff);
    }
    if (n == 0) throw Panic("Reference database has no loaded samples");
    if (n_query == 0) throw Panic("Query database has no loaded samples");
    knn = std::min(knn, n);
    std::vector<uint64_t> idx(n_query * knn);
    std::vector<float> d0(n_query * knn), d1(n_query * knn);
    const skl_dist_params p = to_params(dist_type, completeness_cutoff);
    const std::vector<size_t> b = even_bounds(n_query, devs.size());
    for_each_device(devs, [&](size_t d) {
        if (b[d + 1] <= b[d]) return;
        Slab r(devs[d], ref_sketches, ref_completeness_vec);
        Slab q(devs[d], query_sketches, query_completeness_vec);
        check(skl_cross_dists_knn_rows(devs[d].ctx(), r.h, q.h, &p, knn, b[d], b[d + 1], idx.data() + b[d] * knn,
                                       d0.data() + b[d] * knn, d1.data() + b[d] * knn, 0));
    });
    SparseDistanceMatrix out = assemble_knn(dist_type, knn, idx.data(), d0.data(), d1.data(), idx.size());
    out.ref_names = sketch_names(ref_sketches);
    out.query_names = sketch_names(query_sketches);
    return out;
}

}  // namespace distances
}  // namespace skl_host
