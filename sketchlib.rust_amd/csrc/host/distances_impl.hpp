// distances_impl.hpp -- what distances.cpp (one device) and multi/distances_multi.cpp (several) share; defined in distances.cpp.
#pragma once

#include "distances.hpp"

#include "../../../include/sketchlib_dist.h"

namespace skl_host {
namespace detail {

// SKL_OK, or the library's message thrown: a Panic for the reference's panics (exit 101), a runtime_error for the rest
void check(int rc);

// RAII for a device-resident MultiSketch
struct Slab {
    skl_sketches *h = nullptr;
    Slab(Device &dev, const MultiSketch &m, const std::vector<double> *comp)
    {
        const size_t n = m.number_samples_loaded();
        check(skl_sketches_create(dev.ctx(), m.bins().data(), 0, n, m.kmer_lengths().size(),
                                  m.kmer_lengths().data(), (size_t)m.sketchsize64, &h));
        if (comp) check(skl_sketches_set_completeness(h, comp->data()));
    }
    ~Slab() { skl_sketches_destroy(h); }
    Slab(const Slab &) = delete;
    Slab &operator=(const Slab &) = delete;
};

skl_dist_params to_params(const DistType &d, double cutoff);
std::vector<std::string> sketch_names(const MultiSketch &m);
SparseDistanceMatrix assemble_knn(const DistType &dist_type, size_t knn, const uint64_t *idx, const float *d0, const float *d1, size_t n_records);

}  // namespace detail
}  // namespace skl_host
