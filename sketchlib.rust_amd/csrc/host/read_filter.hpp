// read_filter.hpp -- the k-mer count filter of read sketching (src/hashing/bloom_filter.rs) and the
// rule that offers a window's sign to it (Sketch::bin_sign, src/sketch/mod.rs:198-210).  The CPU path
// (sketch.cpp) offers every window; the GPU path (sketch_gpu.cpp) offers only the survivors of
// skl_reads_survivors, in the same order -- DESIGN.md §4.5 has why both give the same bins.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <unordered_map>
#include <vector>

namespace skl_host {

// KmerFilter (bloom_filter.rs:31-175): a blocked Bloom filter of round(2^27 * 12 / 8 / 64) u64 words
// removes singletons; from its second hit on, a hash map counts (starting at 2) and the k-mer passes
// when the count EQUALS min_count.  min_count 0 or 1: everything passes; 2: the Bloom filter alone.
class KmerFilter {
public:
    explicit KmerFilter(uint16_t min_count);
    // clear (bloom_filter.rs:113-118): empty Bloom filter and counts; called before every k-mer length
    void clear();
    // filter(hash) == Ordering::Equal (bloom_filter.rs:120-152)
    bool pass(uint64_t hash);
    uint16_t min_count() const { return min_count_; }

private:
    bool bloom_add_and_check(uint64_t key);
    struct FreeDeleter {
        void operator()(uint64_t *p) const { std::free(p); }
    };
    uint64_t buf_size_;
    std::unique_ptr<uint64_t, FreeDeleter> buffer_;   // zeroed lazily (calloc): a filter nobody offers to costs no pages
    std::unordered_map<uint64_t, uint16_t> counts_;
    uint16_t min_count_;
};

// bin_sign with a filter (sketch/mod.rs:198-210): the sign is offered only if it would lower its bin.
inline void offer_sign(uint64_t *signs, uint64_t bin_size, KmerFilter &filter, uint64_t sign)
{
    uint64_t &slot = signs[sign / bin_size];
    if (sign < slot && filter.pass(sign)) slot = sign;
}

// Sketch::new's sequence length of a read set (sketch/mod.rs:95-128):
// `(nk as f64 / sum_k (signs_k[0] as f64 / SIGN_MOD as f64)) as usize`, the sum in k order, signs taken after
// densification; Rust's `as usize` saturates (inf -> usize::MAX, NaN and negatives -> 0).
uint64_t reads_seq_length(const std::vector<uint64_t> &first_sign_per_k);

}  // namespace skl_host
