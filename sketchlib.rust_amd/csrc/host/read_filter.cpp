#include "read_filter.hpp"

#include <cmath>
#include <new>

#include "sketch.hpp"

namespace skl_host {

namespace {
// reduce / cheap_mix / fingerprint, bloom_filter.rs:43-66
inline uint64_t reduce(uint64_t key, uint64_t range)
{
    return (uint64_t)(((unsigned __int128)key * (unsigned __int128)range) >> 64);
}
inline uint64_t cheap_mix(uint64_t key) { return (key ^ (key >> 31)) * 0x85D059AA333121CFull; }
inline uint64_t fingerprint(uint64_t key)
{
    return (1ull << (key & 63)) | (1ull << ((key >> 6) & 63)) | (1ull << ((key >> 12) & 63)) |
           (1ull << ((key >> 18) & 63)) | (1ull << ((key >> 24) & 63));
}
}  // namespace

KmerFilter::KmerFilter(uint16_t min_count)
    // BLOOM_WIDTH 2^27, BITS_PER_ENTRY 12 (bloom_filter.rs:12-17, 93-95): 3 145 728 words, 24 MiB
    : buf_size_((uint64_t)std::llround((double)(1u << 27) * (12.0 / 8.0) / 64.0)), min_count_(min_count)
{
}

void KmerFilter::clear()
{
    buffer_.reset();
    counts_.clear();
}

bool KmerFilter::bloom_add_and_check(uint64_t key)
{
    if (!buffer_) {
        buffer_.reset(static_cast<uint64_t *>(std::calloc(buf_size_, sizeof(uint64_t))));
        if (!buffer_) throw std::bad_alloc();
    }
    const uint64_t f_print = fingerprint(key);
    uint64_t &word = buffer_.get()[reduce(cheap_mix(key), buf_size_)];
    if ((word & f_print) == f_print) return true;
    word |= f_print;
    return false;
}

bool KmerFilter::pass(uint64_t hash)
{
    if (min_count_ <= 1) return true;
    if (!bloom_add_and_check(hash)) return false;
    if (min_count_ == 2) return true;
    uint16_t count = 2;
    auto it = counts_.find(hash);
    if (it == counts_.end()) {
        counts_.emplace(hash, count);
    } else {
        count = it->second == UINT16_MAX ? UINT16_MAX : (uint16_t)(it->second + 1);   // saturating_add
        it->second = count;
    }
    return count == min_count_;
}

uint64_t reads_seq_length(const std::vector<uint64_t> &first_sign_per_k)
{
    double minhash_sum = 0.0;
    for (uint64_t s : first_sign_per_k) minhash_sum += (double)s / (double)SIGN_MOD;
    const double v = (double)first_sign_per_k.size() / minhash_sum;
    if (std::isnan(v) || v <= 0.0) return 0;
    if (v >= 18446744073709551616.0) return UINT64_MAX;   // 2^64 and inf
    return (uint64_t)v;
}

}  // namespace skl_host
