// finish_u16_check.cpp -- the u16 form of csrc/finish_plan.hpp on the CPU: its launch rules as numbers, and finish_stream_host_u16
// (the two steps, then `sign as u16`) against the sequential loop of the host sketcher (skl_host::densify_bin).  Host compiler only.
//
//   finish_u16_check plan <num_bins>...   one line per size: num_bins lds_form threads_u16 lds_bytes_u16 threads lds_bytes workgroups(5000 streams)
//   finish_u16_check stream               reads u64 signs from stdin; writes flag (1 byte) and the u16 row to stdout; exit 1 if the
//                                         row differs from skl_host::densify_bin's signs cut to 16 bits (or an all-empty row is not zero)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../sketchlib.rust_amd/csrc/finish_plan.hpp"
#include "../../sketchlib.rust_amd/csrc/host/sketch.hpp"

using namespace skl;

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plan") {
        for (int a = 2; a < argc; ++a) {
            const uint64_t n = strtoull(argv[a], nullptr, 10);
            printf("%llu %d %u %llu %u %llu %llu\n", (unsigned long long)n, finish_lds_form(n) ? 1 : 0, finish_threads_u16(n),
                   (unsigned long long)finish_lds_bytes_u16(n), finish_threads(n), (unsigned long long)finish_lds_bytes(n),
                   (unsigned long long)finish_workgroups(5000, n));
        }
        return 0;
    }
    if (mode == "stream") {
        std::vector<uint64_t> v;
        uint64_t x;
        while (fread(&x, sizeof x, 1, stdin) == 1) v.push_back(x);
        std::vector<uint16_t> row(v.size(), 0xABCD);
        const uint8_t flag = finish_stream_host_u16(v.data(), v.size(), row.data());
        bool all_empty = true;
        for (uint64_t s : v) all_empty &= s == FINISH_EMPTY;
        if (all_empty != ((flag & FINISH_ALL_EMPTY) != 0)) return 1;
        if (all_empty) {   // (the sequential loop does not end on it)
            for (uint16_t r : row) if (r != 0) return 1;
        } else {
            std::vector<uint64_t> want = v;
            const bool densified = skl_host::densify_bin(want);
            if (flag != (densified ? FINISH_DENSIFIED : 0)) return 1;
            for (size_t i = 0; i < v.size(); ++i) if (row[i] != (uint16_t)want[i]) return 1;
        }
        fwrite(&flag, 1, 1, stdout);
        fwrite(row.data(), sizeof(uint16_t), row.size(), stdout);
        return 0;
    }
    fprintf(stderr, "usage: finish_u16_check plan|stream ...\n");
    return 2;
}
