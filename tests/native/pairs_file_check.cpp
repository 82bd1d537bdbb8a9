// pairs_file_check -- the pairs-file parser of `sketchlib dist --pairs` (csrc/host/pairs_file.cpp) and the listing writer
// (write_pair_list, csrc/host/distance_matrix.cpp) as a stand-alone host program: no GPU, no library.
//
//   pairs_file_check parse <pairs file> <names file> [<second names file>]
//       names files: one sample name per line.  Prints "ok <n>" and one "first<TAB>second" index line per pair, or
//       "error: <message>" on stderr with exit code 1.
//   pairs_file_check list <pairs file> <names file> <threads>
//       the listing of those pairs with the values (x / 4, x / 8) for entry x, through the block-parallel writer, on stdout.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "distance_matrix.hpp"
#include "pairs_file.hpp"

using namespace skl_host;

static std::vector<std::string> read_names(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error(std::string("Unable to open ") + path);
    std::vector<std::string> names;
    std::string line;
    while (std::getline(f, line)) names.push_back(line);
    return names;
}

int main(int argc, char **argv)
{
    if (argc < 4) {
        std::fprintf(stderr, "usage: pairs_file_check parse|list <pairs file> <names file> [<second names file> | <threads>]\n");
        return 2;
    }
    try {
        const std::vector<std::string> names = read_names(argv[3]);
        if (std::strcmp(argv[1], "parse") == 0) {
            PairsFile p;
            if (argc > 4) {
                const std::vector<std::string> second = read_names(argv[4]);
                p = read_pairs_file(argv[2], names, second, "query");
            } else {
                p = read_pairs_file(argv[2], names, names, "reference");
            }
            std::printf("ok %zu\n", p.size());
            for (size_t x = 0; x < p.size(); ++x) std::printf("%u\t%u\n", p.first[x], p.second[x]);
            return 0;
        }
        if (std::strcmp(argv[1], "list") == 0 && argc > 4) {
            const PairsFile p = read_pairs_file(argv[2], names, names, "reference");
            std::vector<float> dist(p.size() * 2);
            for (size_t x = 0; x < p.size(); ++x) {
                dist[2 * x] = (float)x / 4.0f;
                dist[2 * x + 1] = (float)x / 8.0f;
            }
            StreamSink sink(std::cout);
            write_pair_list(sink, names, names, p.first.data(), p.second.data(), p.size(), dist.data(), 2, (size_t)std::atoi(argv[4]));
            std::cout.flush();
            return 0;
        }
        std::fprintf(stderr, "unknown mode %s\n", argv[1]);
        return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
