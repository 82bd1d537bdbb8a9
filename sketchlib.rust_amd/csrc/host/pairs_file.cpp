#include "pairs_file.hpp"

#include <fstream>
#include <istream>
#include <stdexcept>
#include <string_view>
#include <unordered_map>

namespace skl_host {

namespace {
using Lookup = std::unordered_map<std::string_view, uint32_t>;

Lookup make_lookup(const std::vector<std::string> &names)
{
    Lookup m;
    m.reserve(names.size() * 2);
    for (size_t i = 0; i < names.size(); ++i) m.emplace(std::string_view(names[i]), (uint32_t)i);   // (the first of equal names stays)
    return m;
}

// what an error message shows of a name from the file: at most 200 bytes, control characters as '?'
std::string shown(std::string_view name)
{
    std::string s(name.substr(0, 200));
    for (char &ch : s) {
        if ((unsigned char)ch < 0x20 || ch == 0x7f) ch = '?';
    }
    if (name.size() > 200) s += "...";
    return s;
}
}  // namespace

PairsFile parse_pairs(std::istream &in, const std::string &label, const std::vector<std::string> &first_names,
                      const std::vector<std::string> &second_names, const char *second_what)
{
    if (first_names.size() > 0xFFFFFFFFull || second_names.size() > 0xFFFFFFFFull) throw std::runtime_error("too many samples for a pairs file");
    const Lookup first = make_lookup(first_names);
    const bool same = &first_names == &second_names;
    const Lookup second_own = same ? Lookup() : make_lookup(second_names);
    const Lookup &second = same ? first : second_own;
    PairsFile out;
    std::string line;
    size_t line_no = 0;
    while (std::getline(in, line)) {
        ++line_no;
        std::string_view v(line);
        if (!v.empty() && v.back() == '\r') v.remove_suffix(1);
        if (v.empty()) continue;
        const std::string where = label + ": line " + std::to_string(line_no) + ": ";
        const size_t tab1 = v.find('\t');
        if (tab1 == std::string_view::npos) throw std::runtime_error(where + "expected two tab-separated sample names");
        const size_t tab2 = v.find('\t', tab1 + 1);
        const std::string_view name1 = v.substr(0, tab1);
        const std::string_view name2 = v.substr(tab1 + 1, tab2 == std::string_view::npos ? std::string_view::npos : tab2 - tab1 - 1);
        if (name1.empty() || name2.empty()) throw std::runtime_error(where + "expected two tab-separated sample names");
        const auto it1 = first.find(name1);
        if (it1 == first.end()) throw std::runtime_error(where + "sample \"" + shown(name1) + "\" is not in the reference database");
        const auto it2 = second.find(name2);
        if (it2 == second.end()) throw std::runtime_error(where + "sample \"" + shown(name2) + "\" is not in the " + second_what + " database");
        out.first.push_back(it1->second);
        out.second.push_back(it2->second);
    }
    if (in.bad()) throw std::runtime_error(label + ": read error");
    return out;
}

PairsFile read_pairs_file(const std::string &path, const std::vector<std::string> &first_names,
                          const std::vector<std::string> &second_names, const char *second_what)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("Unable to open " + path);
    return parse_pairs(f, path, first_names, second_names, second_what);
}

}  // namespace skl_host
