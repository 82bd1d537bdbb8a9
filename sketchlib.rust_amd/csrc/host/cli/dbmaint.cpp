// dbmaint.cpp -- `sketchlib merge | delete | info` (src/cli.rs:240-322, src/lib.rs:454-483 and 793-947): file operations
// (host/dbmaint.cpp), no device context is made.  The three accept the global -v / --verbose / --quiet and ignore them.
#include "../dbmaint.hpp"

#include "common.hpp"

namespace skl_cli {

int run_merge(int argc, char **argv, int first, Verbosity &, const char *usage)
{
    std::vector<std::string> dbs;
    std::optional<std::string> output;
    ArgReader r(argc, argv, first, Syntax{/* --flag=value */ false, /* attached values */ "o"});
    Verbosity ignored;
    while (r.next()) {
        if (r.is_help()) {
            std::cout << "Merge two sketch files (.skm and .skd pair)\n\nUsage: " << usage << "\n\n"
                         "Arguments:\n  <DB1>  The first .skd (sketch data) file\n  <DB2>  The second .skd (sketch data) file\n\n"
                         "Options:\n  -o <OUTPUT>  Output filename for the merged sketch\n  -h, --help   Print help\n";
            throw HelpRequested{};
        }
        else if (ignored.accept(r)) continue;
        else if (r.is("-o")) output = r.value("-o <OUTPUT>");
        else if (r.is_option()) r.unexpected();
        else dbs.push_back(r.arg());
    }
    require({{dbs.size() >= 1, "<DB1>"}, {dbs.size() >= 2, "<DB2>"}});
    if (dbs.size() > 2) unexpected(dbs[2]);
    require({{output.has_value(), "-o <OUTPUT>"}});
    db_merge(dbs[0], dbs[1], *output);
    return 0;
}

int run_delete(int argc, char **argv, int first, Verbosity &, const char *usage)
{
    std::vector<std::string> pos;
    ArgReader r(argc, argv, first);
    Verbosity ignored;
    while (r.next()) {
        if (r.is_help()) {
            std::cout << "Delete genome(s) from a database (input: one id per line)\n\nUsage: " << usage << "\n\n"
                         "Arguments:\n  <DB>           Sketching database\n  <SAMPLES>      Input file with IDs to delete (one ID per line)\n"
                         "  <OUTPUT_FILE>  Output prefix of the database without them\n\nOptions:\n  -h, --help  Print help\n";
            throw HelpRequested{};
        }
        else if (ignored.accept(r)) continue;
        else if (r.is_option()) r.unexpected();
        else pos.push_back(r.arg());
    }
    require({{pos.size() >= 1, "<DB>"}, {pos.size() >= 2, "<SAMPLES>"}, {pos.size() >= 3, "<OUTPUT_FILE>"}});
    if (pos.size() > 3) unexpected(pos[3]);
    db_delete(pos[0], pos[1], pos[2]);
    return 0;
}

int run_info(int argc, char **argv, int first, Verbosity &, const char *usage)
{
    std::optional<std::string> file;
    bool sample_info = false;
    ArgReader r(argc, argv, first);
    Verbosity ignored;
    while (r.next()) {
        if (r.is_help()) {
            std::cout << "Print information about a .skm or .ski file\n\nUsage: " << usage << "\n\n"
                         "Arguments:\n  <SKM_FILE>  Sketch metadata file (.skm) or inverted index (.ski) to describe\n\n"
                         "Options:\n      --sample-info  Write out the information for every sample contained\n  -h, --help         Print help\n";
            throw HelpRequested{};
        }
        else if (ignored.accept(r)) continue;
        else if (r.is("--sample-info")) sample_info = true;
        else if (r.is_option() || file) r.unexpected();
        else file = r.arg();
    }
    require({{file.has_value(), "<SKM_FILE>"}});
    db_info(*file, sample_info, std::cout);
    std::cout.flush();
    return 0;
}

}  // namespace skl_cli
