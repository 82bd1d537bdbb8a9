// main.cpp -- `sketchlib <command>`: the global flags, the top-level help, the table of commands and the one guarded call
// that turns what a command throws into the reference's exit behaviour (usage -> 2, panic -> 101, error -> 1).
#include <cstring>

#include "common.hpp"

using namespace skl_cli;

namespace {

const char *const DIST_USAGE = "sketchlib dist [OPTIONS] <REF_DB> [QUERY_DB]";

// `inverted` alone, or with a word that is none of its subcommands (--help among them)
int run_inverted_unknown(int argc, char **argv, int first, Verbosity &, const char *)
{
    if (first >= argc) throw UsageError{"'sketchlib inverted' requires a subcommand: build | query | precluster"};
    std::cerr << "error: unrecognized subcommand 'inverted " << argv[first] << "' (this build provides `inverted build`, `inverted query` and `inverted precluster`)\n";
    return 2;
}

struct CommandEntry {
    const char *name, *sub;    // `name` or `name sub`; sub == nullptr after the entries with one: any other word, or none
    const char *usage;         // the line a usage error is reported under
    Command run;
    bool complete_in;          // a returned exit code is followed by the verbose "Complete in" line (lib.rs:949-957)
    bool leaves_fast;          // leaves through leave_after_success
    bool flushes_for_panic;    // stdout is flushed before a panic message
};

const CommandEntry COMMANDS[] = {
    {"dist", nullptr, DIST_USAGE, run_dist, true, true, false},
    {"sketch", nullptr, "sketchlib sketch [OPTIONS] -o <OUTPUT> <--k-vals <K_VALS>|--k-seq <K_SEQ>> <SEQ_FILES|-f <FILE_LIST>>", run_sketch, false, false, false},
    {"merge", nullptr, "sketchlib merge -o <OUTPUT> <DB1> <DB2>", run_merge, false, false, true},
    {"append", nullptr, "sketchlib append [OPTIONS] -o <OUTPUT> <DB> <SEQ_FILES|-f <FILE_LIST>>", run_append, false, false, true},
    {"delete", nullptr, "sketchlib delete <DB> <SAMPLES> <OUTPUT_FILE>", run_delete, false, false, true},
    {"info", nullptr, "sketchlib info [OPTIONS] <SKM_FILE>", run_info, false, false, true},
    {"inverted", "build", "sketchlib inverted build [OPTIONS] -o <OUTPUT> <SEQ_FILES|-f <FILE_LIST>>", run_inverted_build, true, true, false},
    {"inverted", "query", "sketchlib inverted query [OPTIONS] <SKI> <SEQ_FILES|-f <FILE_LIST>>", run_inverted_query, true, true, false},
    {"inverted", "precluster", "sketchlib inverted precluster [OPTIONS] <SKI> <--skd <SKD>|--count>", run_inverted_precluster, true, true, false},
    {"inverted", nullptr, DIST_USAGE, run_inverted_unknown, true, true, false},
};

int guarded(const CommandEntry &cmd, int argc, char **argv, int first, Verbosity verbosity, std::chrono::steady_clock::time_point start)
{
    try {
        const int rc = cmd.run(argc, argv, first, verbosity, cmd.usage);
        if (cmd.complete_in && verbosity.info()) {
            const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
            std::cerr << "INFO  [sketchlib] Complete in " << s << "s\n";
        }
        return cmd.leaves_fast ? leave_after_success(rc) : rc;
    } catch (const UsageError &u) {
        std::cerr << "error: " << u.message << "\n\n"
                  << "Usage: " << cmd.usage << "\n\n"
                  << "For more information, try '--help'.\n";
        return 2;
    } catch (const HelpRequested &) {
        return 0;
    } catch (const Panic &p) {
        if (cmd.flushes_for_panic) std::cout.flush();
        std::cerr << "thread 'main' panicked:\n" << p.what() << "\n";
        return 101;
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << "\n";
        return 1;
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const auto start = std::chrono::steady_clock::now();
    // global flags may precede the command
    Verbosity verbosity;
    int sub = 1;
    for (ArgReader r(argc, argv, 1); r.next() && verbosity.accept(r);) ++sub;
    if (sub >= argc || strcmp(argv[sub], "-h") == 0 || strcmp(argv[sub], "--help") == 0) {
        std::cout << "Usage: sketchlib [OPTIONS] <COMMAND>\n\nCommands:\n"
                     "  sketch  Create sketches from input data (DNA assemblies and read sets, amino-acid sequences; CPU, or GPU with --gpu)\n"
                     "  dist    Calculate pairwise distances using sketches (GPU)\n"
                     "  inverted build|query|precluster  Inverted index of single-k sketches of DNA assemblies and read sets (CPU, or GPU\n"
                     "                                   with --gpu); match queries against it (GPU; --gpu sketches the queries there too);\n"
                     "                                   kNN restricted to its candidates (GPU)\n"
                     "  merge   Merge two sketch databases (.skm and .skd pair) into a new one (files only)\n"
                     "  append  Sketch new samples the way a database was sketched and write both as a new database, the new\n"
                     "          samples first (CPU, or GPU with --gpu)\n"
                     "  delete  Write a database without the samples listed in a file (files only)\n"
                     "  info    Print information about a .skm or .ski file (files only)\n";
        return sub >= argc ? 2 : 0;
    }
    for (const CommandEntry &cmd : COMMANDS) {
        if (strcmp(argv[sub], cmd.name) != 0) continue;
        if (!cmd.sub) return guarded(cmd, argc, argv, sub + 1, verbosity, start);
        if (sub + 1 < argc && strcmp(argv[sub + 1], cmd.sub) == 0) return guarded(cmd, argc, argv, sub + 2, verbosity, start);
    }
    std::cerr << "error: unrecognized subcommand '" << argv[sub]
              << "' (this build provides `sketch` (DNA assemblies and read sets), `dist` (GPU) and `inverted build|query|precluster`"
                 ", and the database commands `merge`, `append`, `delete` and `info`)\n";
    return 2;
}
