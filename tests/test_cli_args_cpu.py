"""csrc/host/cli/args.hpp on the CPU: the CLI's one argument reader and its value readers, driven over the edges of their
input by tests/native/cli_args_check.cpp -- a program of its own that includes nothing else of the project, built with the
host compiler under AddressSanitizer and UBSan and run directly.  The outcomes below are the rules of the command loops the
reader replaced (clap's messages, strtoull's reading of a number), written down case by case."""
import functools
import os
import subprocess
import tempfile

from conftest import ROOT

_DIR = tempfile.TemporaryDirectory(prefix="cli_args_check_")
CLI_DIR = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "host", "cli")

DIGIT = "invalid digit found in string"
EXPECTED = r"""
reader/empty	ok
reader/words	ok [a word][- word][-x option][--y option][ word]
reader/flag-last	usage: a value is required for '--knn <V>' but none was supplied
reader/value-detached	ok [-o option = 'file'][b word]
reader/value-is-a-flag	ok [-o option = '--knn'][b word]
reader/equals-empty	ok [--x option = '']
reader/equals-value	ok [--x option = 'a=b'][c word]
reader/equals-on-a-switch	ok [--x option]
reader/equals-off	ok [--x=a option]
reader/equals-short	ok [-x=a option]
reader/attached	ok [-o option = 'file'][b word]
reader/attached-detached	ok [-o option = 'file'][b word]
reader/attached-last	usage: a value is required for '-o <V>' but none was supplied
reader/attached-other-letter	ok [-kx option]
reader/attached-off	ok [-ofile option]
reader/attached-long	ok [--ofile option]
reader/dist-syntax	ok [-k option = '21'][-o option = 'file'][--knn option = '5'][-k option = '31'][--knn option = '6'][-k option = '=']
reader/help	help
reader/help-short	help
reader/unexpected	usage: unexpected argument '--frob' found
usize/0	ok 0
usize/7	ok 7
usize/9999999999999999999	ok 9999999999999999999
usize/18446744073709551615	ok 18446744073709551615
usize/18446744073709551616	ok 18446744073709551615
usize/999999999999999999999	ok 18446744073709551615
usize/	usage: invalid value '' for '--knn <KNN>': DIGIT
usize/-1	usage: invalid value '-1' for '--knn <KNN>': DIGIT
usize/-	usage: invalid value '-' for '--knn <KNN>': DIGIT
usize/+1	ok 1
usize/ 1	ok 1
usize/1 	usage: invalid value '1 ' for '--knn <KNN>': DIGIT
usize/1x	usage: invalid value '1x' for '--knn <KNN>': DIGIT
usize/x	usage: invalid value 'x' for '--knn <KNN>': DIGIT
usize/3.5	usage: invalid value '3.5' for '--knn <KNN>': DIGIT
usize/0x10	usage: invalid value '0x10' for '--knn <KNN>': DIGIT
bounded-u16/0	ok 0
bounded-u16/65535	ok 65535
bounded-u16/65536	usage: invalid value '65536' for '--min-count <MIN_COUNT>': 65536 is not in 0..=65535
bounded-u16/00000000000000000001	ok 1
bounded-u16/000000000000000000001	usage: invalid value '000000000000000000001' for '--min-count <MIN_COUNT>': 000000000000000000001 is not in 0..=65535
bounded-u16/18446744073709551615	usage: invalid value '18446744073709551615' for '--min-count <MIN_COUNT>': 18446744073709551615 is not in 0..=65535
bounded-u16/18446744073709551616	usage: invalid value '18446744073709551616' for '--min-count <MIN_COUNT>': 18446744073709551616 is not in 0..=65535
bounded-u16/-1	usage: invalid value '-1' for '--min-count <MIN_COUNT>': DIGIT
bounded-u16/x	usage: invalid value 'x' for '--min-count <MIN_COUNT>': DIGIT
bounded-u16/	usage: invalid value '' for '--min-count <MIN_COUNT>': DIGIT
bounded-u8/255	ok 255
bounded-u8/256	usage: invalid value '256' for '--min-qual <MIN_QUAL>': 256 is not in 0..=255
bounded-top/0	usage: invalid value '0' for '--top <N>': 0 is not in 1..=1024
bounded-top/1	ok 1
bounded-top/1024	ok 1024
bounded-top/1025	usage: invalid value '1025' for '--top <N>': 1025 is not in 1..=1024
bounded-top/99999999999999999999999	usage: invalid value '99999999999999999999999' for '--top <N>': 99999999999999999999999 is not in 1..=1024
list/7	ok 7
list/1,2,3	ok 1 2 3
list/17,31,4	ok 17 31 4
list/1,,2	usage: invalid value '' for '--k-vals <K_VALS>': DIGIT
list/	usage: invalid value '' for '--k-vals <K_VALS>': DIGIT
list/,	usage: invalid value '' for '--k-vals <K_VALS>': DIGIT
list/1,	usage: invalid value '' for '--k-vals <K_VALS>': DIGIT
list/,1	usage: invalid value '' for '--k-vals <K_VALS>': DIGIT
list/1,x	usage: invalid value 'x' for '--k-vals <K_VALS>': DIGIT
list/1,-2	usage: invalid value '-2' for '--k-vals <K_VALS>': DIGIT
list/18446744073709551616,0	ok 18446744073709551615 0
threads-strict/1	ok 1
threads-lenient/1	ok 1
threads-strict/4	ok 4
threads-lenient/4	ok 4
threads-strict/0	usage: invalid value '0' for '--threads <THREADS>': Threads must be one or higher
threads-lenient/0	ok 1
threads-strict/-2	usage: invalid value '-2' for '--threads <THREADS>': Threads must be one or higher
threads-lenient/-2	usage: invalid value '-2' for '--threads <THREADS>': DIGIT
threads-strict/x	usage: invalid value 'x' for '--threads <THREADS>': `x` isn't a valid number of cores
threads-lenient/x	usage: invalid value 'x' for '--threads <THREADS>': DIGIT
threads-strict/	usage: invalid value '' for '--threads <THREADS>': `` isn't a valid number of cores
threads-lenient/	usage: invalid value '' for '--threads <THREADS>': DIGIT
threads-strict/1x	usage: invalid value '1x' for '--threads <THREADS>': `1x` isn't a valid number of cores
threads-lenient/1x	usage: invalid value '1x' for '--threads <THREADS>': DIGIT
threads-strict/+3	ok 3
threads-lenient/+3	ok 3
threads-strict/99999999999999999999999	ok 9223372036854775807
threads-lenient/99999999999999999999999	ok 18446744073709551615
float/0.5	ok 0.5
float/1e-3	ok 0.001
float/1	ok 1
float/-0.25	ok -0.25
float/x	usage: invalid value 'x' for '--completeness-cutoff <COMPLETENESS_CUTOFF>': invalid float literal
float/	usage: invalid value '' for '--completeness-cutoff <COMPLETENESS_CUTOFF>': invalid float literal
float/0.5x	usage: invalid value '0.5x' for '--completeness-cutoff <COMPLETENESS_CUTOFF>': invalid float literal
float/inf	ok inf
choice-inline/canonical	ok 0
choice-inline/reference	ok 1
choice-inline/Canonical	usage: invalid value 'Canonical' for '--knn-ties <RULE>': possible values: canonical, reference
choice-inline/	usage: invalid value '' for '--knn-ties <RULE>': possible values: canonical, reference
choice-block/match-count	ok 0
choice-block/any-bins	ok 2
choice-block/some-bins	usage: invalid value 'some-bins' for '--query-type <QUERY_TYPE>'\n  [possible values: match-count, all-bins, any-bins]
choice-block/	usage: invalid value '' for '--query-type <QUERY_TYPE>'\n  [possible values: match-count, all-bins, any-bins]
choice/one	usage: invalid value 'b' for '--x <X>': possible values: a
require/all-given	ok
require/second	usage: the following required arguments were not provided:\n  <DB2>
require/all-three	usage: the following required arguments were not provided:\n  <DB>\n  <SAMPLES>\n  <OUTPUT_FILE>
require/none-listed	ok
conflict	usage: the argument '--pairs <FILE>' cannot be used with '--knn <KNN>'
knn-ties/canonical	ok 1
knn-ties/reference	ok 0
knn-ties/x	usage: invalid value 'x' for '--knn-ties <RULE>': possible values: canonical, reference
knn-ties/--knn-ties	usage: a value is required for '--knn-ties <RULE>' but none was supplied
knn-ties/--knn-ties=canonical	ok 1
level/level1	ok 1
level/level2	ok 2
level/level3	ok 3
level/level4	usage: invalid value 'level4' for '--level <LEVEL>'\n  [possible values: level1, level2, level3]
level/3	usage: invalid value '3' for '--level <LEVEL>'\n  [possible values: level1, level2, level3]
level/none	usage: a value is required for '--level' but none was supplied
inputs/neither	usage: exactly one of <SEQ_FILES>... or -f <FILE_LIST> must be given
inputs/files	ok files=2 list=- min_count=5 min_qual=20 threads=1 single_strand=0 sketch_device=-1 gpu=0 device=0
inputs/list	ok files=0 list=rfile.txt min_count=5 min_qual=20 threads=1 single_strand=0 sketch_device=-1 gpu=0 device=0
inputs/both	usage: exactly one of <SEQ_FILES>... or -f <FILE_LIST> must be given
inputs/all-options	ok files=1 list=- min_count=65535 min_qual=255 threads=1 single_strand=1 sketch_device=-1 gpu=0 device=0
inputs/gpu-then-device	ok files=1 list=- min_count=5 min_qual=20 threads=1 single_strand=0 sketch_device=2 gpu=1 device=2
inputs/device-then-gpu	ok files=1 list=- min_count=5 min_qual=20 threads=1 single_strand=0 sketch_device=0 gpu=1 device=2
inputs/device-alone	ok files=1 list=- min_count=5 min_qual=20 threads=1 single_strand=0 sketch_device=3 gpu=0 device=3
inputs/no-single-strand	usage: unexpected argument '--single-strand' found
inputs/min-count-over	usage: invalid value '65536' for '--min-count <MIN_COUNT>': 65536 is not in 0..=65535
inputs/min-qual-over	usage: invalid value '256' for '--min-qual <MIN_QUAL>': 256 is not in 0..=255
inputs/value-missing-f	usage: a value is required for '-f <FILE_LIST>' but none was supplied
inputs/value-missing-device	usage: a value is required for '--device' but none was supplied
inputs/unknown	usage: unexpected argument '--k-vals' found
"""


@functools.lru_cache(maxsize=None)
def outcomes():
    exe = os.path.join(_DIR.name, "cli_args_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CLI_DIR, os.path.join(ROOT, "tests", "native", "cli_args_check.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stderr == "", res.stderr          # no sanitizer report
    out = {}
    for line in res.stdout.splitlines():
        name, outcome = line.split("\t")
        assert name not in out, name
        out[name] = outcome.rstrip()
    return out


def expected():
    want = {}
    for line in EXPECTED.strip("\n").splitlines():
        name, outcome = line.split("\t")
        want[name] = outcome.replace("DIGIT", DIGIT).rstrip()
    return want


def test_args_hpp_includes_nothing_of_the_project():
    """Header only, on the standard library alone: the check program's single include path is host/cli/ itself."""
    src = open(os.path.join(CLI_DIR, "args.hpp")).read()
    assert '#include "' not in src
    check = open(os.path.join(ROOT, "tests", "native", "cli_args_check.cpp")).read()
    assert [line for line in check.splitlines() if line.startswith('#include "')] == ['#include "args.hpp"']


def test_every_case_has_its_outcome():
    got, want = outcomes(), expected()
    assert sorted(got) == sorted(want)
    wrong = {name: (got[name], want[name]) for name in want if got[name] != want[name]}
    assert not wrong, wrong


def test_the_cases_the_reader_must_survive_are_there():
    """Empty argv, a flag as the last element, --x= with an empty value, -o attached and detached, an empty list element,
    numbers of 0 / 19 / 20 / 21 digits, 2^64 - 1 and 2^64, and the four combinations of files and -f."""
    got = outcomes()
    for name in ("reader/empty", "reader/flag-last", "reader/equals-empty", "reader/attached", "reader/attached-detached", "list/1,,2",
                 "usize/", "usize/9999999999999999999", "usize/18446744073709551615", "usize/18446744073709551616",
                 "usize/999999999999999999999", "bounded-u16/00000000000000000001", "bounded-u16/000000000000000000001",
                 "inputs/neither", "inputs/files", "inputs/list", "inputs/both"):
        assert name in got, name
