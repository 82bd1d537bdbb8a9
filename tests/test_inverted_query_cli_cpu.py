"""`sketchlib inverted query` without a GPU: argument errors exit 2 with the clap-style message that
`inverted build` and `precluster` print (src/cli.rs:380-412), a missing .ski is `Error:` and exit 1, and
an index the query cannot take -- not DNA, or not exactly one value per (sample, bin) -- is refused with
its own message, never with the device error of this GPU-less host."""
import os
import shutil
import subprocess

import msgpack
import pytest

from conftest import REF_FIXTURES, ROOT
from helpers import FIXTURE_NAMES
from test_fileformat_cpu import _py_frame
from test_inverted_cli_cpu import FIELDS, ski_decode

CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")
USAGE = "Usage: sketchlib inverted query [OPTIONS] <SKI> <SEQ_FILES|-f <FILE_LIST>>"


@pytest.fixture(scope="module", autouse=True)
def _built(skl):
    assert os.path.exists(CLI)


@pytest.fixture(scope="module")
def wd(tmp_path_factory):
    d = tmp_path_factory.mktemp("invq")
    for f in FIXTURE_NAMES + ["rfile.txt"]:
        shutil.copy(os.path.join(REF_FIXTURES, f), d / f)
    res = subprocess.run([CLI, "inverted", "build", "-k", "21", "-s", "10", "-f", "rfile.txt", "-o", "inverted"],
                         cwd=d, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return d


def run(wd, *args):
    return subprocess.run([CLI, "inverted", "query", *args], cwd=wd, capture_output=True, text=True)


def usage_error(res, message):
    assert res.returncode == 2, res.stderr
    assert res.stdout == ""
    assert res.stderr.startswith(f"error: {message}\n"), res.stderr
    assert USAGE in res.stderr


def test_unknown_query_type(wd):
    res = run(wd, "-f", "rfile.txt", "inverted.ski", "--query-type", "some-bins")
    usage_error(res, "invalid value 'some-bins' for '--query-type <QUERY_TYPE>'\n"
                     "  [possible values: match-count, all-bins, any-bins]")


def test_query_type_needs_a_value(wd):
    usage_error(run(wd, "-f", "rfile.txt", "inverted.ski", "--query-type"),
                "a value is required for '--query-type <QUERY_TYPE>' but none was supplied")


@pytest.mark.parametrize("args", [["inverted.ski"], ["-f", "rfile.txt", "inverted.ski", "R6.fa.gz"]],
                         ids=["neither", "both"])
def test_exactly_one_input_form(wd, args):
    usage_error(run(wd, *args), "exactly one of <SEQ_FILES>... or -f <FILE_LIST> must be given")


def test_ski_is_required(wd):
    usage_error(run(wd), "the following required arguments were not provided:\n  <SKI>")


def test_unknown_flag(wd):
    usage_error(run(wd, "-f", "rfile.txt", "inverted.ski", "--kmer", "21"), "unexpected argument '--kmer' found")


def test_missing_ski_is_an_error(wd):
    res = run(wd, "-f", "rfile.txt", "missing.ski")
    assert res.returncode == 1 and res.stdout == ""
    assert res.stderr == "Error: Could not open missing.ski\n"


def test_unknown_subcommand_lists_query(wd):
    res = subprocess.run([CLI, "inverted", "search"], cwd=wd, capture_output=True, text=True)
    assert res.returncode == 2
    assert "unrecognized subcommand 'inverted search'" in res.stderr and "`inverted query`" in res.stderr
    top = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert top.returncode == 0 and "inverted build|query|precluster" in top.stdout


def _rewrite(wd, name, change):
    ski = ski_decode(wd / "inverted.ski")
    change(ski)
    (wd / f"{name}.ski").write_bytes(_py_frame(msgpack.packb([ski[f] for f in FIELDS], use_bin_type=True)))


def test_non_dna_index_is_refused_before_the_device(wd):
    _rewrite(wd, "aa", lambda ski: ski.update(hash_type={"AA": "Level1"}))
    res = run(wd, "-f", "rfile.txt", "aa.ski")
    assert res.returncode == 2 and res.stdout == ""
    assert res.stderr == "error: this build queries DNA indices only (aa.ski has hash_type AA(Level1))\n"


def test_bin_missing_a_sample_is_refused(wd):
    def drop(ski):
        first = sorted(ski["index"][3])[0]
        del ski["index"][3][first]
    _rewrite(wd, "gap", drop)
    res = run(wd, "-f", "rfile.txt", "gap.ski")
    assert res.returncode == 1 and res.stdout == ""
    assert res.stderr.startswith("Error: gap.ski: bin 3 holds ") and "one value per sample and bin" in res.stderr
    assert "HIP" not in res.stderr


def test_two_values_for_one_sample_are_refused(wd):
    def dup(ski):
        values = sorted(ski["index"][0])
        spare = next(v for v in range(65536) if v not in ski["index"][0])
        ski["index"][0][spare] = ski["index"][0][values[0]]
    _rewrite(wd, "dup", dup)
    res = run(wd, "-f", "rfile.txt", "dup.ski")
    assert res.returncode == 1 and res.stdout == ""
    assert res.stderr.startswith("Error: dup.ski: sample ") and "more than one value at bin 0" in res.stderr
