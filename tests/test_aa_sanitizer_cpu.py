"""The amino-acid sketcher's host code (csrc/host/aahash.cpp with the host layer it uses) and the work plan of its GPU call
(csrc/aa_plan.hpp) under AddressSanitizer and UndefinedBehaviorSanitizer: tests/native/aa_check.cpp, a program with a main() of
its own, compiled with -fsanitize=address,undefined and run on the CPU over the reference's fixture and the edge records of
tests/test_sketch_aa_cpu.py.  Any report ends the program with a non-zero status (-fno-sanitize-recover)."""
import os
import subprocess

import pytest

import aa_native
from conftest import REF_FIXTURES

FIXTURE = os.path.join(REF_FIXTURES, "test_aa_sequence.fa")


@pytest.fixture(scope="module")
def check():
    return aa_native.build(sanitize=True)


def run(check, *args):
    return subprocess.run([check, *map(str, args)], capture_output=True, text=True)


def clean(res):
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    return res


def test_fixture_and_edge_records(check, tmp_path):
    edge = tmp_path / "edge.fa"
    edge.write_text(">a\nMKV*ACD\n>b\nMKVA\n>c\nacdefgBJOUXZ*-ACDEFG\n>d\nMK*ACDE\n>e\n" + "ACDEFGHIKLMNPQRSTVWY" * 20 + "\n")
    for level in (1, 2, 3):
        for concat in (0, 1):
            res = clean(run(check, "sketch", tmp_path / f"f{level}{concat}", level, concat, 1000, "9", FIXTURE))
            assert res.returncode == 0 and res.stdout.startswith("ok 1"), res.stderr
            res = clean(run(check, "sketch", tmp_path / f"e{level}{concat}", level, concat, 64, "3,4", FIXTURE, edge))
            # with --concat-fasta the record MKV*ACD has no seedable window of 4: the reference's panic, reported as an error
            assert (res.returncode, res.stdout[:2]) == ((3, "") if concat else (0, "ok")), res.stderr
    for k in (1, 2, 3, 31, 33, 64, 66, 400, 401):
        for concat in (0, 1):
            assert clean(run(check, "signs", 2, k, 128, concat, edge, FIXTURE)).returncode == 0
    # the errors: FASTQ input, an empty record as a sample, a missing file
    res = clean(run(check, "signs", 1, 5, 64, 0, os.path.join(REF_FIXTURES, "test_1_fwd.fastq.gz")))
    assert res.returncode == 3 and "Unexpected quality information" in res.stderr
    empty = tmp_path / "empty.fa"
    empty.write_text(">a\n>b\nMKVLA\n")
    res = clean(run(check, "sketch", tmp_path / "x", 1, 1, 64, "3", empty))
    assert res.returncode == 3 and "has no valid sequence" in res.stderr
    assert clean(run(check, "signs", 1, 5, 64, 0, tmp_path / "missing.fa")).returncode == 3


def test_plan(check):
    for k, long_min in ((7, 8192), (7, 1), (300, 8192)):
        res = clean(run(check, "plan", k, long_min, 0, 1, 6, 7, 8, 63, 64, 65, 16383, 16384, 16385, 100000, 5, 70))
        assert res.returncode == 0 and res.stdout.startswith("ok "), res.stderr
