"""Read sets in `sketchlib inverted build` / `inverted query` on the CPU path (host/sketch.cpp sketch_sample_inverted): a FASTQ
sample goes through the k-mer count filter in stream order over exactly `sketch_size` bins, is densified and cut to u16
(inverted.rs:303-395).  The expectation is a Python restatement from tests/reads_reference.py's Packed / NtHash / KmerFilter /
densify with num_bins = sketch_size, never the code under test.  Assemblies still give the reference's `.skq`."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import reads_reference as R
from conftest import REF_FIXTURES, ROOT
from helpers import FIXTURE_NAMES

CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")
READS = ["test_1_fwd.fastq.gz", "test_1_rev.fastq.gz", "test_2_fwd.fastq.gz", "test_2_rev.fastq.gz"]
PAIRS = {"test_1": READS[:2], "test_2": READS[2:]}
K, MIN_QUAL = 9, 2


@pytest.fixture(scope="module", autouse=True)
def _built(skl):
    assert os.path.exists(CLI)


@pytest.fixture()
def wd(tmp_path):
    for f in FIXTURE_NAMES + ["rfile.txt", "short_sequence.fa"] + READS:
        shutil.copy(os.path.join(REF_FIXTURES, f), tmp_path / f)
    (tmp_path / "reads.txt").write_text("".join(f"{name}\t" + "\t".join(files) + "\n" for name, files in PAIRS.items()))
    return tmp_path


def run(wd, *args, ok=True):
    res = subprocess.run([CLI, *args], cwd=wd, capture_output=True, text=True, timeout=600)
    if ok:
        assert res.returncode == 0, res.stderr
    return res


@functools.lru_cache(maxsize=None)
def stream_signs(name):
    """Every valid window's sign of a read pair in stream order (the slow part: once per pair)."""
    p = R.Packed([os.path.join(REF_FIXTURES, f) for f in PAIRS[name]], MIN_QUAL)
    assert p.reads
    return [h % R.SIGN_MOD for h in R.NtHash(p, K, True)]


@functools.lru_cache(maxsize=None)
def expected_row(name, sketch_size, min_count):
    """Sketch::get_signs_no_densify over `sketch_size` bins with the count filter, densify_bin, `as u16`."""
    bin_size = (R.SIGN_MOD + sketch_size - 1) // sketch_size
    filt = R.KmerFilter(min_count)
    signs = [R.M64] * sketch_size
    for sign in stream_signs(name):
        b = sign // bin_size
        if sign < signs[b] and filt.equal(sign):
            signs[b] = sign
    assert min(signs) != R.M64
    R.densify(signs)
    return np.array([s & 0xFFFF for s in signs], dtype="<u2")


def build_reads(wd, out, sketch_size, min_count, *extra):
    run(wd, "inverted", "build", "-o", out, "-k", str(K), "-s", str(sketch_size), "--min-count", str(min_count), "--min-qual", str(MIN_QUAL),
        "--write-skq", "-f", "reads.txt", *extra)
    return np.fromfile(wd / f"{out}.skq", dtype="<u2").reshape(len(PAIRS), sketch_size)


@pytest.mark.parametrize("sketch_size", [10, 1000])
def test_read_pairs_equal_the_python_restatement(wd, sketch_size):
    skq = build_reads(wd, "reads", sketch_size, 2)
    for row, name in zip(skq, PAIRS):
        assert np.array_equal(row, expected_row(name, sketch_size, 2)), name
    assert (wd / "reads.ski").stat().st_size > 0


def test_min_count_is_no_longer_ignored(wd):
    one, two = build_reads(wd, "c1", 1000, 1), build_reads(wd, "c2", 1000, 2)
    assert not np.array_equal(one, two)
    for row, name in zip(one, PAIRS):
        assert np.array_equal(row, expected_row(name, 1000, 1)), name


def test_min_count_and_min_qual_are_parsed_with_the_bounds_of_sketch(wd):
    for flag, value in (("--min-count", "65536"), ("--min-qual", "256"), ("--min-count", "x")):
        res = run(wd, "inverted", "build", "-o", "bad", "-k", str(K), "-s", "10", flag, value, "-f", "reads.txt", ok=False)
        ref = run(wd, "sketch", "-o", "bad", "-k", str(K), "-s", "10", flag, value, "-f", "reads.txt", ok=False)
        assert res.returncode == ref.returncode == 2, (flag, value, res.stderr)
        assert res.stderr.splitlines()[0] == ref.stderr.splitlines()[0]


def test_min_count_nobody_reaches_gives_the_message_of_sketch(wd):
    res = run(wd, "inverted", "build", "-o", "none", "-k", str(K), "-s", "10", "--min-count", "60000", "--min-qual", str(MIN_QUAL), "-f", "reads.txt", ok=False)
    assert res.returncode != 0 and "reached --min-count 60000 at k=9" in res.stderr


def test_read_set_query_prints_numpy_counts(wd, skl):
    """The index holds both pairs; the query is test_1.  `inverted query` matches on the device: without one the command must get
    past the sketching (no "FASTQ input is not supported") and stop at the device with the "no CPU path" refusal."""
    index = build_reads(wd, "idx", 1000, 2)
    args = ("inverted", "query", "idx.ski", "--min-count", "2", "--min-qual", str(MIN_QUAL), "test_1_fwd.fastq.gz", "test_1_rev.fastq.gz")
    if skl.device_count() == 0:
        res = run(wd, *args, ok=False)
        assert res.returncode != 0 and "no CPU path" in res.stderr and "not supported" not in res.stderr
        return
    (wd / "q.txt").write_text("q\ttest_1_fwd.fastq.gz\ttest_1_rev.fastq.gz\n")
    out = run(wd, "inverted", "query", "idx.ski", "--min-count", "2", "--min-qual", str(MIN_QUAL), "-f", "q.txt").stdout
    query = expected_row("test_1", 1000, 2)
    counts = [(index[s] == query).sum() for s in range(2)]
    assert counts[0] == 1000
    assert out == "Query\ttest_1\ttest_2\nq\t" + "\t".join(map(str, counts)) + "\n"


def test_assemblies_still_give_the_reference_skq(wd):
    run(wd, "inverted", "build", "-o", "inverted", "-k", "21", "-s", "10", "-f", "rfile.txt", "--write-skq", "--min-count", "3", "--min-qual", "7")
    assert (wd / "inverted.skq").read_bytes() == open(os.path.join(REF_FIXTURES, "inverted.skq"), "rb").read()


def test_gpu_flag_refuses_without_a_device(wd, skl):
    """No silent fallback to the host loop: --gpu without a device is the "no CPU path" refusal of `sketch --gpu`, not a usage error."""
    if skl.device_count() > 0:
        pytest.skip("a GPU is present; the refusal path is only reachable without one")
    run(wd, "inverted", "build", "-o", "inverted", "-k", "21", "-s", "10", "-f", "rfile.txt")
    for args in (("inverted", "build", "--gpu", "-o", "x", "-k", "21", "-s", "10", "-f", "rfile.txt"),
                 ("inverted", "build", "--device", "0", "-o", "x", "-k", "21", "-s", "10", "-f", "rfile.txt"),
                 ("inverted", "query", "--gpu", "inverted.ski", "-f", "rfile.txt")):
        res = run(wd, *args, ok=False)
        assert res.returncode not in (0, 2) and "no CPU path" in res.stderr, (args, res.stderr)
        assert "Usage:" not in res.stderr
    assert not (wd / "x.ski").exists()
