"""`sketchlib append --gpu`: the new samples sketched on the device give the files the host path writes, byte for byte, for
the three kinds of input `sketch --gpu` takes (assemblies, amino acids under --concat-fasta, a read pair); and `dist` on a
database `delete` renumbered prints what it prints on the database sketched from the kept samples."""
import os
import subprocess

import pytest

from conftest import REF_FIXTURES, ROOT
from helpers import FIXTURE_NAMES

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")
PART1, PART2 = FIXTURE_NAMES[:2], FIXTURE_NAMES[2:]


@pytest.fixture(scope="module", autouse=True)
def _built(skl):
    assert os.path.exists(CLI)


def ok(*args, cwd=REF_FIXTURES):
    res = subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, cwd=cwd)
    assert res.returncode == 0, res.stderr
    return res


def assert_same_files(a, b):
    for ext in (".skd", ".skm"):
        assert open(f"{a}{ext}", "rb").read() == open(f"{b}{ext}", "rb").read(), ext


def test_append_gpu_assemblies(tmp_path):
    ok("sketch", "--k-vals", "17", *PART1, "-o", tmp_path / "part1")
    ok("append", tmp_path / "part1", *PART2, "-o", tmp_path / "cpu")
    ok("append", tmp_path / "part1", *PART2, "--gpu", "-o", tmp_path / "gpu")
    assert_same_files(tmp_path / "gpu", tmp_path / "cpu")
    ok("append", tmp_path / "part1", *PART2, "--device", "0", "--threads", "2", "-o", tmp_path / "dev0")
    assert_same_files(tmp_path / "dev0", tmp_path / "cpu")


def test_append_gpu_amino_acids(tmp_path):
    residues = "".join(open(os.path.join(REF_FIXTURES, "test_aa_sequence.fa")).read().splitlines()[1:])
    pieces = [f">piece {i}\n{residues[250 * i:250 * (i + 1)]}\n" for i in range(4)]   # (the fixture is one record)
    (tmp_path / "old.fa").write_text("".join(pieces[:2]))
    (tmp_path / "new.fa").write_text("".join(pieces[2:]))
    ok("sketch", "--seq-type", "aa", "--level", "level2", "--concat-fasta", "-k", "9", "-s", "1000", "old.fa", "-o", "old", cwd=tmp_path)
    ok("append", "old", "new.fa", "--concat-fasta", "-o", "cpu", cwd=tmp_path)
    ok("append", "old", "new.fa", "--concat-fasta", "--gpu", "-o", "gpu", cwd=tmp_path)
    assert_same_files(tmp_path / "gpu", tmp_path / "cpu")


def test_append_gpu_read_pair(tmp_path):
    (tmp_path / "r1.txt").write_text("test_1\ttest_1_fwd.fastq.gz\ttest_1_rev.fastq.gz\n")
    (tmp_path / "r2.txt").write_text("test_2\ttest_2_fwd.fastq.gz\ttest_2_rev.fastq.gz\n")
    reads = ["--min-count", "2", "--min-qual", "2"]
    ok("sketch", "-f", tmp_path / "r1.txt", "-k", "9", *reads, "-o", tmp_path / "db1")
    ok("append", tmp_path / "db1", "-f", tmp_path / "r2.txt", *reads, "-o", tmp_path / "cpu")
    ok("append", tmp_path / "db1", "-f", tmp_path / "r2.txt", *reads, "--gpu", "-o", tmp_path / "gpu")
    assert_same_files(tmp_path / "gpu", tmp_path / "cpu")


def test_dist_on_a_renumbered_delete(tmp_path):
    """Samples 0 and 2 of 4 deleted: `dist` loads the result and prints what the database of samples 1 and 3 gives."""
    ok("sketch", "--k-vals", "17,21", *PART1, *PART2, "-o", tmp_path / "all")
    ok("sketch", "--k-vals", "17,21", PART1[1], PART2[1], "-o", tmp_path / "expect")
    (tmp_path / "ids.txt").write_text(f"{PART1[0]}\n{PART2[0]}\n")
    ok("delete", tmp_path / "all", tmp_path / "ids.txt", tmp_path / "deleted")
    for extra in ([], ["-k", "17"], ["--subset", tmp_path / "subset.txt"]):
        (tmp_path / "subset.txt").write_text(f"{PART2[1]}\n{PART1[1]}\n")
        got, want = ok("dist", tmp_path / "deleted", *extra).stdout, ok("dist", tmp_path / "expect", *extra).stdout
        assert got == want and got.count("\n") == 1
