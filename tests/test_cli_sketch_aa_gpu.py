"""`sketchlib sketch --gpu --seq-type aa` (skl_sketch_signs_aa behind csrc/host/sketch_gpu.cpp) writes the files the CPU path
writes, byte for byte, and fails the way it fails; `dist` reads an amino-acid database like any other."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REF_FIXTURES, ROOT
from helpers import rust_f32

pytestmark = pytest.mark.gpu
BUILD = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build")
CLI = os.path.join(BUILD, "sketchlib")
FIXTURE = os.path.join(REF_FIXTURES, "test_aa_sequence.fa")
LETTERS = "ACDEFGHIKLMNPQRSTVWY"


def run(wd, *args):
    return subprocess.run([CLI, "sketch", "--seq-type", "aa", *args], capture_output=True, text=True, cwd=str(wd))


def both_paths(wd, *args):
    cpu, gpu = run(wd, "-o", "cpu", *args), run(wd, "-o", "gpu", "--gpu", *args)
    assert cpu.returncode == 0, cpu.stderr
    assert gpu.returncode == 0, gpu.stderr
    for ext in (".skd", ".skm"):
        assert open(wd / ("cpu" + ext), "rb").read() == open(wd / ("gpu" + ext), "rb").read(), ext


@pytest.mark.parametrize("extra", [[], ["--level", "level2"], ["--level", "level3"], ["--concat-fasta"]],
                         ids=["default", "level2", "level3", "concat"])
def test_fixture_byte_identical_to_the_cpu_path(gpu_ctx, tmp_path, extra):
    both_paths(tmp_path, *extra, "--min-count", "2", "-v", "--k-vals", "9", "--min-qual", "2", FIXTURE)


def write_proteins(path, rng, n, lo=50, hi=2000):
    with open(path, "w") as f:
        for i in range(n):
            length = int(np.clip(rng.lognormal(np.log(300), 0.6), lo, hi))
            seq = "".join(rng.choice(list(LETTERS + "X"), size=length, p=[0.0495] * 20 + [0.01]))
            f.write(f">p{i}\n{seq}\n")
    return str(path)


def test_2000_proteins_with_concat_fasta(gpu_ctx, tmp_path):
    path = write_proteins(tmp_path / "proteins.fa", np.random.default_rng(31), 2000)
    both_paths(tmp_path, "--concat-fasta", "-k", "5,7", "-s", "1000", "--threads", "4", path)
    both_paths(tmp_path, "-k", "5,7", "-s", "1000", path)          # the same file as one proteome


def test_errors_are_the_cpu_paths(gpu_ctx, tmp_path):
    cases = {"exactly_k.fa": (">a\nMKVLAAC\n>b\nACD\n", ["--concat-fasta"], "K-mer larger than smallest valid sequence"),
             "empty_record.fa": (">a\nMKVLA\n>b\n>c\nMKVLA\n", ["--concat-fasta"], "empty_record.fa_2 has no valid sequence"),
             "all_invalid.fa": (">a\nXX*XX--\n", [], "K-mer larger than smallest valid sequence")}
    for name, (text, extra, message) in cases.items():
        (tmp_path / name).write_text(text)
        cpu = run(tmp_path, "-o", "c", "-k", "3", *extra, name)
        gpu = run(tmp_path, "-o", "g", "--gpu", "-k", "3", *extra, name)
        assert cpu.returncode == gpu.returncode == 101, (name, cpu.stderr, gpu.stderr)
        assert message in cpu.stderr and message in gpu.stderr, (name, cpu.stderr, gpu.stderr)
    fq = os.path.join(REF_FIXTURES, "test_1_fwd.fastq.gz")
    gpu = run(tmp_path, "-o", "g", "--gpu", "-k", "5", fq)
    assert gpu.returncode == 101 and "Unexpected quality information with AA sequences" in gpu.stderr


def test_dist_on_an_amino_acid_database(gpu_ctx, oracle, tmp_path):
    """Two related proteomes, sketched on either path; `dist` prints what the oracle computes from the same bins."""
    rng = np.random.default_rng(32)
    a = rng.choice(list(LETTERS), size=30000)
    b = a.copy()
    hit = rng.choice(a.size, size=600, replace=False)
    b[hit] = rng.choice(list(LETTERS), size=hit.size)
    for name, seq in (("a.fa", a), ("b.fa", b)):
        with open(tmp_path / name, "w") as f:
            for r in range(0, seq.size, 500):
                f.write(f">{name}_{r}\n" + "".join(seq[r:r + 500]) + "\n")
    both_paths(tmp_path, "-k", "5,7,9", "-s", "1000", "a.fa", "b.fa")
    bins = np.fromfile(tmp_path / "gpu.skd", dtype="<u8")
    o = oracle.Sketches(bins, 2, [5, 7, 9], 16)
    res = subprocess.run([CLI, "dist", str(tmp_path / "gpu"), "-k", "7"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    d = oracle.self_dists_all(o, oracle.JACCARD, 1).ravel()
    assert 0.0 < d[0] < 1.0
    assert res.stdout == f"a.fa\tb.fa\t{rust_f32(d[0])}\n"
    res = subprocess.run([CLI, "dist", str(tmp_path / "gpu")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert res.stdout.startswith("a.fa\tb.fa\t")
