"""`sketchlib inverted build --gpu` / `inverted query --gpu`: hashing, bin minima, densification and the u16 rows on the device
(skl_sketch_bins_u16_packed; read sets under a count filter: skl_reads_survivors + skl_sketch_finish_u16).  The `.skq` is the
reference's fixture, the `.ski` byte for byte the CPU build's, the query output the reference's goldens and the CPU path's,
and a sample shorter than k gives the CPU path's error."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REF_FIXTURES, ROOT
from helpers import FIXTURE_NAMES

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")
READS = ["test_1_fwd.fastq.gz", "test_1_rev.fastq.gz", "test_2_fwd.fastq.gz", "test_2_rev.fastq.gz"]


@pytest.fixture()
def wd(tmp_path, gpu_ctx):
    for f in FIXTURE_NAMES + ["rfile.txt", "short_sequence.fa"] + READS:
        shutil.copy(os.path.join(REF_FIXTURES, f), tmp_path / f)
    (tmp_path / "reads.txt").write_text("test_1\ttest_1_fwd.fastq.gz\ttest_1_rev.fastq.gz\ntest_2\ttest_2_fwd.fastq.gz\ttest_2_rev.fastq.gz\n")
    (tmp_path / "mixed.txt").write_text("R6\tR6.fa.gz\ntest_1\ttest_1_fwd.fastq.gz\ttest_1_rev.fastq.gz\nTIGR4\tTIGR4.fa.gz\n")
    return tmp_path


def run(wd, *args, ok=True, env=None):
    res = subprocess.run([CLI, *args], cwd=wd, capture_output=True, text=True, timeout=600, env={**os.environ, **(env or {})})
    if ok:
        assert res.returncode == 0, res.stderr
    return res


def build_both(wd, *args):
    """The same build on the CPU path and with --gpu -> ((skq, ski) bytes of each)."""
    out = []
    for tag, extra in (("cpu", ["--threads", "4"]), ("gpu", ["--gpu", "--threads", "4"])):
        run(wd, "inverted", "build", "-o", tag, "--write-skq", *args, *extra)
        out.append(((wd / f"{tag}.skq").read_bytes(), (wd / f"{tag}.ski").read_bytes()))
    return out


def golden(name):
    with open(os.path.join(REF_FIXTURES, name), "rb") as f:
        return f.read()


def test_build_gives_the_reference_skq_and_the_cpu_ski(wd):
    cpu, gpu = build_both(wd, "-k", "21", "-s", "10", "-f", "rfile.txt")
    assert gpu[0] == golden("inverted.skq")
    assert gpu == cpu


def test_build_at_1000_bins_and_with_species_names(wd):
    cpu, gpu = build_both(wd, "-k", "21", "-s", "1000", "-f", "rfile.txt")
    assert gpu == cpu and len(gpu[0]) == 4 * 1000 * 2
    (wd / "species.txt").write_text("R6.fa.gz\tA\nTIGR4.fa.gz\tA\n14412_3#82.contigs_velvet.fa.gz\tB\n14412_3#84.contigs_velvet.fa.gz\tB\n")
    for s in ("10", "1000"):
        cpu, gpu = build_both(wd, "-k", "21", "-s", s, "-f", "rfile.txt", "--species-names", "species.txt")
        assert gpu == cpu
    assert gpu[0] != build_both(wd, "-k", "21", "-s", "1000", "-f", "rfile.txt")[1][0]      # (the labels did reorder the rows)


def test_device_flag_and_timing_line(wd):
    res = run(wd, "inverted", "build", "--device", "0", "-o", "dev", "--write-skq", "-k", "21", "-s", "10", "-f", "rfile.txt", env={"SKL_CLI_TIMING": "1"})
    assert (wd / "dev.skq").read_bytes() == golden("inverted.skq")
    line = [l for l in res.stderr.splitlines() if l.startswith("TIMING inverted build:")]
    assert len(line) == 1 and all(p in line[0] for p in ("parse=", "pack=", "device=", "invert=", "write="))


@pytest.mark.parametrize("mode,name", [(None, "inverted_query_count.stdout"), ("any-bins", "inverted_query_any.stdout"),
                                       ("all-bins", "inverted_query_all.stdout")])
def test_query_reproduces_the_goldens_and_the_cpu_path(wd, mode, name):
    run(wd, "inverted", "build", "--gpu", "-o", "inverted", "-k", "21", "-s", "10", "-f", "rfile.txt")
    extra = [] if mode is None else ["--query-type", mode]
    cpu = run(wd, "inverted", "query", "-f", "rfile.txt", "inverted.ski", *extra).stdout
    gpu = run(wd, "inverted", "query", "--gpu", "--threads", "3", "-f", "rfile.txt", "inverted.ski", *extra).stdout
    assert gpu == cpu
    want = golden(name).decode().splitlines()
    got = gpu.splitlines()
    assert got[0] == want[0] and sorted(got[1:]) == sorted(want[1:])      # (the reference's rows come in thread order)


@pytest.mark.parametrize("min_count", ["2", "1"])
def test_read_pairs(wd, min_count):
    """--min-count 2: survivors on the device, the filter replayed on the host, the u16 finish of the signs on the device;
    --min-count 1: the plain bin-minimum path."""
    args = ("-k", "9", "--min-count", min_count, "--min-qual", "2")
    for s in ("10", "1000"):
        cpu, gpu = build_both(wd, *args, "-s", s, "-f", "reads.txt")
        assert gpu == cpu
    q = ("inverted", "query", "cpu.ski", *args[2:], "-f", "reads.txt")
    cpu_out, gpu_out = run(wd, *q).stdout, run(wd, *q, "--gpu").stdout
    assert gpu_out == cpu_out
    # the counts numpy gives from the .skq rows (the queries are the indexed samples)
    skq = np.frombuffer(cpu[0], dtype="<u2").reshape(2, 1000)
    want = "Query\ttest_1\ttest_2\n" + "".join(f"test_{i + 1}\t" + "\t".join(str(int((skq[i] == skq[j]).sum())) for j in range(2)) + "\n" for i in range(2))
    assert cpu_out == want


def test_read_set_between_two_assemblies_keeps_input_order(wd):
    cpu, gpu = build_both(wd, "-k", "9", "-s", "1000", "--min-count", "2", "--min-qual", "2", "-f", "mixed.txt")
    assert gpu == cpu
    rows = np.frombuffer(gpu[0], dtype="<u2").reshape(3, 1000)
    run(wd, "inverted", "build", "--gpu", "-o", "alone", "--write-skq", "-k", "9", "-s", "1000", "--min-count", "2", "--min-qual", "2", "-f", "reads.txt")
    assert np.array_equal(rows[1], np.fromfile(wd / "alone.skq", dtype="<u2").reshape(2, 1000)[0])


def test_host_finish_switch_writes_the_same_files(wd):
    device = build_both(wd, "-k", "21", "-s", "1000", "-f", "rfile.txt")[1]
    run(wd, "inverted", "build", "--gpu", "-o", "host", "--write-skq", "-k", "21", "-s", "1000", "-f", "rfile.txt", env={"SKL_SKETCH_FINISH": "host"})
    assert ((wd / "host.skq").read_bytes(), (wd / "host.ski").read_bytes()) == device


def test_error_of_a_sample_shorter_than_k(wd):
    (wd / "short.txt").write_text("R6\tR6.fa.gz\nshort\tshort_sequence.fa\n")
    runs = [run(wd, "inverted", "build", "-o", tag, "-k", "60", "-s", "10", "-f", "short.txt", *extra, ok=False) for tag, extra in (("cpu", []), ("gpu", ["--gpu"]))]
    assert runs[0].returncode == runs[1].returncode != 0
    assert "K-mer larger than smallest valid sequence" in runs[0].stderr
    assert runs[0].stderr == runs[1].stderr
    run(wd, "inverted", "build", "-o", "idx", "-k", "60", "-s", "10", "R6.fa.gz")
    runs = [run(wd, "inverted", "query", "idx.ski", "short_sequence.fa", *extra, ok=False) for extra in ([], ["--gpu"])]
    assert runs[0].returncode == runs[1].returncode != 0 and runs[0].stderr == runs[1].stderr
