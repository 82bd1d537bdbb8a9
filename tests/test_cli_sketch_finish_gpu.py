"""`sketchlib sketch --gpu` with densification and the transpose on the device (skl_sketch_usigs_packed / skl_sketch_usigs_aa,
csrc/sketch_finish.hip): the `.skd` and `.skm` files are byte for byte those of the CPU path, the metadata (densified bit, a
read set's length estimate from the device's first signs) included, and a sample without a valid k-mer gives the CPU path's error."""
import os
import subprocess

import pytest

from conftest import REF_FIXTURES, ROOT
from helpers import FIXTURE_NAMES

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")
ASSEMBLIES = [os.path.join(REF_FIXTURES, n) for n in FIXTURE_NAMES[:2]]
PAIRS = [[os.path.join(REF_FIXTURES, f"test_{i}_{d}.fastq.gz") for d in ("fwd", "rev")] for i in (1, 2)]


def both_paths(tmp_path, args, env=None):
    """The same command without and with --gpu -> the two (.skd, .skm) byte pairs."""
    outs = []
    for tag, extra in (("cpu", []), ("gpu", ["--gpu"])):
        out = str(tmp_path / tag)
        res = subprocess.run([CLI, "sketch", "-o", out, "--threads", "4", *args, *extra], capture_output=True, text=True, timeout=600,
                             env={**os.environ, **(env or {})})
        assert res.returncode == 0, (tag, res.stderr)
        outs.append((open(out + ".skd", "rb").read(), open(out + ".skm", "rb").read()))
    return outs


def rfile(tmp_path, samples):
    path = tmp_path / "rfile.txt"
    path.write_text("".join(f"s{i}\t" + "\t".join(files) + "\n" for i, files in enumerate(samples)))
    return str(path)


def test_assemblies(gpu_ctx, tmp_path):
    cpu, gpu = both_paths(tmp_path, ["-k", "17,21", "-s", "1000", *ASSEMBLIES])
    assert cpu == gpu


def test_short_proteins_mostly_densified(gpu_ctx, tmp_path):
    fixture = os.path.join(REF_FIXTURES, "test_aa_sequence.fa")
    cpu, gpu = both_paths(tmp_path, ["--seq-type", "aa", "--concat-fasta", "-k", "5", "-s", "1000", fixture])
    assert cpu == gpu


def test_unfiltered_read_set_length_from_the_first_signs(gpu_ctx, tmp_path):
    """(The fixture's reads are few and short: k = 7 and 9 and every base quality, as the other tests of this fixture.)"""
    cpu, gpu = both_paths(tmp_path, ["-k", "7,9", "-s", "1000", "--min-count", "1", "--min-qual", "2", "-f", rfile(tmp_path, PAIRS)])
    assert cpu == gpu


def test_host_finish_switch_writes_the_same_files(gpu_ctx, tmp_path):
    device = both_paths(tmp_path, ["-k", "17,21", "-s", "1000", *ASSEMBLIES])[1]
    host = both_paths(tmp_path, ["-k", "17,21", "-s", "1000", *ASSEMBLIES], env={"SKL_SKETCH_FINISH": "host"})[1]
    assert device == host


def test_filtered_read_set_between_two_assemblies(gpu_ctx, tmp_path):
    """The read set under a count filter keeps the host finish; the assemblies either side of it are not consecutive in the
    `.skd` image, so their finished words are placed sample by sample."""
    samples = [[ASSEMBLIES[0]], PAIRS[0], [ASSEMBLIES[1]]]
    cpu, gpu = both_paths(tmp_path, ["-k", "9", "-s", "1000", "--min-count", "2", "--min-qual", "2", "-f", rfile(tmp_path, samples)])
    assert cpu == gpu


def test_error_text_of_a_sample_shorter_than_k(gpu_ctx, tmp_path):
    runs = [subprocess.run([CLI, "sketch", "-o", str(tmp_path / tag), "-k", "60", *extra, "short_sequence.fa"], cwd=REF_FIXTURES,
                           capture_output=True, text=True) for tag, extra in (("cpu", []), ("gpu", ["--gpu"]))]
    assert runs[0].returncode == runs[1].returncode != 0
    assert "K-mer larger than smallest valid sequence" in runs[0].stderr
    assert runs[0].stderr == runs[1].stderr
