"""`sketchlib sketch` on read sets (FASTQ, one or two files per sample) on the CPU: the reference's own test case
(tests/sketch.rs:46-100), byte equality with an independent Python restatement of the reference
(tests/reads_reference.py) on the reference's fixtures and on synthetic read pairs, the errors, and FASTA runs
that --min-count / --min-qual leave alone."""
import os
import subprocess

import numpy as np
import pytest

import reads_reference as R
from conftest import REF_FIXTURES, ROOT

BUILD = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build")
CLI = os.path.join(BUILD, "sketchlib")
DBTOOL = os.path.join(BUILD, "skl_dbtool")
PAIRS = [[os.path.join(REF_FIXTURES, f"test_{i}_{d}.fastq.gz") for d in ("fwd", "rev")] for i in (1, 2)]


@pytest.fixture(scope="module", autouse=True)
def _built(skl):
    assert os.path.exists(CLI)


def rfile(tmp_path, samples):
    path = tmp_path / "rfile.txt"
    path.write_text("".join(f"s{i}\t" + "\t".join(files) + "\n" for i, files in enumerate(samples)))
    return str(path)


def run_sketch(tmp_path, name, *args, check=True):
    out = str(tmp_path / name)
    res = subprocess.run([CLI, "sketch", "-o", out, *args], capture_output=True, text=True, cwd=REF_FIXTURES)
    if check:
        assert res.returncode == 0, res.stderr
    return out, res


def info_samples(prefix):
    """dbtool info's sample lines -> [(name, seq_length, flags rc/reads/densified, acgt, non_acgt)]."""
    txt = subprocess.check_output([DBTOOL, "info", prefix], text=True)
    rows = [l.split("\t") for l in txt.splitlines() if l.startswith("sample\t")]
    return [(r[2], int(r[4]), r[5], [int(x) for x in r[6].split(",")], int(r[7])) for r in rows], txt


def test_reference_read_sketch_info(tmp_path):
    """sketch -f <the two pairs> -k 9 --min-count 2 --min-qual 2: read_sketch_full_info.stdout's values."""
    path = tmp_path / "rfile.txt"
    path.write_text("test_1\ttest_1_fwd.fastq.gz\ttest_1_rev.fastq.gz\ntest_2\ttest_2_fwd.fastq.gz\ttest_2_rev.fastq.gz\n")
    out, _ = run_sketch(tmp_path, "reads", "-f", str(path), "-k", "9", "--min-count", "2", "--min-qual", "2")
    rows, txt = info_samples(out)
    # (acgt is stored A, C, G, T; the reference prints A, C, T, G: [603, 330, 334, 603])
    assert rows == [("test_1", 1, "111", [603, 330, 603, 334], 0), ("test_2", 1, "111", [617, 312, 617, 314], 0)]
    for key in ("sketch_size\t1024", "kmer_lengths\t9", "n_samples\t2"):
        assert key in txt


@pytest.mark.parametrize("min_count,min_qual,rc", [(2, 2, True), (1, 2, True), (3, 2, False), (3, 2, True)])
def test_fixtures_equal_restatement(tmp_path, min_count, min_qual, rc):
    args = ["-k", "9", "--min-count", str(min_count), "--min-qual", str(min_qual)] + ([] if rc else ["--single-strand"])
    out, _ = run_sketch(tmp_path, "reads", "-f", rfile(tmp_path, PAIRS), *args)
    skd, metas = R.sketch_skd(PAIRS, [9], 1000, rc, min_count, min_qual)
    assert open(out + ".skd", "rb").read() == skd
    rows, _ = info_samples(out)
    assert [r[1] for r in rows] == [m["seq_length"] for m in metas]


def synthetic_pairs(tmp_path, seed, residue, n_samples=2):
    """Read pairs from a small random genome: 1 % substitutions, 1 % N, 5 % low-quality ('#' < '5') bases; the kept bases
    of every first file number `residue` mod 4 (so 4 - residue padding bases sit between the files)."""
    rng = np.random.default_rng(seed)
    samples = []
    for s in range(n_samples):
        genome = R.random_genome(rng, 300)
        files = []
        for end in (1, 2):
            reads = R.synthetic_reads(rng, genome, 50, (20, 45), 0.01, 0.01, 0.05)
            if end == 1:
                reads = R.pad_to_residue(reads, ord("5"), residue)
            path = str(tmp_path / f"syn{seed}_{s}_{end}.fastq.gz")
            R.write_fastq(path, reads)
            files.append(path)
        samples.append(files)
    return samples


@pytest.mark.parametrize("residue", [1, 2, 3])
@pytest.mark.parametrize("min_count", [1, 2, 3, 5])
@pytest.mark.parametrize("rc", [True, False])
def test_synthetic_pairs_equal_restatement(tmp_path, residue, min_count, rc):
    samples = synthetic_pairs(tmp_path, 100 * residue + min_count, residue)
    kmers = [7, 11]
    args = ["-k", "7,11", "-s", "100", "--min-count", str(min_count), "--min-qual", "53"] + ([] if rc else ["--single-strand"])
    out, _ = run_sketch(tmp_path, "syn", "-f", rfile(tmp_path, samples), *args)
    skd, metas = R.sketch_skd(samples, kmers, 100, rc, min_count, 53)
    assert open(out + ".skd", "rb").read() == skd
    rows, _ = info_samples(out)
    assert [(r[1], r[3], r[4]) for r in rows] == [(m["seq_length"], m["acgt"], m["non_acgt"]) for m in metas]
    assert all(r[2][1] == "1" for r in rows)   # reads


def test_single_fastq_file_and_padding_windows(tmp_path):
    """One file per sample has no padding; two files with 1-3 padding bases hash the windows that span them."""
    samples = synthetic_pairs(tmp_path, 7, 1, n_samples=1)
    single = [[samples[0][0]]]
    out, _ = run_sketch(tmp_path, "one", "-f", rfile(tmp_path, single), "-k", "9", "-s", "64", "--min-count", "1", "--min-qual", "53")
    assert open(out + ".skd", "rb").read() == R.sketch_skd(single, [9], 64, True, 1, 53)[0]
    # the window list of the pair includes starts inside the padding of file 1's last byte
    wins, codes, offs = R.window_signs(samples[0], 9, True, 53)
    n1 = R.kept_bases(R.read_fastx(samples[0][0])[0], 53)
    assert n1 % 4 == 1 and any(n1 <= s < n1 + 3 for s, _ in wins)


@pytest.fixture(scope="module")
def abi_pair(tmp_path_factory):
    """A read pair built as tests/test_gpu_sketch_reads.py's ABI test builds its own: a 2 kb genome, 120 reads per
    file (here of 30-90 bases, so that k = 65 has windows) with 1 % N and 5 % low-quality bases, two padding bases
    between the files at min_qual 53."""
    d = tmp_path_factory.mktemp("abi_pair")
    rng = np.random.default_rng(5)
    genome = R.random_genome(rng, 2000)
    files = []
    for end in (1, 2):
        reads = R.synthetic_reads(rng, genome, 120, (30, 90), 0.01, 0.01, 0.05)
        if end == 1:
            reads = R.pad_to_residue(reads, 53, 2)
        path = str(d / f"abi_{end}.fastq.gz")
        R.write_fastq(path, reads)
        files.append(path)
    return files


@pytest.mark.parametrize("k,rc", [(1, True), (9, True), (32, False), (33, True), (65, True)])
def test_window_table_equals_literal_iterator(abi_pair, k, rc):
    """The vectorised window list the GPU survivor tests expect from (searchsorted mask, non-rolling hashes) against
    the literal restatement of the reference's iterator (rolling hashes, next_iterator's restarts): the same starts
    and the same signs, on the codes and offsets the literal one hands to the device."""
    wins, codes, offs = R.window_signs(abi_pair, k, rc, 53)
    starts, signs = R.window_table(codes, offs, k, rc)
    assert wins   # (k = 65 leaves a handful on this input, k = 1 about 14 000)
    assert starts.tolist() == [s for s, _ in wins]
    assert signs.tolist() == [g for _, g in wins]


def test_three_read_files_panic(tmp_path):
    f = PAIRS[0]
    _, res = run_sketch(tmp_path, "x", "-f", rfile(tmp_path, [f + [f[0]]]), "-k", "9", check=False)
    assert res.returncode == 101
    assert "Input files are reads, but there are more than two input files" in res.stderr


@pytest.mark.parametrize("body", [
    b"@r0\nACGTACGTAC\n+\nIIIIIIIIII\n@r1\nACGTAC\n",          # truncated record
    b"@r0\nACGTACGTAC\n+\nIIIIIII\n",                          # quality shorter than the sequence
    b"@r0\nACGTACGTAC\nIIIIIIIIII\n+\n",                       # lines out of order
])
def test_bad_fastq_is_an_error_not_a_crash(tmp_path, body):
    path = tmp_path / "bad.fastq"
    path.write_bytes(body)
    _, res = run_sketch(tmp_path, "x", "-k", "5", str(path), check=False)
    assert res.returncode == 101, (res.returncode, res.stderr)
    assert "Invalid FASTA/Q record" in res.stderr


@pytest.mark.parametrize("flag,value", [("--min-count", "70000"), ("--min-qual", "256"), ("--min-count", "-1")])
def test_out_of_range_filters_are_usage_errors(tmp_path, flag, value):
    _, res = run_sketch(tmp_path, "x", "-k", "9", flag, value, PAIRS[0][0], check=False)
    assert res.returncode == 2 and flag in res.stderr


def test_nothing_passes_is_an_error(tmp_path):
    """--min-count above every k-mer's count leaves every bin empty (the reference loops forever in densify)."""
    _, res = run_sketch(tmp_path, "x", "-f", rfile(tmp_path, PAIRS), "-k", "9", "--min-count", "1000", check=False)
    assert res.returncode == 101 and "reached --min-count 1000" in res.stderr


@pytest.mark.parametrize("extra", [["--min-count", "3"], ["--min-qual", "90"], ["--min-count", "1", "--min-qual", "0"]])
def test_fasta_unchanged_by_read_options(tmp_path, extra):
    out, _ = run_sketch(tmp_path, "sketches1", "-k", "31", "-s", "1000", "-f", "rfile.txt", *extra)
    assert open(out + ".skd", "rb").read() == open(os.path.join(REF_FIXTURES, "sketches1.skd"), "rb").read()
    rows, _ = info_samples(out)
    ref, _ = info_samples(os.path.join(REF_FIXTURES, "sketches1"))
    assert rows == ref


def test_reads_entry_without_device(skl):
    """No CPU fall-back: without a device, skl_reads_create refuses with SKL_ERR_NO_DEVICE."""
    if skl.device_count() > 0:
        pytest.skip("a GPU is present; the refusal path is only reachable without one")
    with pytest.raises(skl.SklError) as e:
        skl.Reads(None, np.zeros(1, np.uint32), [0, 16], [], [0, 0], [9], 64)
    assert e.value.code == skl.ERR_NO_DEVICE
    assert "no CPU path" in e.value.message
