"""`sketchlib sketch --gpu` on read sets: survivors of the count filter on the device (skl_reads_survivors,
csrc/read_survivors.hip), the filter replayed on the host.  The output files must equal the CPU
path's byte for byte; at the ABI level the survivors under a threshold table must be exactly the windows whose
sign is below their bin's threshold (tests/reads_reference.py's hashes)."""
import os
import subprocess

import numpy as np
import pytest

import reads_reference as R
from conftest import REF_FIXTURES, ROOT

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")
PAIRS = [[os.path.join(REF_FIXTURES, f"test_{i}_{d}.fastq.gz") for d in ("fwd", "rev")] for i in (1, 2)]


def rfile(tmp_path, samples):
    path = tmp_path / "rfile.txt"
    path.write_text("".join(f"s{i}\t" + "\t".join(files) + "\n" for i, files in enumerate(samples)))
    return str(path)


def both_ways(tmp_path, samples, args, env=None):
    """CPU and --gpu runs of the same command -> the two (.skd, .skm) byte pairs."""
    rf = rfile(tmp_path, samples)
    outs = []
    for tag, extra in (("cpu", []), ("gpu", ["--gpu"])):
        out = str(tmp_path / tag)
        res = subprocess.run([CLI, "sketch", "-o", out, "-f", rf, "--threads", "4", *args, *extra], capture_output=True,
                             text=True, timeout=600, env={**os.environ, **(env or {})})
        assert res.returncode == 0, (tag, res.stderr)
        outs.append((open(out + ".skd", "rb").read(), open(out + ".skm", "rb").read()))
    return outs


@pytest.fixture(scope="module")
def genome_reads(tmp_path_factory):
    """Two samples of paired reads from random 200 kb genomes at 30x: 100 bp reads, 1 % substitutions, random
    qualities between '#' and 'I'; the third sample adds 900 poly-A reads (a k-mer seen > 65 535 times)."""
    d = tmp_path_factory.mktemp("reads")
    rng = np.random.default_rng(2024)
    samples = []
    for s in range(3):
        genome = R.random_genome(rng, 200_000)
        files = []
        for end in (1, 2):
            reads = R.synthetic_reads(rng, genome, 30 * 200_000 // 200, 100, 0.01)
            reads = [(sq, rng.integers(35, 74, size=len(sq), dtype=np.uint8).tobytes()) for sq, _ in reads]
            if s == 2:
                reads += [(b"A" * 100, b"I" * 100)] * 900
            path = str(d / f"g{s}_{end}.fastq.gz")
            R.write_fastq(path, reads)
            files.append(path)
        samples.append(files)
    return samples


def test_fixtures_gpu_equals_cpu(tmp_path):
    cpu, gpu = both_ways(tmp_path, PAIRS, ["-k", "9", "--min-count", "2", "--min-qual", "2"])
    assert cpu == gpu


@pytest.mark.parametrize("args,env", [
    (["-k", "15,21,31", "-s", "1000", "--min-count", "5"], None),
    (["-k", "21", "-s", "100000", "--min-count", "3", "--min-qual", "40"], None),
    (["-k", "17", "-s", "1000", "--min-count", "2"], None),
    (["-k", "21", "-s", "1000", "--min-count", "5", "--single-strand"], None),
    (["-k", "15,31", "-s", "1000", "--min-count", "3"], {"SKL_READS_CHUNK_WINDOWS": "3000"}),
])
def test_synthetic_pairs_gpu_equals_cpu(tmp_path, genome_reads, args, env):
    cpu, gpu = both_ways(tmp_path, genome_reads, args, env)
    assert cpu == gpu


def test_min_count_65535_every_window_survives(tmp_path, genome_reads):
    """Only the poly-A k-mer reaches 65 535, so every bin but one stays empty: every window survives every chunk."""
    cpu, gpu = both_ways(tmp_path, genome_reads[2:], ["-k", "21", "-s", "1000", "--min-count", "65535"],
                         {"SKL_READS_CHUNK_WINDOWS": "200000"})
    assert cpu == gpu


def test_survivors_abi_equal_python_hashes(gpu_ctx, skl, tmp_path):
    rng = np.random.default_rng(5)
    genome = R.random_genome(rng, 2000)
    files = []
    for end in (1, 2):
        reads = R.synthetic_reads(rng, genome, 120, (30, 60), 0.01, 0.01, 0.05)
        if end == 1:
            reads = R.pad_to_residue(reads, 53, 2)
        path = str(tmp_path / f"abi_{end}.fastq.gz")
        R.write_fastq(path, reads)
        files.append(path)
    kmers, num_bins = [9, 14], 128
    bin_size = (R.SIGN_MOD + num_bins - 1) // num_bins
    per_k = [R.window_signs(files, k, True, 53) for k in kmers]
    codes, offs = per_k[0][1], per_k[0][2]
    n = codes.size
    packed = skl.pack_codes(codes, [0, n])
    reads = skl.Reads(gpu_ctx, packed, [0, n], offs, [0, offs.size], kmers, num_bins, True)
    thr = rng.integers(0, R.SIGN_MOD, size=(len(kmers), num_bins), dtype=np.uint64)
    thr[:, :4] = np.uint64(2 ** 64 - 1)   # some bins empty: everything in them survives
    for lo, hi in ((0, n // 3), (n // 3 + 5, n + 100)):
        want = [sorted((s, g) for s, g in wins if lo <= s < hi and g < int(thr[ki][g // bin_size]))
                for ki, (wins, _, _) in enumerate(per_k)]
        recs, counts = reads.survivors([lo], [hi], thr, n)
        assert [int(c) for c in counts] == [len(w) for w in want]
        for ki in range(len(kmers)):
            got = sorted(map(tuple, recs[ki, :int(counts[ki])].tolist()))
            assert got == want[ki]
        # room for fewer than found: the counts stay exact, every record written is a true survivor
        cap = max(1, min(len(w) for w in want) // 2)
        recs, counts = reads.survivors([lo], [hi], thr, cap)
        assert [int(c) for c in counts] == [len(w) for w in want]
        for ki in range(len(kmers)):
            got = set(map(tuple, recs[ki, :cap].tolist()))
            assert len(got) == cap and got <= set(want[ki])
    reads.close()
