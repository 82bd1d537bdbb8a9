"""`sketchlib sketch --seq-type aa` on the CPU (csrc/host/aahash.cpp) against tests/aa_reference.py, the line-by-line Python
restatement of the reference's AaHashIterator -- a restatement no reference binary has confirmed (see its docstring).  The C++
derives its roll values as srol^k(seed) and hashes position by position with a run counter; the restatement builds the
reference's split 31 / 33-bit tables and walks the iterator's own state machine.  They meet in the `.skd` bytes.

`dist` needs a GPU: `dist` on an amino-acid database is checked in tests/test_cli_sketch_aa_gpu.py.  The reference refuses
k < 3 for every sequence type (parse_kmers, src/io.rs:153-156) and so does the CLI; k = 1 and 2 are hashed through
tests/native/aa_check.cpp, which calls the same host code without the CLI's rule."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import aa_native
import aa_reference as R
from conftest import REF_FIXTURES, ROOT

BUILD = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build")
CLI = os.path.join(BUILD, "sketchlib")
DBTOOL = os.path.join(BUILD, "skl_dbtool")
FIXTURE = "test_aa_sequence.fa"
REF_ARGS = ["--min-count", "2", "-v", "--k-vals", "9", "--min-qual", "2"]     # tests/sketch.rs:102-140


@pytest.fixture(scope="module", autouse=True)
def _built(skl):
    assert os.path.exists(CLI)


def run_cli(wd, *args):
    return subprocess.run([CLI, "sketch", *args], capture_output=True, text=True, cwd=str(wd))


def sketch(wd, name, *args):
    res = run_cli(wd, "-o", name, "--seq-type", "aa", *args)
    assert res.returncode == 0, res.stderr
    return os.path.join(str(wd), name)


def info(prefix):
    txt = subprocess.check_output([DBTOOL, "info", prefix], text=True)
    fields = dict(l.split("\t", 1) for l in txt.splitlines() if not l.startswith("sample\t"))
    samples = [l.split("\t") for l in txt.splitlines() if l.startswith("sample\t")]
    return fields, samples


def skd(prefix):
    return np.fromfile(prefix + ".skd", dtype="<u8")


def write_fasta(path, records, width=60):
    with open(path, "w") as f:
        for i, seq in enumerate(records):
            f.write(f">rec{i} something\n")
            for x in range(0, len(seq), width):
                f.write(seq[x:x + width] + "\n")
    return str(path)


def assert_matches_restatement(prefix, inputs, kmers, sketch_size, level=1, concat=False, rc=True):
    # (a positional path with a known FASTA extension is named by its file name: read_input_fastas, src/io.rs:20-40)
    inputs = [(os.path.basename(name) if name.endswith((".fa", ".fa.gz")) else name, files) for name, files in inputs]
    want, meta = R.sketch_files(inputs, kmers, sketch_size, level, concat, rc)
    assert np.array_equal(skd(prefix), want.ravel())
    fields, samples = info(prefix)
    assert fields["hash_type"] == f"AA:Level{level}"
    assert fields["kmer_lengths"] == ",".join(str(k) for k in sorted(kmers))
    assert len(samples) == len(meta)
    for i, (row, (name, seq_length, non_acgt, densified)) in enumerate(zip(samples, meta)):
        # sample, position, name, index, seq_length, rc reads densified, acgt, non_acgt
        assert row[1:] == [str(i), name, str(i), str(seq_length), f"{int(rc)}0{int(densified)}", "0,0,0,0", str(non_acgt)], row


@pytest.fixture()
def wd(tmp_path):
    src = os.path.join(REF_FIXTURES, FIXTURE)
    with open(src, "rb") as f, open(tmp_path / FIXTURE, "wb") as g:
        g.write(f.read())
    return tmp_path


@pytest.mark.parametrize("extra,level,concat", [([], 1, False), (["--level", "level2"], 2, False), (["--level", "level3"], 3, False),
                                                 (["--concat-fasta"], 1, True)])
def test_fixture_at_the_references_invocations(wd, extra, level, concat):
    prefix = sketch(wd, "aastest", *extra, *REF_ARGS, "./" + FIXTURE)
    assert_matches_restatement(prefix, [(FIXTURE, [str(wd / FIXTURE)])], [9], 1000, level, concat)
    _, samples = info(prefix)
    assert samples[0][2] == (FIXTURE + "_1" if concat else FIXTURE)
    assert samples[0][4] == ("1000" if concat else "1001")     # a separator follows the record unless it is a sample of its own


def test_fixture_at_three_kmer_lengths(wd):
    prefix = sketch(wd, "k357", "-k", "3,5,7", "-s", "500", "--single-strand", FIXTURE)
    assert_matches_restatement(prefix, [(FIXTURE, [str(wd / FIXTURE)])], [3, 5, 7], 500, rc=False)


def random_protein(rng, n):
    return "".join(rng.choice(list(R.LETTERS), size=n))


def test_levels_group_what_they_say(tmp_path):
    """D<->E and I<->L are one residue from level 2 on, A<->S only at level 3."""
    rng = np.random.default_rng(5)
    base = random_protein(rng, 400)
    swap = lambda s, pairs: s.translate(str.maketrans(pairs[0] + pairs[1], pairs[1] + pairs[0]))
    files = {"base": base, "de_il": swap(base, ("DI", "EL")), "as": swap(base, ("A", "S"))}
    assert files["de_il"] != base and files["as"] != base
    out = {}
    for name, seq in files.items():
        path = write_fasta(tmp_path / (name + ".fa"), [seq])
        for level in (1, 2, 3):
            out[name, level] = open(sketch(tmp_path, f"{name}{level}", "-k", "5", "-s", "256", "--level", f"level{level}", path) + ".skd", "rb").read()
    assert out["de_il", 1] != out["base", 1] and out["as", 1] != out["base", 1]
    assert out["de_il", 2] == out["base", 2] and out["de_il", 3] == out["base", 3]
    assert out["as", 2] != out["base", 2] and out["as", 3] == out["base", 3]


def test_lower_case_equals_upper_case(tmp_path):
    seq = random_protein(np.random.default_rng(6), 300)
    up = sketch(tmp_path, "up", "-k", "4", "-s", "128", write_fasta(tmp_path / "up.fa", [seq]))
    lo = sketch(tmp_path, "lo", "-k", "4", "-s", "128", write_fasta(tmp_path / "lo.fa", [seq.lower()]))
    assert open(up + ".skd", "rb").read() == open(lo + ".skd", "rb").read()
    assert_matches_restatement(lo, [(str(tmp_path / "lo.fa"), [str(tmp_path / "lo.fa")])], [4], 128)


@pytest.mark.parametrize("bad", list("BJOUXZ*-") + ["7"])
def test_invalid_residues_break_windows_and_are_counted(tmp_path, bad):
    rng = np.random.default_rng(7)
    seq = random_protein(rng, 120)
    broken = seq[:50] + bad + seq[51:90] + bad + seq[91:]
    path = write_fasta(tmp_path / "b.fa", [broken])
    prefix = sketch(tmp_path, "b", "-k", "6", "-s", "64", path)
    assert_matches_restatement(prefix, [(path, [path])], [6], 64)
    assert info(prefix)[1][0][7] == "2"
    # and the windows over the two positions are gone: the same as three records cut there
    cut = write_fasta(tmp_path / "c.fa", [seq[:50], seq[51:90], seq[91:]])
    assert open(sketch(tmp_path, "c", "-k", "6", "-s", "64", cut) + ".skd", "rb").read() == open(prefix + ".skd", "rb").read()


def signs_of(check, level, k, bins, concat, *files):
    rows = subprocess.check_output([check, "signs", str(level), str(k), str(bins), str(int(concat)), *files], text=True).splitlines()
    out = []
    for row in rows:
        name, length, invalid, signs = row.split("\t")
        out.append(None if signs == "none" else np.array([int(x) for x in signs.split(",")], dtype=np.uint64))
    return out


def test_end_rule_with_concat_fasta(tmp_path):
    """The iterator seeds only where start < len - k: the window at len - k exists only when it is rolled into."""
    check = aa_native.build()
    k, bins = 3, 4096
    recs = {"MKV*ACD": ["MKV"], "MKVA": ["MKV", "KVA"], "ACDEFG": ["ACD", "CDE", "DEF", "EFG"], "MK*ACDE": ["ACD", "CDE"]}
    path = write_fasta(tmp_path / "e.fa", list(recs))
    got = signs_of(check, 1, k, bins, True, path)
    for (rec, windows), g in zip(recs.items(), got):
        assert np.array_equal(g, R.get_signs_no_densify(R.iterator_of(rec), k, bins)), rec
        assert int((g != np.uint64(R.U64)).sum()) == len(windows), rec     # (these few signs fall into different bins)
    # through the CLI: byte-identical to the restatement, one sample per record
    prefix = sketch(tmp_path, "e", "-k", "3", "-s", "64", "--concat-fasta", path)
    assert_matches_restatement(prefix, [(path, [path])], [3], 64, concat=True)
    # without --concat-fasta a separator ends every record and all the windows are there
    whole = signs_of(check, 1, k, bins, False, path)[0]
    assert np.array_equal(whole, R.natural_signs("*".join(recs), k, bins))
    assert int((whole != np.uint64(R.U64)).sum()) == len({"MKV", "ACD", "KVA", "CDE", "DEF", "EFG"})
    prefix = sketch(tmp_path, "w", "-k", "3", "-s", "64", path)
    assert_matches_restatement(prefix, [(path, [path])], [3], 64)


def test_exactly_k_residues_panic_with_concat_fasta(tmp_path):
    path = write_fasta(tmp_path / "x.fa", ["MKVLA", "ACD"])
    res = run_cli(tmp_path, "-o", "x", "--seq-type", "aa", "-k", "3", "--concat-fasta", path)
    assert res.returncode == 101 and "K-mer larger than smallest valid sequence" in res.stderr
    # a record shorter than k, and one whose only window is not seedable
    for rec in ("AC", "AC*DEF"):
        res = run_cli(tmp_path, "-o", "x", "--seq-type", "aa", "-k", "3", "--concat-fasta", write_fasta(tmp_path / "y.fa", ["MKVLA", rec]))
        assert res.returncode == 101 and "K-mer larger than smallest valid sequence" in res.stderr, rec
        with pytest.raises(R.ReferencePanic):
            R.iterator_of(rec).set_k(3)
    # the same records without --concat-fasta give all their windows
    prefix = sketch(tmp_path, "z", "-k", "3", "-s", "64", path)
    assert_matches_restatement(prefix, [(path, [path])], [3], 64)
    # an empty record is a sample without sequence
    empty = tmp_path / "empty.fa"
    empty.write_text(">a\nMKVLA\n>b\n>c\nMKVLA\n")
    res = run_cli(tmp_path, "-o", "x", "--seq-type", "aa", "-k", "3", "--concat-fasta", str(empty))
    assert res.returncode == 101 and "empty.fa_2 has no valid sequence" in res.stderr


@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 34, 62, 64, 66])
def test_roll_periods_on_a_random_protein(tmp_path, k):
    """k at and around the periods of the two halves of the split rotation (31, 33, and twice those)."""
    seq = random_protein(np.random.default_rng(8), 300)
    path = write_fasta(tmp_path / "p.fa", [seq])
    if k < 3:     # the reference's parse_kmers panics, whatever the sequence type
        res = run_cli(tmp_path, "-o", "p", "--seq-type", "aa", "-k", str(k), path)
        assert res.returncode != 0 and "K-mers must be >=3" in res.stderr
        got = signs_of(aa_native.build(), 1, k, 1024, False, path)[0]
        assert np.array_equal(got, R.get_signs_no_densify(R.iterator_of(seq + "*"), k, 1024))
        return
    prefix = sketch(tmp_path, "p", "-k", str(k), "-s", "1000", path)
    assert_matches_restatement(prefix, [(path, [path])], [k], 1000)


def test_gz_input_and_two_files_per_sample(tmp_path):
    rng = np.random.default_rng(9)
    a, b = [random_protein(rng, 200), random_protein(rng, 90)], [random_protein(rng, 150)]
    fa = write_fasta(tmp_path / "a.fa", a)
    fb = write_fasta(tmp_path / "b.fa", b)
    gz = str(tmp_path / "a.fa.gz")
    with open(fa, "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read())
    plain = sketch(tmp_path, "plain", "-k", "5", "-s", "128", fa)
    zipped = sketch(tmp_path, "zipped", "-k", "5", "-s", "128", gz)
    assert open(plain + ".skd", "rb").read() == open(zipped + ".skd", "rb").read()
    (tmp_path / "rfile.txt").write_text(f"both\t{gz}\t{fb}\nalone\t{fb}\n")
    for concat in (False, True):
        prefix = sketch(tmp_path, f"two{int(concat)}", "-k", "5", "-s", "128", "-f", "rfile.txt", *(["--concat-fasta"] if concat else []))
        assert_matches_restatement(prefix, [("both", [gz, fb]), ("alone", [fb])], [5], 128, concat=concat)
        if concat:
            assert [s[2] for s in info(prefix)[1]] == ["both_1", "both_2", "both_3", "alone_1"]     # n counts across a sample's files


def test_refusals():
    fq = os.path.join(REF_FIXTURES, "test_1_fwd.fastq.gz")
    res = run_cli(REF_FIXTURES, "-o", "/dev/null/x", "--seq-type", "aa", "-k", "5", fq)
    assert res.returncode == 101 and "Unexpected quality information with AA sequences" in res.stderr
    res = run_cli(REF_FIXTURES, "-o", "/dev/null/x", "--concat-fasta", "-k", "21", "R6.fa.gz")
    assert res.returncode == 101 and "--concat-fasta currently only supported with --seq-type aa" in res.stderr
    res = run_cli(REF_FIXTURES, "-o", "/dev/null/x", "--seq-type", "pdb", "-k", "5", FIXTURE)
    assert res.returncode == 2 and "structures are not part of this build" in res.stderr
    res = run_cli(REF_FIXTURES, "-o", "/dev/null/x", "--seq-type", "aa", "--level", "level4", "-k", "5", FIXTURE)
    assert res.returncode == 2 and "level4" in res.stderr


def test_dna_still_ignores_level_and_writes_dna(tmp_path):
    res = run_cli(REF_FIXTURES, "-o", str(tmp_path / "d"), "--seq-type", "dna", "--level", "level2", "-k", "21", "-s", "1000", "R6.fa.gz")
    assert res.returncode == 0, res.stderr
    assert info(str(tmp_path / "d"))[0]["hash_type"] == "DNA"
