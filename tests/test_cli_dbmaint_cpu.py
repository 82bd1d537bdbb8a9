"""`sketchlib merge | append | delete | info` without a GPU: the reference's own test plans (tests/merge.rs, concat.rs,
delete.rs) on the four fixture assemblies at --k-vals 17, plus this project's deliberate differences -- `append` sketches
amino acids at the DATABASE's level and refuses its own input as output, `delete` renumbers the kept samples -- and the
exact text of `info`.  Databases are compared through their `.skd` bytes and through `skl_dbtool info` (every field of the
`.skm` but the order of the name map)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REF_FIXTURES, ROOT
from helpers import FIXTURE_NAMES

BUILD = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build")
CLI = os.path.join(BUILD, "sketchlib")
DBTOOL = os.path.join(BUILD, "skl_dbtool")
PART1, PART2 = FIXTURE_NAMES[:2], FIXTURE_NAMES[2:]
AA_FIXTURE = "test_aa_sequence.fa"
READS_RFILE = ("test_1\ttest_1_fwd.fastq.gz\ttest_1_rev.fastq.gz\n", "test_2\ttest_2_fwd.fastq.gz\ttest_2_rev.fastq.gz\n")
READS_ARGS = ["--min-count", "2", "--min-qual", "2"]


@pytest.fixture(scope="module", autouse=True)
def _built(skl):
    assert os.path.exists(CLI)


def run(*args, cwd=REF_FIXTURES, env=None):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, cwd=cwd, env=env)


def ok(*args, **kw):
    res = run(*args, **kw)
    assert res.returncode == 0, res.stderr
    return res


def dbinfo(prefix):
    """skl_dbtool info as (fields, sample rows); the version is left out (merge.rs / concat.rs ignore it too)."""
    lines = subprocess.check_output([DBTOOL, "info", str(prefix)], text=True).splitlines()
    fields = dict(l.split("\t", 1) for l in lines if not l.startswith("sample\t"))
    return fields, [l.split("\t") for l in lines if l.startswith("sample\t")]


def assert_same_database(a, b):
    assert open(f"{a}.skd", "rb").read() == open(f"{b}.skd", "rb").read()
    (fa, sa), (fb, sb) = dbinfo(a), dbinfo(b)
    fa.pop("sketch_version"), fb.pop("sketch_version")
    assert fa == fb
    assert sa == sb


@pytest.fixture(scope="module")
def dbs(tmp_path_factory, _built):
    """part1 = the two velvet assemblies, part2 = R6 + TIGR4, and the four in both orders, all at --k-vals 17."""
    d = tmp_path_factory.mktemp("dbmaint")
    for name, files in (("part1", PART1), ("part2", PART2), ("all", PART1 + PART2), ("new_first", PART2 + PART1)):
        ok("sketch", "--k-vals", "17", *files, "-o", d / name)
    return d


# ---- merge (tests/merge.rs) ----
def test_merge_equals_one_go(dbs, tmp_path):
    ok("merge", dbs / "part1", dbs / "part2.skm", "-v", "-o", tmp_path / "merged")
    assert_same_database(tmp_path / "merged", dbs / "all")


def test_merge_refuses_shared_names_and_incompatible_databases(dbs, tmp_path):
    res = run("merge", dbs / "part1", dbs / "part1", "-o", tmp_path / "x")
    assert res.returncode == 101 and f"{PART1[0]} appears in both databases. Cannot merge sketches." in res.stderr
    for other in ("sketches2", "sketches3"):   # another sketch size, another k-mer list
        res = run("merge", "sketches1", other, "-o", tmp_path / "x")
        assert res.returncode == 101 and "Databases are not compatible for merging." in res.stderr
    res = run("merge", "sketches1", "-o", tmp_path / "x")
    assert res.returncode == 2 and "<DB2>" in res.stderr


# ---- append (tests/concat.rs): the NEW samples come first ----
def test_append_equals_one_go_new_samples_first(dbs, tmp_path):
    ok("append", dbs / "part1", *PART2, "-v", "-o", tmp_path / "appended")
    assert_same_database(tmp_path / "appended", dbs / "new_first")
    _, samples = dbinfo(tmp_path / "appended")
    assert [s[2] for s in samples] == PART2 + PART1 and [s[3] for s in samples] == ["0", "1", "2", "3"]


def test_append_refuses_duplicates_before_sketching(dbs, tmp_path):
    res = run("append", dbs / "part1", "R6.fa.gz", PART1[0], "-o", tmp_path / "x")
    assert res.returncode == 101 and "Databases are not compatible for merging." in res.stderr
    assert res.stdout == f'Duplicates found: ["{PART1[0]}"]\n'
    assert not os.path.exists(tmp_path / "x.skd") and not os.path.exists(tmp_path / "x.skm")


def test_append_refuses_its_database_as_output_and_concat_fasta_on_dna(dbs, tmp_path):
    before = open(dbs / "part1.skd", "rb").read()
    for out in (dbs / "part1", str(dbs / "part1") + ".skm"):
        res = run("append", dbs / "part1", *PART2, "-o", out)
        assert res.returncode == 1 and res.stderr.startswith("Error: ")
    assert open(dbs / "part1.skd", "rb").read() == before
    res = run("append", dbs / "part1", *PART2, "--concat-fasta", "-o", tmp_path / "x")
    assert res.returncode == 101 and "--concat-fasta currently only supported with --seq-type aa" in res.stderr
    res = run("append", dbs / "part1", "-o", tmp_path / "x")
    assert res.returncode == 2
    assert "append" in ok("--help").stdout


def split_fasta(path):
    """The fixture is ONE record of 1 000 residues: its sequence cut into four records of 250, two for each half."""
    residues = "".join(open(path).read().splitlines()[1:])
    assert len(residues) == 1000
    records = [f">piece {i}\n{residues[250 * i:250 * (i + 1)]}\n" for i in range(4)]
    return records[:2], records[2:]


@pytest.mark.parametrize("level", ["level1", "level2"])
def test_append_amino_acids_at_the_databases_level(tmp_path, level):
    first, second = split_fasta(os.path.join(REF_FIXTURES, AA_FIXTURE))
    assert first and second
    (tmp_path / "old.fa").write_text("".join(first))
    (tmp_path / "new.fa").write_text("".join(second))
    aa = ["--seq-type", "aa", "--level", level, "--concat-fasta", "-k", "9", "-s", "1000"]
    ok("sketch", *aa, "old.fa", "-o", "old", cwd=tmp_path)
    ok("sketch", *aa, "new.fa", "old.fa", "-o", "one_go", cwd=tmp_path)
    ok("append", "old", "new.fa", "--concat-fasta", "-o", "appended", cwd=tmp_path)   # no --level: the database's
    assert_same_database(tmp_path / "appended", tmp_path / "one_go")
    assert dbinfo(tmp_path / "appended")[0]["hash_type"] == "AA:Level" + level[-1]
    ok("append", "old", "new.fa", "--concat-fasta", "--level", level, "-o", "same_level", cwd=tmp_path)
    assert_same_database(tmp_path / "same_level", tmp_path / "one_go")
    other = "level3" if level != "level3" else "level1"
    res = run("append", "old", "new.fa", "--concat-fasta", "--level", other, "-o", "other_level", cwd=tmp_path)
    assert res.returncode == 1 and res.stderr.startswith("Error: ") and other in res.stderr
    assert not os.path.exists(tmp_path / "other_level.skd")


def test_append_read_sets(tmp_path):
    for name, lines in (("r1.txt", READS_RFILE[:1]), ("r2.txt", READS_RFILE[1:]), ("r21.txt", READS_RFILE[::-1])):
        (tmp_path / name).write_text("".join(lines))
    ok("sketch", "-f", tmp_path / "r1.txt", "-k", "9", *READS_ARGS, "-o", tmp_path / "db1")
    ok("sketch", "-f", tmp_path / "r21.txt", "-k", "9", *READS_ARGS, "-o", tmp_path / "one_go")
    ok("append", tmp_path / "db1", "-f", tmp_path / "r2.txt", *READS_ARGS, "-o", tmp_path / "appended")
    assert_same_database(tmp_path / "appended", tmp_path / "one_go")
    assert [s[2] + s[5][1] for s in dbinfo(tmp_path / "appended")[1]] == ["test_21", "test_11"]   # (name, then the reads flag)


# ---- delete (tests/delete.rs) ----
def test_delete_equals_database_of_the_others(dbs, tmp_path):
    (tmp_path / "ids.txt").write_text("R6.fa.gz\nTIGR4.fa.gz\n")
    ok("delete", dbs / "all", tmp_path / "ids.txt", tmp_path / "deleted")
    assert_same_database(tmp_path / "deleted", dbs / "part1")


def test_delete_renumbers_the_kept_samples(dbs, tmp_path):
    """Samples 0 and 2 of 4 go: the reference would keep index 1 and 3; here the output is the database of samples 1, 3.
    (`dist` needs a device: that it prints the same for both databases is tests/test_cli_append_gpu.py's.)"""
    (tmp_path / "ids.txt").write_text(f"{PART1[0]}\n{PART2[0]}")   # (no final newline)
    ok("delete", str(dbs / "all") + ".skd", tmp_path / "ids.txt", tmp_path / "deleted")
    ok("sketch", "--k-vals", "17", PART1[1], PART2[1], "-o", tmp_path / "expect")
    assert_same_database(tmp_path / "deleted", tmp_path / "expect")
    _, samples = dbinfo(tmp_path / "deleted")
    assert [(s[2], s[3]) for s in samples] == [(PART1[1], "0"), (PART2[1], "1")]
    # it loads: every slice read through the loader is the block of the expected database
    words = 16 * 14
    expect = np.fromfile(tmp_path / "expect.skd", dtype="<u8").reshape(2, words)
    for i in range(2):
        got = subprocess.check_output([DBTOOL, "slice", str(tmp_path / "deleted"), str(i), "0"], text=True).split()
        assert np.array_equal(np.array(got, dtype=np.uint64), expect[i])
    # ... and by name, through the renumbered name map (a stale index 3 would be out of range)
    got = subprocess.check_output([DBTOOL, "slice-selected", str(tmp_path / "deleted"), "0", "0", PART2[1]], text=True).split()
    assert np.array_equal(np.array(got, dtype=np.uint64), expect[1])


def test_delete_unknown_ids(dbs, tmp_path):
    (tmp_path / "ids.txt").write_text("R6.fa.gz\n\nnope\n")   # the blank middle line is the id ""
    res = run("delete", dbs / "all", tmp_path / "ids.txt", tmp_path / "deleted")
    assert res.returncode == 1
    assert res.stderr == 'Error: The following samples have not been found in the database: ["", "nope"]\n'
    assert not os.path.exists(tmp_path / "deleted.skd") and not os.path.exists(tmp_path / "deleted.skm")
    (tmp_path / "ids.txt").write_text("R6.fa.gz\n")           # the final newline yields no empty id
    ok("delete", dbs / "all", tmp_path / "ids.txt", tmp_path / "deleted")
    assert dbinfo(tmp_path / "deleted")[0]["n_samples"] == "3"
    res = run("delete", dbs / "all", tmp_path / "ids.txt", dbs / "all")
    assert res.returncode == 1


# ---- info ----
def expected_info(prefix):
    f, samples = dbinfo(prefix)
    version = [l for l in subprocess.check_output([DBTOOL, "info", str(prefix)], text=True).splitlines()
               if l.startswith("sketch_version")][0].split("\t")[1]
    seq = f["hash_type"]
    if ":" in seq:
        seq = "{}({})".format(*seq.split(":"))
    kmers = ", ".join(f["kmer_lengths"].split(","))
    head = (f"sketch_version={version}\nsequence_type={seq}\nsketch_size={f['sketch_size']}\nn_samples={f['n_samples']}\n"
            f"kmers=[{kmers}]\ninverted=false\n")
    rows = "Name\tSequence length\tBase frequencies\tMissing/ambig bases\tFrom reads\tSingle strand\tDensified\n"
    for _, _, name, _, seq_length, flags, acgt, non_acgt in samples:
        a, c, g, t = acgt.split(",")      # stored order; printed as acgt[0], [1], [3], [2]
        rc, reads, densified = (ch == "1" for ch in flags)
        tf = {True: "true", False: "false"}
        rows += f"{name}\t{seq_length}\t[{a}, {c}, {t}, {g}]\t{non_acgt}\t{tf[reads]}\t{tf[not rc]}\t{tf[densified]}\n"
    return head, rows + "\n"


@pytest.mark.parametrize("db,arg", [("sketches1", "sketches1"), ("sketches1", "sketches1.skm"), ("legacy_db", "legacy_db.skd")])
def test_info_text(db, arg):
    head, rows = expected_info(os.path.join(REF_FIXTURES, db))
    res = ok("info", arg, "-v")
    assert res.stdout == head and "Complete in" not in res.stderr
    assert ok("info", arg, "--sample-info").stdout == rows


def test_info_fixture_values():
    """The same against values written out: the reference prints the bins (1024; 2 x 64 for the pre-0.2.0 file)."""
    assert ok("info", "sketches1").stdout == "sketch_version=0.2.0\nsequence_type=DNA\nsketch_size=1024\nn_samples=4\nkmers=[31]\ninverted=false\n"
    assert ok("info", "legacy_db").stdout == ("sketch_version=0.1.3\nsequence_type=DNA\nsketch_size=128\nn_samples=2\n"
                                             "kmers=[17, 21, 25]\ninverted=false\n")
    first = ok("info", "sketches1", "--sample-info").stdout.splitlines()[1]
    assert first == f"{FIXTURE_NAMES[0]}\t1832266\t[571702, 352572, 343740, 564252]\t579\tfalse\tfalse\tfalse"
    res = run("info", "no_such_db")
    assert res.returncode == 101 and "Could not read sketch metadata from no_such_db.skm" in res.stderr


def test_info_amino_acid_level(tmp_path):
    ok("sketch", "--seq-type", "aa", "--level", "level2", "-k", "9", "-s", "1000", AA_FIXTURE, "-o", tmp_path / "aa")
    assert "sequence_type=AA(Level2)\n" in ok("info", tmp_path / "aa").stdout


def rust_f64(x):
    return np.format_float_positional(np.float64(x), unique=True, trim="-")


def test_info_inverted_index(tmp_path):
    ok("inverted", "build", "-o", tmp_path / "idx", "-k", "21", "-s", "10", "-f", "rfile.txt", "--write-skq")
    skq = np.fromfile(tmp_path / "idx.skq", dtype="<u2").reshape(4, 10)
    sizes = [len(set(skq[:, b].tolist())) for b in range(10)]   # distinct values per bin = hash lists per bin
    want = ("sketch_version=0.3.0\nsequence_type=DNA\nsketch_size=10\nn_samples=4\nkmer=21\nrc=true\ninverted=true\n"
            f"max_hashes_per_bin={max(sizes)}\nmin_hashes_per_bin={min(sizes)}\navg_hashes_per_bin={rust_f64(sum(sizes) / 10)}\n")
    assert ok("info", str(tmp_path / "idx") + ".ski").stdout == want
    names = [l.split("\t")[0] for l in open(os.path.join(REF_FIXTURES, "rfile.txt")).read().splitlines()]
    assert ok("info", str(tmp_path / "idx") + ".ski", "--sample-info").stdout == "Name\n" + "".join(n + "\n" for n in names) + "\n"
    # a whole-number average prints without a fraction, as Rust's `{}` does: one sample, one value in every bin
    ok("inverted", "build", "-o", tmp_path / "one", "-k", "21", "-s", "10", "R6.fa.gz")
    assert ok("info", str(tmp_path / "one") + ".ski").stdout.endswith("max_hashes_per_bin=1\nmin_hashes_per_bin=1\navg_hashes_per_bin=1\n")
    res = run("info", tmp_path / "missing.ski")
    assert res.returncode == 101 and res.stdout.startswith("Read error: ") and "Could not read inverted index" in res.stderr


# ---- no device ----
def test_file_commands_need_no_device(dbs, tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    ok("merge", dbs / "part1", dbs / "part2", "-o", tmp_path / "merged", env=env)
    assert_same_database(tmp_path / "merged", dbs / "all")
    (tmp_path / "ids.txt").write_text("R6.fa.gz\nTIGR4.fa.gz\n")
    ok("delete", tmp_path / "merged", tmp_path / "ids.txt", tmp_path / "deleted", env=env)
    assert_same_database(tmp_path / "deleted", dbs / "part1")
    assert ok("info", tmp_path / "deleted", env=env).stdout.count("n_samples=2") == 1
    # append --gpu without a device is an error, never the host loop
    res = run("append", dbs / "part1", *PART2, "--gpu", "-o", tmp_path / "x", env=env)
    assert res.returncode != 0 and not os.path.exists(tmp_path / "x.skm")
