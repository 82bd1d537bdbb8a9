"""`sketchlib dist <ref> [<query>] --pairs <FILE>` end to end: the listing of an earlier `dist --knn` run is a valid pairs
file and comes back byte for byte; an arbitrary list gives the matching lines of the dense listing, names in the order
given; errors and the empty file."""
import os
import subprocess

import pytest

from conftest import REF_FIXTURES, ROOT
from helpers import FIXTURE_NAMES

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")
SKETCHES1 = os.path.join(REF_FIXTURES, "sketches1")


def dist(*args, ok=True):
    res = subprocess.run([CLI, "dist", *args], capture_output=True, text=True, timeout=300)
    if ok:
        assert res.returncode == 0, res.stderr
        return res.stdout
    return res


@pytest.fixture(scope="module")
def sketch_db(tmp_path_factory):
    """The four reference fixtures sketched by the project's CPU sketcher, as rfile.txt lists them (tests/distance.rs:270-328)."""
    db = str(tmp_path_factory.mktemp("pairs_db") / "sketch_db")
    subprocess.check_call([CLI, "sketch", "-o", db, "--k-seq", "17,31,4", "-s", "10000", "-f", "rfile.txt"], cwd=REF_FIXTURES,
                          stderr=subprocess.DEVNULL)
    return db


@pytest.mark.parametrize("flags,golden", [((), "dists_knn_ca.stdout"), (("-k", "21"), "dists_knn_jaccard.stdout"),
                                          (("-k", "21", "--ani"), "dists_knn_ani.stdout")])
def test_knn_listing_round_trip(gpu_ctx, sketch_db, tmp_path, flags, golden):
    knn = dist(sketch_db, "--knn", "1", *flags)
    assert len(knn.splitlines()) == 4
    edges = tmp_path / "edges.txt"
    edges.write_text(knn)
    assert dist(sketch_db, "--pairs", str(edges), *flags) == knn
    # through a file, formatted by several threads
    out = tmp_path / "pairs_out.txt"
    assert dist(sketch_db, "--pairs", str(edges), "-o", str(out), "--threads", "3", *flags) == ""
    assert out.read_text() == knn
    # the CPU-sketched database reproduces the reference's golden listing, so the golden itself is a pairs file that comes back
    expected = open(os.path.join(REF_FIXTURES, golden)).read()
    assert knn == expected
    assert dist(sketch_db, "--pairs", os.path.join(REF_FIXTURES, golden), *flags) == expected


def test_arbitrary_list_matches_the_dense_listing(gpu_ctx, tmp_path):
    n0, n1, n2, n3 = FIXTURE_NAMES
    dense = {tuple(l.split("\t")[:2]): l.split("\t")[2] for l in dist(SKETCHES1, "-k", "31").splitlines()}
    assert len(dense) == 6
    listed = [(n2, n3), (n0, n1), (n3, n2), (n0, n3), (n0, n1), (n1, n2), (n3, n0)]     # arbitrary order, a repeat, two reversed
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("".join(f"{a}\t{b}\n" for a, b in listed))
    expected = "".join(f"{a}\t{b}\t{dense[(a, b)] if (a, b) in dense else dense[(b, a)]}\n" for a, b in listed)
    assert dist(SKETCHES1, "-k", "31", "--pairs", str(pairs)) == expected
    assert "0.33789062" in expected and expected.count("\t1\n") >= 2        # ((2, 3) = 0.33789062, (0, 2) = 1)
    # ANI of the same pairs
    dense_ani = {tuple(l.split("\t")[:2]): l.split("\t")[2] for l in dist(SKETCHES1, "-k", "31", "--ani").splitlines()}
    expected = "".join(f"{a}\t{b}\t{dense_ani[(a, b)] if (a, b) in dense_ani else dense_ani[(b, a)]}\n" for a, b in listed)
    assert dist(SKETCHES1, "-k", "31", "--ani", "--pairs", str(pairs)) == expected
    # with a query database: name1 is a reference sample, name2 a query sample; (x, x) pairs exist there
    cross = {tuple(l.split("\t")[:2]): l.split("\t")[2] for l in dist(SKETCHES1, SKETCHES1, "-k", "31").splitlines()}
    assert len(cross) == 16
    listed += [(n1, n1), (n3, n3)]
    pairs.write_text("".join(f"{a}\t{b}\n" for a, b in listed))
    expected = "".join(f"{a}\t{b}\t{cross[(a, b)]}\n" for a, b in listed)
    assert dist(SKETCHES1, SKETCHES1, "-k", "31", "--pairs", str(pairs)) == expected
    assert expected.endswith(f"{n3}\t{n3}\t0\n")


def test_core_accessory_list_matches_the_dense_listing(gpu_ctx, sketch_db, tmp_path):
    lines = dist(sketch_db).splitlines()
    dense = {tuple(l.split("\t")[:2]): l.split("\t")[2:] for l in lines}
    assert len(dense) == 6 and all(len(v) == 2 for v in dense.values())
    listed = [k for k in reversed(list(dense))] + [(b, a) for a, b in dense]
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("".join(f"{a}\t{b}\tanything\telse\n" for a, b in listed))
    expected = "".join("\t".join([a, b] + (dense[(a, b)] if (a, b) in dense else dense[(b, a)])) + "\n" for a, b in listed)
    assert dist(sketch_db, "--pairs", str(pairs)) == expected


def test_errors(gpu_ctx, tmp_path):
    n0, n1, _n2, n3 = FIXTURE_NAMES
    pairs = tmp_path / "pairs.txt"
    pairs.write_text(f"{n0}\t{n1}\n{n3}\tno_such_sample.fa\n")
    res = dist(SKETCHES1, "-k", "31", "--pairs", str(pairs), ok=False)
    assert res.returncode == 1 and res.stdout == ""
    assert "line 2" in res.stderr and '"no_such_sample.fa"' in res.stderr and str(pairs) in res.stderr
    res = dist(SKETCHES1, "-k", "31", "--pairs", str(tmp_path / "missing.txt"), ok=False)
    assert res.returncode == 1 and "Unable to open" in res.stderr
    pairs.write_text(f"{n0}\t{n1}\n")
    res = dist(SKETCHES1, "-k", "31", "--pairs", str(pairs), "--knn", "1", ok=False)
    assert res.returncode == 2 and "'--pairs <FILE>' cannot be used with '--knn <KNN>'" in res.stderr
    subset = tmp_path / "subset.txt"
    subset.write_text(f"{n0}\n{n1}\n")
    res = dist(SKETCHES1, "-k", "31", "--pairs", str(pairs), "--subset", str(subset), ok=False)
    assert res.returncode == 2 and "'--pairs <FILE>' cannot be used with '--subset <SUBSET>'" in res.stderr
    # core/accessory distances of a database with one k-mer length: the error of the dense call
    res = dist(SKETCHES1, "--pairs", str(pairs), ok=False)
    assert res.returncode == 101 and "Need at least two k-mer lengths" in res.stderr


def test_empty_file(gpu_ctx, tmp_path):
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("")
    assert dist(SKETCHES1, "-k", "31", "--pairs", str(pairs)) == ""
    pairs.write_text("\n\n")
    out = tmp_path / "out.txt"
    assert dist(SKETCHES1, "-k", "31", "--pairs", str(pairs), "-o", str(out)) == ""
    assert out.read_text() == ""
