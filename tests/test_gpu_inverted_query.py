"""`sketchlib inverted query` and skl_inverted_query on the MI355X (src/inverted.rs:229-269, src/lib.rs:605-680).

count(q, s) = #{ b : R[s][b] == q[b] } over the full 16-bit bin values; match-count prints the counts,
any-bins the samples with count > 0, all-bins those with count == S, in ascending .ski index; the query
itself is not excluded.  The CLI is pinned to the reference's goldens (tests/inverted.rs:169-241, compared
unordered as there), the ABI to numpy."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REF_FIXTURES, ROOT
from helpers import FIXTURE_NAMES
from test_inverted_cli_cpu import ski_decode

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")
MODES = ("match-count", "any-bins", "all-bins")


def expect(R, Q, mode):
    counts = (R[None, :, :] == Q[:, None, :]).sum(-1, dtype=np.uint32)
    if mode == "match-count":
        return counts
    return counts > 0 if mode == "any-bins" else counts == R.shape[1]


def query(skl, ctx, R, Q, mode):
    code = {"match-count": skl.INVQ_MATCH_COUNT, "any-bins": skl.INVQ_ANY_BINS, "all-bins": skl.INVQ_ALL_BINS}[mode]
    ix = skl.Inverted(ctx, R)
    try:
        out = ix.query(Q, code)
    finally:
        ix.close()
    if mode == "match-count":
        return out
    # bits past n in the last word must be clear
    n = R.shape[0]
    full = skl.unpack_bitmap(out, out.shape[1] * 64)
    assert not full[:, n:].any()
    return full[:, :n]


def clustered(rng, n, S, n_clusters=5):
    """Samples around a few centres, each bin kept with a per-sample probability from 0 to 1 and otherwise drawn
    from a small alphabet (so that unrelated samples still share some bins): counts cover 0..S."""
    centres = rng.integers(0, 65536, size=(n_clusters, S), dtype=np.uint16)
    keep = rng.random(n)[:, None]
    own = rng.integers(0, 4, size=(n, S), dtype=np.uint16) * 16411
    R = np.where(rng.random((n, S)) < keep, centres[rng.integers(0, n_clusters, n)], own).astype(np.uint16)
    return R


def queries_for(rng, R, nq):
    """Copies of indexed samples (count S), mutated copies, and unrelated sketches (count 0 in most bins)."""
    n, S = R.shape
    Q = R[rng.integers(0, n, nq)].copy()
    kind = rng.integers(0, 3, nq)
    flip = rng.random((nq, S)) < rng.random(nq)[:, None]
    Q = np.where((kind == 1)[:, None] & flip, Q ^ np.uint16(0x8001), Q)
    Q[kind == 2] = rng.integers(0, 65536, size=(int((kind == 2).sum()), S), dtype=np.uint16)
    return Q.astype(np.uint16)


# ---------------------------------------------------------------------------
# CLI against the reference's goldens
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wd(tmp_path_factory, skl):
    d = tmp_path_factory.mktemp("invq_gpu")
    for f in FIXTURE_NAMES + ["rfile.txt"]:
        shutil.copy(os.path.join(REF_FIXTURES, f), d / f)
    res = subprocess.run([CLI, "inverted", "build", "-k", "21", "-s", "10", "-f", "rfile.txt", "-o", "inverted"],
                         cwd=d, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return d


def run_query(wd, *args):
    res = subprocess.run([CLI, "inverted", "query", *args], cwd=wd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    return res.stdout


@pytest.mark.parametrize("mode,golden", [(None, "inverted_query_count.stdout"), ("any-bins", "inverted_query_any.stdout"),
                                         ("all-bins", "inverted_query_all.stdout")])
def test_goldens(wd, mode, golden):
    extra = [] if mode is None else ["--query-type", mode]
    out = run_query(wd, "-v", "-f", "rfile.txt", "inverted.ski", *extra)
    with open(os.path.join(REF_FIXTURES, golden)) as f:
        want = f.read()
    got_lines, want_lines = out.splitlines(), want.splitlines()
    assert got_lines[0] == want_lines[0]
    assert sorted(got_lines[1:]) == sorted(want_lines[1:])
    # rows in input order (rfile.txt)
    with open(wd / "rfile.txt") as f:
        names = [line.split("\t")[0] for line in f if line.strip()]
    assert [line.split("\t")[0] for line in got_lines[1:]] == names
    # -o writes the same bytes
    run_query(wd, "-f", "rfile.txt", "inverted.ski", "-o", "out.txt", "--threads", "3", *extra)
    assert (wd / "out.txt").read_text() == out


def test_seq_files_form_and_timing(wd):
    res = subprocess.run([CLI, "inverted", "query", "inverted.ski", "R6.fa.gz", "TIGR4.fa.gz"], cwd=wd,
                         capture_output=True, text=True, timeout=300, env={**os.environ, "SKL_CLI_TIMING": "1"})
    assert res.returncode == 0, res.stderr
    with open(os.path.join(REF_FIXTURES, "inverted_query_count.stdout")) as f:
        want = {line.split("\t")[0]: line for line in f.read().splitlines()[1:]}
    # a query's name is its file name, as in `inverted build`
    assert res.stdout.splitlines()[1:] == [want["R6.fa.gz"], want["TIGR4.fa.gz"]]
    assert "TIMING inverted query: load=" in res.stderr
    for phase in ("sketch=", "device=", "query=", "write="):
        assert phase in res.stderr


def test_reordered_ski_follows_ski_order(wd):
    # labels put the two pneumococci first: the .ski lists R6, TIGR4, then the others
    (wd / "species.txt").write_text("R6.fa.gz\tA\nTIGR4.fa.gz\tA\n14412_3#82.contigs_velvet.fa.gz\tB\n"
                                    "14412_3#84.contigs_velvet.fa.gz\tB\n")
    res = subprocess.run([CLI, "inverted", "build", "-k", "21", "-s", "10", "-f", "rfile.txt", "-o", "reordered",
                          "--species-names", "species.txt"], cwd=wd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    order = ski_decode(wd / "reordered.ski")["sample_names"]
    assert order[:2] == ["R6.fa.gz", "TIGR4.fa.gz"]
    plain = run_query(wd, "-f", "rfile.txt", "inverted.ski").splitlines()
    re = run_query(wd, "-f", "rfile.txt", "reordered.ski").splitlines()
    assert re[0] == "Query\t" + "\t".join(order)
    cols = plain[0].split("\t")[1:]
    for a, b in zip(plain[1:], re[1:]):
        a, b = a.split("\t"), b.split("\t")
        assert a[0] == b[0]
        by_name = dict(zip(cols, a[1:]))
        assert b[1:] == [by_name[c] for c in order]
    anyb = run_query(wd, "-f", "rfile.txt", "reordered.ski", "--query-type", "any-bins").splitlines()
    assert anyb[0] == "Query\tMatches"
    for line in anyb[1:]:
        matches = line.split("\t")[1].split(",")
        assert matches == sorted(matches, key=order.index)


# ---------------------------------------------------------------------------
# ABI against numpy
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 10, 31, 32, 33, 1000, 1001])
@pytest.mark.parametrize("n,nq", [(1, 1), (63, 7), (257, 65), (700, 130)])
def test_abi_matches_numpy(skl, gpu_ctx, S, n, nq):
    rng = np.random.default_rng(S * 7919 + n * 31 + nq)
    R = clustered(rng, n, S)
    Q = queries_for(rng, R, nq)
    for mode in MODES:
        got = query(skl, gpu_ctx, R, Q, mode)
        np.testing.assert_array_equal(got, expect(R, Q, mode), err_msg=f"{mode} S={S} n={n} nq={nq}")
    if n > 1 and S > 1:
        counts = expect(R, Q, "match-count")
        assert counts.min() == 0 and counts.max() == S


@pytest.mark.parametrize("pair", [(0x0000, 0x8000), (0x3FFF, 0x7FFF), (0x0000, 0x4000), (0x8000, 0xC000)])
def test_bits_14_and_15_count(skl, gpu_ctx, pair):
    """Index and query differ only in bit 14 or bit 15: no bin matches (a 14-plane comparison would say all do)."""
    a, b = pair
    for S in (10, 33):
        R = np.full((5, S), a, dtype=np.uint16)
        Q = np.full((2, S), b, dtype=np.uint16)
        assert not query(skl, gpu_ctx, R, Q, "match-count").any()
        assert not query(skl, gpu_ctx, R, Q, "any-bins").any()
        assert not query(skl, gpu_ctx, R, Q, "all-bins").any()
        assert (query(skl, gpu_ctx, R, R[:2], "match-count") == S).all()


@pytest.mark.parametrize("S", [10, 33])
def test_tail_bins_never_count(skl, gpu_ctx, S):
    R = np.zeros((70, S), dtype=np.uint16)
    Q = np.full((3, S), 0xFFFF, dtype=np.uint16)
    assert not query(skl, gpu_ctx, R, Q, "match-count").any()
    assert not query(skl, gpu_ctx, R, Q, "any-bins").any()
    assert not query(skl, gpu_ctx, R, Q, "all-bins").any()
    same = np.zeros((2, S), dtype=np.uint16)
    assert (query(skl, gpu_ctx, R, same, "match-count") == S).all()
    assert query(skl, gpu_ctx, R, same, "all-bins").all()


def test_bands_equal_one_band(skl, gpu_ctx, set_switch):
    rng = np.random.default_rng(5)
    R = clustered(rng, 3000, 45)
    Q = queries_for(rng, R, 203)
    one = {m: query(skl, gpu_ctx, R, Q, m) for m in MODES}
    ix = skl.Inverted(gpu_ctx, R)
    assert ix.band_queries(skl.INVQ_MATCH_COUNT) >= 203
    ix.close()
    set_switch("SKL_INVQ_BAND_BYTES", 20 * 3000 * 4)   # ~19 queries a band
    ix = skl.Inverted(gpu_ctx, R)
    assert 1 < ix.band_queries(skl.INVQ_MATCH_COUNT) < 30
    ix.close()
    for m in MODES:
        np.testing.assert_array_equal(query(skl, gpu_ctx, R, Q, m), one[m], err_msg=m)
        np.testing.assert_array_equal(one[m], expect(R, Q, m), err_msg=m)
    set_switch("SKL_INVQ_BAND_BYTES", 1)   # one query a band
    for m in MODES:
        np.testing.assert_array_equal(query(skl, gpu_ctx, R, Q[:9], m), one[m][:9], err_msg=m)


def test_more_samples_than_cand_gen_takes(skl, gpu_ctx):
    n = 1_400_000
    assert n > skl.load().skl_shared_bins_max_samples()
    rng = np.random.default_rng(11)
    R = rng.integers(0, 8, size=(n, 16), dtype=np.uint16)
    Q = np.stack([R[0], R[n - 1], R[777_777] ^ np.uint16(0x4000)]).astype(np.uint16)
    for mode in MODES:
        np.testing.assert_array_equal(query(skl, gpu_ctx, R, Q, mode), expect(R, Q, mode), err_msg=mode)
