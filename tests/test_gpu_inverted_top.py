"""`sketchlib inverted query --top N` and skl_inverted_query_top on the MI355X (csrc/inv_top.hip; the reference's
identification query, src/lib.rs:1019-1109).

Hit r of a query is the indexed sample with the r-th largest key (count << 32) | index: counts descend, and at equal count the
HIGHER .ski index comes first (the reference's stable ascending sort followed by reverse()).  The ABI is compared with numpy's
argsort of those keys, exactly; the CLI with lines derived from the reference's match-count golden."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REF_FIXTURES
from helpers import FIXTURE_NAMES
from test_gpu_inverted_query import CLI, clustered, queries_for
from test_inverted_cli_cpu import ski_decode

pytestmark = pytest.mark.gpu

PAD = 0xFFFFFFFF


def match_counts(R, Q):
    out = np.empty((Q.shape[0], R.shape[0]), dtype=np.uint32)
    for q0 in range(0, Q.shape[0], 16):    # (a few queries at a time: the comparison is nq x n x S)
        out[q0:q0 + 16] = (R[None, :, :] == Q[q0:q0 + 16, None, :]).sum(-1, dtype=np.uint32)
    return out


def expect_top(counts, top):
    """(ids, counts) [nq, top] from the match counts [nq, n]: argsort of the u64 keys, descending; padding past n."""
    nq, n = counts.shape
    keys = (counts.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)[None, :]
    order = np.argsort(keys, axis=1)[:, ::-1][:, :top]
    ids = np.full((nq, top), PAD, dtype=np.uint32)
    cnt = np.zeros((nq, top), dtype=np.uint32)
    ids[:, :order.shape[1]] = order
    cnt[:, :order.shape[1]] = np.take_along_axis(counts, order, axis=1)
    return ids, cnt


def check(ix, counts, Q, top, msg=""):
    ids, cnt = ix.top(Q, top)
    assert ids.dtype == np.uint32 and cnt.dtype == np.uint32 and ids.shape == cnt.shape == (Q.shape[0], top)
    want_ids, want_cnt = expect_top(counts, top)
    np.testing.assert_array_equal(ids, want_ids, err_msg=f"ids top={top} {msg}")
    np.testing.assert_array_equal(cnt, want_cnt, err_msg=f"counts top={top} {msg}")
    return ids, cnt


# ---------------------------------------------------------------------------
# ABI against numpy
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 10, 33, 1000, 2047, 2048])
@pytest.mark.parametrize("n,nq", [(1, 1), (63, 7), (257, 65), (700, 130)])
def test_abi_matches_numpy(skl, gpu_ctx, S, n, nq):
    rng = np.random.default_rng(S * 7919 + n * 31 + nq)
    R = clustered(rng, n, S)
    Q = queries_for(rng, R, nq)
    counts = match_counts(R, Q)
    ix = skl.Inverted(gpu_ctx, R)
    try:
        for top in (1, 5, 64, n, n + 3):
            ids, cnt = check(ix, counts, Q, top, f"S={S} n={n} nq={nq}")
            if top > n:     # the padding, spelled out
                assert (ids[:, n:] == PAD).all() and (cnt[:, n:] == 0).all()
                assert (ids[:, :n] != PAD).all()
    finally:
        ix.close()


def test_all_equal_counts_give_the_highest_indices(skl, gpu_ctx):
    S, n = 10, 700
    ix = skl.Inverted(gpu_ctx, np.zeros((n, S), dtype=np.uint16))
    try:
        ids, cnt = ix.top(np.zeros((2, S), dtype=np.uint16), 5)
    finally:
        ix.close()
    assert ids.tolist() == [[699, 698, 697, 696, 695]] * 2
    assert (cnt == S).all()


@pytest.mark.parametrize("last", [63, 64, 255, 256, 257])
def test_quota_of_equal_entries_ends_at(skl, gpu_ctx, last):
    """Two samples above the threshold and six at it, of which the quota takes three: the last one taken is entry `last` of
    the row counted from its top (the end of a wave, of a chunk of 256, the start of the next); the equal entries just
    below it are left out."""
    S, n, k = 10, 700, 3
    R = np.zeros((n, S), dtype=np.uint16)
    Q = np.ones((1, S), dtype=np.uint16)
    equal_at = [5, last // 2, last, last + 1, last + 2, 600]        # positions from the top of the row: index n - 1 - position
    above_at = [last + 5, 650]
    for p in equal_at:
        R[n - 1 - p, :k] = 1
    for p in above_at:
        R[n - 1 - p, :k + 2] = 1
    ix = skl.Inverted(gpu_ctx, R)
    try:
        ids, cnt = check(ix, match_counts(R, Q), Q, 5, f"last={last}")
    finally:
        ix.close()
    assert ids[0].tolist() == [n - 1 - p for p in above_at] + [n - 1 - p for p in equal_at[:3]]
    assert cnt[0].tolist() == [k + 2] * 2 + [k] * 3


def test_threshold_zero_fills_from_the_highest_indices(skl, gpu_ctx):
    S, n = 33, 700
    rng = np.random.default_rng(3)
    R = rng.integers(2, 65536, size=(n, S), dtype=np.uint16)
    Q = np.zeros((3, S), dtype=np.uint16)                  # shares nothing with any sample ...
    R[[10, 400], :4] = 0                                   # ... but these two
    R[400, 4] = 0
    R[698, :2] = 0                                         # (and, for the last query only, one of the highest indices)
    Q[:2, :2] = 1
    ix = skl.Inverted(gpu_ctx, R)
    try:
        ids, cnt = check(ix, match_counts(R, Q), Q, 5)
    finally:
        ix.close()
    assert ids[0].tolist() == [400, 10, 699, 698, 697] and cnt[0].tolist() == [3, 2, 0, 0, 0]
    assert ids[2].tolist() == [400, 10, 698, 699, 697] and cnt[2].tolist() == [5, 4, 2, 0, 0]


def test_digit_widths_agree(skl, gpu_ctx, set_switch):
    """SKL_INVQ_TOP_DIGIT_BITS = 1, 3, 8 walk the counts of S = 1 000 in 10, 4 and 2 passes, 11 in one."""
    S, n = 1000, 700
    rng = np.random.default_rng(17)
    R = clustered(rng, n, S)
    Q = queries_for(rng, R, 40)
    counts = match_counts(R, Q)
    results = {}
    for bits in (1, 3, 8, 11):
        set_switch("SKL_INVQ_TOP_DIGIT_BITS", bits)
        ix = skl.Inverted(gpu_ctx, R)
        try:
            results[bits] = [check(ix, counts, Q, top, f"bits={bits}") for top in (1, 64, 700)]
        finally:
            ix.close()
    for bits in (1, 3, 8):
        for a, b in zip(results[bits], results[11]):
            np.testing.assert_array_equal(a[0], b[0])
            np.testing.assert_array_equal(a[1], b[1])


def test_bands_equal_one_band(skl, gpu_ctx, set_switch):
    rng = np.random.default_rng(5)
    R = clustered(rng, 3000, 45)
    Q = queries_for(rng, R, 203)
    counts = match_counts(R, Q)
    ix = skl.Inverted(gpu_ctx, R)
    assert ix.band_queries(skl.INVQ_MATCH_COUNT) >= 203
    one = check(ix, counts, Q, 10, "one band")
    ix.close()
    set_switch("SKL_INVQ_BAND_BYTES", 20 * 3000 * 4)   # ~19 queries a band
    ix = skl.Inverted(gpu_ctx, R)
    assert 1 < ix.band_queries(skl.INVQ_MATCH_COUNT) < 30
    some = ix.top(Q, 10)
    ix.close()
    set_switch("SKL_INVQ_BAND_BYTES", 1)   # one query a band
    ix = skl.Inverted(gpu_ctx, R)
    assert ix.band_queries(skl.INVQ_MATCH_COUNT) == 1
    single = ix.top(Q[:9], 10)
    ix.close()
    for k in range(2):
        np.testing.assert_array_equal(some[k], one[k])
        np.testing.assert_array_equal(single[k], one[k][:9])


def test_many_chunks(skl, gpu_ctx):
    n = 1_400_000
    rng = np.random.default_rng(11)
    R = rng.integers(0, 8, size=(n, 16), dtype=np.uint16)
    Q = np.stack([R[0], R[777_777], R[n - 1]]).astype(np.uint16)
    counts = np.stack([(R == q).sum(1, dtype=np.uint32) for q in Q])
    ix = skl.Inverted(gpu_ctx, R)
    try:
        ids, cnt = check(ix, counts, Q, 50)
    finally:
        ix.close()
    assert (cnt[:, 0] == 16).all()
    assert 0 in ids[0] and 777_777 in ids[1] and n - 1 in ids[2]


def test_argument_errors_and_empty_cases(skl, gpu_ctx):
    R = np.zeros((7, 10), dtype=np.uint16)
    ix = skl.Inverted(gpu_ctx, R)
    try:
        for top in (0, 1025):
            with pytest.raises(skl.SklError) as e:
                ix.top(R[:2], top)
            assert e.value.code == skl.ERR_INVALID_ARG and "1 to 1024" in e.value.message
        ids, cnt = ix.top(R[:0], 4)                   # no query: nothing to do
        assert ids.shape == cnt.shape == (0, 4)
        ids, cnt = ix.top(R[:2], 1024)                # the limit itself
        assert ids[:, :7].tolist() == [[6, 5, 4, 3, 2, 1, 0]] * 2 and (ids[:, 7:] == PAD).all()
        assert (cnt[:, :7] == 10).all() and (cnt[:, 7:] == 0).all()
    finally:
        ix.close()
    empty = skl.Inverted(gpu_ctx, np.zeros((0, 10), dtype=np.uint16))
    try:
        ids, cnt = empty.top(R[:3], 4)
    finally:
        empty.close()
    assert (ids == PAD).all() and (cnt == 0).all() and ids.shape == (3, 4)


# ---------------------------------------------------------------------------
# CLI against the reference's match-count golden
# ---------------------------------------------------------------------------

HEADER = "Query\tSample\tMatches\tJaccard\tLabel\tMetadata"
SPECIES = {"R6.fa.gz": "A", "TIGR4.fa.gz": "A", "14412_3#82.contigs_velvet.fa.gz": "B", "14412_3#84.contigs_velvet.fa.gz": "B"}
METADATA = {"R6.fa.gz": "serotype 2", "TIGR4.fa.gz": "serotype 4", "14412_3#82.contigs_velvet.fa.gz": "group A",
            "14412_3#84.contigs_velvet.fa.gz": "group A, second"}


@pytest.fixture(scope="module")
def wd(tmp_path_factory, skl):
    d = tmp_path_factory.mktemp("invq_top_gpu")
    for f in FIXTURE_NAMES + ["rfile.txt"]:
        shutil.copy(os.path.join(REF_FIXTURES, f), d / f)
    (d / "species.txt").write_text("".join(f"{k}\t{v}\n" for k, v in SPECIES.items()))
    (d / "metadata.txt").write_text("".join(f"{k}\t{v}\n" for k, v in METADATA.items()))
    for out, extra in (("inverted", []), ("labelled", ["--species-names", "species.txt", "--metadata", "metadata.txt"])):
        res = subprocess.run([CLI, "inverted", "build", "-k", "21", "-s", "10", "-f", "rfile.txt", "-o", out, *extra],
                             cwd=d, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
    return d


def run_query(wd, *args, env=None):
    res = subprocess.run([CLI, "inverted", "query", *args], cwd=wd, capture_output=True, text=True, timeout=300,
                         env={**os.environ, **(env or {})})
    assert res.returncode == 0, res.stderr
    return res


def golden_hits(order, top):
    """{query: [(sample, count)]} in hit order for a .ski whose samples come in `order`, from the reference's match counts."""
    with open(os.path.join(REF_FIXTURES, "inverted_query_count.stdout")) as f:
        lines = f.read().splitlines()
    cols = lines[0].split("\t")[1:]
    hits = {}
    for line in lines[1:]:
        name, *values = line.split("\t")
        by_name = dict(zip(cols, map(int, values)))
        ranked = sorted(range(len(order)), key=lambda s: (by_name[order[s]], s), reverse=True)
        hits[name] = [(order[s], by_name[order[s]]) for s in ranked[:top]]
    return hits


def parse(stdout, S=10):
    lines = stdout.splitlines()
    assert lines[0] == HEADER
    rows = [line.split("\t") for line in lines[1:]]
    for row in rows:
        assert len(row) == 6
        c, j = int(row[2]), row[3]
        assert float(j) == c / (2 * S - c)                      # exactly: the f64 the reference computes
        assert "e" not in j.lower() and len(j) <= len(repr(c / (2 * S - c)))     # fixed notation, shortest digits
    return rows


def input_names(wd):
    with open(wd / "rfile.txt") as f:
        return [line.split("\t")[0] for line in f if line.strip()]


def test_cli_top3_follows_the_golden(wd):
    out = run_query(wd, "-f", "rfile.txt", "inverted.ski", "--top", "3").stdout
    rows = parse(out)
    want = golden_hits(FIXTURE_NAMES, 3)
    names = input_names(wd)
    assert [r[0] for r in rows] == [q for q in names for _ in range(3)]          # queries in input order, three lines each
    for q in names:
        assert [(r[1], int(r[2])) for r in rows if r[0] == q] == want[q]
    # R6's counts are 0 0 10 7: the third hit is the HIGHER of the two indices with count 0
    assert [r[1] for r in rows if r[0] == "R6.fa.gz"] == ["R6.fa.gz", "TIGR4.fa.gz", "14412_3#84.contigs_velvet.fa.gz"]
    assert [r[3] for r in rows if r[0] == "R6.fa.gz"] == ["1", "0.5384615384615384", "0"]
    assert all(r[4] == "" and r[5] == "" for r in rows)                          # no labels or metadata in this .ski
    assert all(line.endswith("\t\t") for line in out.splitlines()[1:])


def test_cli_top_above_the_index_prints_every_sample(wd):
    rows = parse(run_query(wd, "-f", "rfile.txt", "inverted.ski", "--top", "9").stdout)
    want = golden_hits(FIXTURE_NAMES, 9)
    names = input_names(wd)
    assert len(rows) == 4 * len(names)
    for q in names:
        assert [(r[1], int(r[2])) for r in rows if r[0] == q] == want[q]


def test_cli_output_file_threads_gpu_sketching_and_timing(wd):
    out = run_query(wd, "-f", "rfile.txt", "inverted.ski", "--top", "3").stdout
    run_query(wd, "-f", "rfile.txt", "inverted.ski", "--top", "3", "-o", "out.txt", "--threads", "3")
    assert (wd / "out.txt").read_text() == out
    res = run_query(wd, "-f", "rfile.txt", "inverted.ski", "--top", "3", "--gpu", "--query-type", "match-count",
                    env={"SKL_CLI_TIMING": "1"})
    assert res.stdout == out
    assert "TIMING inverted query: load=" in res.stderr
    # sequence files instead of a list: a query's name is its file name
    two = run_query(wd, "inverted.ski", "R6.fa.gz", "TIGR4.fa.gz", "--top", "3").stdout.splitlines()
    assert two == [HEADER] + [line for line in out.splitlines()[1:] if line.split("\t")[0] in ("R6.fa.gz", "TIGR4.fa.gz")]


def test_cli_labels_and_metadata_of_a_reordered_ski(wd):
    order = ski_decode(wd / "labelled.ski")["sample_names"]
    assert order[:2] == ["R6.fa.gz", "TIGR4.fa.gz"]                               # the labels put the pneumococci first
    rows = parse(run_query(wd, "-f", "rfile.txt", "labelled.ski", "--top", "3").stdout)
    want = golden_hits(order, 3)
    for q in input_names(wd):
        assert [(r[1], int(r[2])) for r in rows if r[0] == q] == want[q]
    for r in rows:
        assert r[4] == SPECIES[r[1]] and r[5] == METADATA[r[1]]
