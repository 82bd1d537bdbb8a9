"""The lean early-break epilogue after its load chain was shortened (epilogue.hip coreacc_epilogue_lean_kernel): the workgroup's
row slices are requested at kernel entry beside the counts -- every workgroup stages them, one barrier -- and the trip-ahead
iterator never requests under a condition (requests past the last pair re-read one address and are not counted).

Every case compares the WHOLE output with the oracle: max |delta| == 0 without a completeness correction, <= 1e-6 with one,
and the (1, 1) pattern exactly.  The sketches are random (chance matches only) with PLANTED relatives: sample c copies ~60 % of
sample a's bins at its first m k-mer lengths, so that the pair (a, c) passes the reference's test at exactly m lengths and leaves
its loop after 2, 3, 4 or 5 of them.

The library takes the early break from 65 536 row x column pairs on (eb_plan.hpp EB_MIN_PAIR_SPACE), and stages the rows only
where the SAMPLED share of pairs still in the running -- the same number of samples from every block of 256 x 256 sample ids,
pooled -- is at least 3 % (dense_plan.hpp); a forced number of lengths carries no share and never stages.  The shapes below
the floor (n = 40 ... 192, the small cross matrices) check the same data through the form the library picks there.  The
cases that are about the staging and the iterator run at n = 256 (one block: the sampled share is the true one, kept well
above 3 % by a cluster of relatives) or on cross matrices whose blocks all hold the same share, and each of them asserts from
skl_ctx_last_kernel that the lean kernel ran with its rows staged."""
import numpy as np
import pytest

from sketchlib.rust_amd import synth

pytestmark = pytest.mark.gpu

KMERS = [15, 19, 23, 27, 31]
NK = len(KMERS)


def _planted(n, ss64, plants, seed=3):
    """Random 14-bit bins [n, NK, ss64 * 64]; plants = [(a, c, m)]: sample c shares ~60 % of a's bins at lengths 0 .. m - 1."""
    rng = np.random.default_rng(seed)
    nb = ss64 * 64
    vals = rng.integers(0, 1 << 14, size=(n, NK, nb), dtype=np.uint16)
    for a, c, m in plants:
        keep = rng.random((m, nb)) < 0.6
        vals[c, :m] = np.where(keep, vals[a, :m], vals[c, :m])
    return np.ascontiguousarray(synth.bitslice(vals).reshape(n, NK * ss64 * synth.BBITS))


def _plants(n):
    """Row 1 has 16 consecutive related columns (all five lengths: in the running whatever is counted); pairs leaving after 2, 3, 4
    and 5 lengths near the start, in the middle and among the last rows (where a workgroup of 256 pairs spans many rows)."""
    out = [(1, c, 5) for c in range(8, 24)]
    out += [(0, 5, 2), (0, 6, 3), (0, 7, 4), (2, 30, 5), (n // 2, n // 2 + 3, 3), (n // 2, n - 2, 4)]
    out += [(n - 9, n - 4, 2), (n - 8, n - 3, 3), (n - 7, n - 2, 4), (n - 6, n - 1, 5), (n - 3, n - 1, 3)]
    return out


def _passed_lengths(oracle, o, ss64):
    """The oracle's own bin-match counts: how many leading lengths pass the reference's test.  Valid for bimodal data only -- a
    planted length shares 0.6 x bins (0.36 between two copies of one sample, 0.24 with a sample planted twice), a chance length a
    handful -- and asserted to be so."""
    same = oracle.self_binmatch(o, threads=8)
    nb, expected = ss64 * 64, (ss64 * 64) >> 14
    assert not ((same > 24 + expected) & (same < nb // 8)).any()
    ok = same > expected
    return np.cumprod(ok, axis=1).sum(axis=1)


def _check(got, exp, comp=False):
    if comp:
        assert np.max(np.abs(got.astype(np.float64) - exp.astype(np.float64))) <= 1e-6
    else:
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), np.argwhere(got != exp)[:5]
    assert np.array_equal((got[:, 0] == 1.0) & (got[:, 1] == 1.0), (exp[:, 0] == 1.0) & (exp[:, 1] == 1.0))


_REF = {}


def _reference(oracle, n, ss64):
    """(bins, oracle sketches, expected matrix), computed once per shape and shared."""
    key = (n, ss64)
    if key not in _REF:
        bins = _planted(n, ss64, _plants(n))
        o = oracle.Sketches(bins, n, KMERS, ss64)
        exp = oracle.self_dists_all(o, oracle.COREACC, threads=8).reshape(-1, 2)
        exp.setflags(write=False)
        _REF[key] = (bins, o, exp)
    return _REF[key]


def _waves_are_as_planted(oracle, o, ss64):
    """Some wave (64 consecutive flat pairs) holds >= 12 pairs still in the running after two lengths, some wave exactly one."""
    passed = _passed_lengths(oracle, o, ss64)
    assert {2, 3, 4, 5} <= set(np.unique(passed).tolist())
    live = passed >= 2
    pad = (-live.size) % 64
    per_wave = np.concatenate([live, np.zeros(pad, dtype=bool)]).reshape(-1, 64).sum(axis=1)
    assert per_wave.max() >= 12 and (per_wave == 1).any(), np.bincount(per_wave)


@pytest.mark.parametrize("n", [192, 272])
def test_every_leaving_position_sampled_choice(oracle, skl, gpu_ctx, n):
    ss64 = 64
    bins, o, exp = _reference(oracle, n, ss64)
    _waves_are_as_planted(oracle, o, ss64)
    g = gpu_ctx.sketches(bins, n, KMERS, ss64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    if n >= 256:
        assert "early break: " in gpu_ctx.last_kernel(), gpu_ctx.last_kernel()
    g.close()


@pytest.mark.ab_library
@pytest.mark.parametrize("ke", [2, 3, 4])
@pytest.mark.parametrize("n", [192, 272])
def test_every_leaving_position_forced_lengths(oracle, skl, gpu_ctx, monkeypatch, n, ke):
    ss64 = 64
    bins, o, exp = _reference(oracle, n, ss64)
    monkeypatch.setenv("SKL_EARLY_BREAK", str(ke))
    gpu_ctx.reload_env()
    g = gpu_ctx.sketches(bins, n, KMERS, ss64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    if n >= 256:
        assert "early break: %d of 5" % ke in gpu_ctx.last_kernel() and "[lean epilogue" in gpu_ctx.last_kernel(), gpu_ctx.last_kernel()
    g.close()


@pytest.mark.parametrize("n", [96, 264])
@pytest.mark.parametrize("ss64", [32, 64, 65, 157])
def test_one_two_and_more_trips(oracle, skl, gpu_ctx, n, ss64):
    """1 trip, 2 trips, 3 trips with the last one partial, and `sketch -s 10000`'s size (rows beyond the LDS copy)."""
    bins, o, exp = _reference(oracle, n, ss64)
    g = gpu_ctx.sketches(bins, n, KMERS, ss64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    g.close()


@pytest.mark.parametrize("n", [40, 70, 258])
def test_workgroups_spanning_many_rows(oracle, skl, gpu_ctx, n):
    """Rows shorter than 256 pairs (a workgroup spans 4+ rows: row_off >= 2 reads the row from memory) / a first row that fills a
    workgroup by itself.  At n = 258 the early break is taken and the matrix' last rows hold planted pairs."""
    bins, o, exp = _reference(oracle, n, 64)
    g = gpu_ctx.sketches(bins, n, KMERS, 64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    if n >= 256:
        assert "early break: " in gpu_ctx.last_kernel(), gpu_ctx.last_kernel()
    g.close()


def test_rows_band_that_starts_mid_row_and_cross_forms(oracle, skl, gpu_ctx):
    n, ss64 = 272, 64
    bins, o, exp = _reference(oracle, n, ss64)
    g = gpu_ctx.sketches(bins, n, KMERS, ss64)
    part = skl.self_dists_rows(gpu_ctx, g, g.set_k(), 1, n - 5)
    lo = 1 * n - 1 * 2 // 2
    _check(part, exp[lo:lo + part.shape[0]])
    g.close()
    # cross matrices: columns = samples of the same planted set, so related pairs exist; nB_cols < 64 locates every lane's pair itself
    for rows, cols in [(64, 130), (3, 50), (520, 130), (1100, 60)]:
        m = max(rows, cols)
        big = _planted(m, ss64, _plants(max(min(rows, cols), 32)), seed=5)
        g_r, g_q = gpu_ctx.sketches(big[:rows], rows, KMERS, ss64), gpu_ctx.sketches(big[:cols], cols, KMERS, ss64)
        o_r, o_q = oracle.Sketches(big[:rows], rows, KMERS, ss64), oracle.Sketches(big[:cols], cols, KMERS, ss64)
        want = oracle.cross_dists_all(o_r, o_q, oracle.COREACC, threads=8).reshape(-1, 2)
        assert ((want[:, 0] != 1.0) | (want[:, 1] != 1.0)).any()
        _check(skl.cross_dists_all(gpu_ctx, g_r, g_q, g_r.set_k()).reshape(-1, 2), want)
        if rows * cols >= 65536:
            assert "early break: " in gpu_ctx.last_kernel(), gpu_ctx.last_kernel()
        g_r.close()
        g_q.close()


@pytest.mark.parametrize("above_one", [False, True])
def test_completeness(oracle, skl, gpu_ctx, above_one):
    """16 384 bins (expected_samebits = 1: counts between the chance level and min_alive exist) with values in (0, 1]; and a
    vector with a value above 1, which keeps the general kernel."""
    n, ss64 = 272, 256
    bins = _planted(n, ss64, _plants(n), seed=7)
    comp = np.random.default_rng(11).uniform(0.4, 1.0, n)
    comp[::5] = 1.0
    if above_one:
        comp[3] = 1.25
    o = oracle.Sketches(bins, n, KMERS, ss64, completeness=comp)
    exp = oracle.self_dists_all(o, oracle.COREACC, cutoff=0.3, threads=8).reshape(-1, 2)
    same = oracle.self_binmatch(o, threads=8)
    assert ((same[:, 0] > 1) & (same[:, 0] <= 3)).any()      # (between the chance level and what passes uncorrected)
    g = gpu_ctx.sketches(bins, n, KMERS, ss64, completeness=comp)
    got = skl.self_dists_all(gpu_ctx, g, g.set_k(cutoff=0.3))
    name = gpu_ctx.last_kernel()
    _check(got, exp, comp=True)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    g.close()
    assert "early break: " in name and ("[lean epilogue" in name) == (not above_one), name


def _disjoint(n, ss64, seed):
    """Unrelated for certain: sample s holds only bin values = s (mod n), so no two samples share a bin at any length."""
    rng = np.random.default_rng(seed)
    nb = ss64 * 64
    r = rng.integers(0, (1 << 14) // n, size=(n, NK, nb)).astype(np.uint16)
    return (r * np.uint16(n) + np.arange(n, dtype=np.uint16)[:, None, None]).astype(np.uint16)


@pytest.mark.parametrize("relatives", [0, 64])
def test_workgroups_without_a_live_pair(oracle, skl, gpu_ctx, relatives):
    """1 024 bins, all unrelated: everything is (1, 1).  (Random sketches of 1 024 bins do share a bin at three lengths now and
    then -- the oracle finds fits among them -- so the samples here hold disjoint bin values.)  With no pair in the running the
    plan does not ask for the rows, so the second case makes the first 64 of 256 samples relatives of one another (one block,
    6.2 % of its pairs): every workgroup stages its rows, and those of the rows from 64 on use none."""
    n, ss64 = (256 if relatives else 300), 16
    vals = _disjoint(n, ss64, seed=13)
    if relatives:
        keep = np.random.default_rng(17).random((relatives, NK, ss64 * 64)) < 0.7
        vals[:relatives] = np.where(keep, vals[0], vals[:relatives])
    bins = np.ascontiguousarray(synth.bitslice(vals).reshape(n, NK * ss64 * synth.BBITS))
    o = oracle.Sketches(bins, n, KMERS, ss64)
    exp = oracle.self_dists_all(o, oracle.COREACC, threads=8).reshape(-1, 2)
    first_unrelated = relatives * n - relatives * (relatives + 1) // 2 if relatives else 0
    assert np.all(exp[first_unrelated:] == 1.0) and (relatives == 0 or np.any(exp[:first_unrelated] != 1.0))
    g = gpu_ctx.sketches(bins, n, KMERS, ss64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    if relatives:
        _ran_staged(gpu_ctx)
    g.close()


# ---- the cases that prove the staging and the iterator ran ----

STAGED = "[row slices staged in LDS]"


def _ran_staged(gpu_ctx, lengths=None):
    name = gpu_ctx.last_kernel()
    assert "[lean epilogue" in name and STAGED in name, name
    if lengths is not None:
        assert "early break: %d of 5" % lengths in name, name


def _clustered(n, ss64, plants, clusters, seed=21):
    """_planted plus clusters = [(first, count, m, keep)]: `count` samples from `first` on copy `keep` of one parent's bins at their
    first m lengths (two members share keep^2 of the bins)."""
    rng = np.random.default_rng(seed)
    nb = ss64 * 64
    vals = rng.integers(0, 1 << 14, size=(n, NK, nb), dtype=np.uint16)
    for first, count, m, keep in clusters:
        parent = rng.integers(0, 1 << 14, size=(m, nb), dtype=np.uint16)
        mask = rng.random((count, m, nb)) < keep
        vals[first:first + count, :m] = np.where(mask, parent[None], vals[first:first + count, :m])
    for a, c, m in plants:
        keep = rng.random((m, nb)) < 0.6
        vals[c, :m] = np.where(keep, vals[a, :m], vals[c, :m])
    return np.ascontiguousarray(synth.bitslice(vals).reshape(n, NK * ss64 * synth.BBITS))


def _self_case(oracle, key, n, ss64, plants, clusters):
    if key not in _REF:
        bins = _clustered(n, ss64, plants, clusters)
        o = oracle.Sketches(bins, n, KMERS, ss64)
        exp = oracle.self_dists_all(o, oracle.COREACC, threads=8).reshape(-1, 2)
        exp.setflags(write=False)
        _REF[key] = (bins, o, exp)
    return _REF[key]


N1 = 256                                    # one block of the sampler: 256 x 256 = the floor
CLUSTER = [(150, 40, 5, 0.8)]               # 780 pairs in the running at every length: + 2.4 % on top of chance


def test_staged_every_leaving_position(oracle, skl, gpu_ctx):
    """n = 256, 4 096 bins: 4.8 % of random pairs share a bin at both counted lengths, the cluster adds 2.4 %: two lengths
    counted, rows staged.  Pairs leave after 2, 3, 4 and 5 lengths; one wave holds 16 pairs in a row, one exactly one; the last
    workgroups span many short rows (row_off >= 2: the row from memory) and hold planted pairs; a row band that starts mid-row."""
    bins, o, exp = _self_case(oracle, "every", N1, 64, _plants(N1), CLUSTER)
    _waves_are_as_planted(oracle, o, 64)
    g = gpu_ctx.sketches(bins, N1, KMERS, 64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    _ran_staged(gpu_ctx, 2)
    part = skl.self_dists_rows(gpu_ctx, g, g.set_k(), 1, N1 - 5)
    lo = N1 - 1
    _check(part, exp[lo:lo + part.shape[0]])
    _ran_staged(gpu_ctx, 2)
    g.close()


def test_staged_three_lengths_counted(oracle, skl, gpu_ctx):
    """The sampled choice counts THREE lengths where many pairs pass exactly two: 73 samples related at their first two lengths
    only (8 % of the pairs; 22 % of those share a bin at the third by chance), 40 related at all five (2.4 %).  Shares still in
    the running after 2 / 3 / 4 lengths: 14.7 / 5.1 / 3.0 %; modelled cost (eb_plan.hpp: lengths + 20 x share, at most 4.5):
    4.9 / 4.0 / 4.6 -- three lengths, 5.1 % in the running: staged."""
    clusters = [(10, 73, 2, 0.8), (150, 40, 5, 0.8)]
    bins, o, exp = _self_case(oracle, "three", N1, 64, [(0, 5, 3), (2, 9, 4), (200, 230, 5), (250, 255, 4)], clusters)
    g = gpu_ctx.sketches(bins, N1, KMERS, 64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    _ran_staged(gpu_ctx, 3)
    g.close()


@pytest.mark.parametrize("ss64", [32, 64, 65, 157])
def test_staged_trips(oracle, skl, gpu_ctx, ss64):
    """1 trip (2 048 bins: 1.4 % by chance, so 64 relatives: + 6.2 %), 2 trips, 3 trips with the last one partial; at 157 chunks
    the two rows do not fit the 16 KB the launch may ask for: no staging, whatever form the library picks."""
    bins, o, exp = _self_case(oracle, ("trips", ss64), N1, ss64, _plants(N1), [(150, 64, 5, 0.8)])
    g = gpu_ctx.sketches(bins, N1, KMERS, ss64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    name = gpu_ctx.last_kernel()
    if ss64 <= 73:
        assert "early break: " in name and "[lean epilogue" in name and STAGED in name, name
    else:           # (10 048 bins: 46 % of random pairs share a bin at a length; whether the early break pays is the sample's call)
        assert STAGED not in name, name
    g.close()


def test_staged_relatives_in_the_last_rows(oracle, skl, gpu_ctx):
    """The last 24 samples are one cluster: its 276 pairs lie in rows of 23 ... 1 pairs, all in the matrix' last two workgroups,
    which span a dozen rows each -- every one of those pairs but the first two rows' reads its row from memory."""
    bins, o, exp = _self_case(oracle, "last", N1, 64, [(0, 5, 3)], [(232, 24, 5, 0.8), (60, 40, 5, 0.8)])
    g = gpu_ctx.sketches(bins, N1, KMERS, 64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    _ran_staged(gpu_ctx, 2)
    g.close()


@pytest.mark.parametrize("rows,cols", [(256, 256), (520, 130), (1100, 60)])
def test_staged_cross_forms(oracle, skl, gpu_ctx, rows, cols):
    """Cross matrices above the floor; every block of 256 rows holds chance pairs alike (4.8 %) and relatives of the column
    samples.  130 columns: a workgroup spans two or three rows; 60 columns: every lane locates its own pair, four or five rows."""
    m = max(rows, cols)
    big = _clustered(m, 64, _plants(60), [(30, 20, 5, 0.8)], seed=5)
    g_r, g_q = gpu_ctx.sketches(big[:rows], rows, KMERS, 64), gpu_ctx.sketches(big[:cols], cols, KMERS, 64)
    o_r, o_q = oracle.Sketches(big[:rows], rows, KMERS, 64), oracle.Sketches(big[:cols], cols, KMERS, 64)
    want = oracle.cross_dists_all(o_r, o_q, oracle.COREACC, threads=8).reshape(-1, 2)
    assert ((want[:, 0] != 1.0) | (want[:, 1] != 1.0)).sum() >= 100
    _check(skl.cross_dists_all(gpu_ctx, g_r, g_q, g_r.set_k()).reshape(-1, 2), want)
    _ran_staged(gpu_ctx, 2)
    g_r.close()
    g_q.close()


def test_staged_with_a_completeness_correction(oracle, skl, gpu_ctx):
    """coreacc_epilogue_lean_kernel<.., COMP = true> with its rows staged (4 096 bins, values in (0, 1])."""
    bins, o, exp = _self_case(oracle, "every", N1, 64, _plants(N1), CLUSTER)
    comp = np.random.default_rng(11).uniform(0.4, 1.0, N1)
    comp[::5] = 1.0
    oc = oracle.Sketches(bins, N1, KMERS, 64, completeness=comp)
    want = oracle.self_dists_all(oc, oracle.COREACC, cutoff=0.3, threads=8).reshape(-1, 2)
    g = gpu_ctx.sketches(bins, N1, KMERS, 64, completeness=comp)
    got = skl.self_dists_all(gpu_ctx, g, g.set_k(cutoff=0.3))
    _check(got, want, comp=True)
    _ran_staged(gpu_ctx)
    g.close()


@pytest.mark.ab_library
def test_staged_blocked_order(oracle, skl, gpu_ctx, monkeypatch):
    """SKL_EB_BLOCKED=1 (A/B build) with the sampled choice: the blocked order stages ONE row per workgroup."""
    bins, o, exp = _self_case(oracle, "every", N1, 64, _plants(N1), CLUSTER)
    monkeypatch.setenv("SKL_EB_BLOCKED", "1")
    monkeypatch.setenv("SKL_EB_BLK_ROW_SHIFT", "7")
    gpu_ctx.reload_env()
    g = gpu_ctx.sketches(bins, N1, KMERS, 64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    assert "pairs per XCD" in gpu_ctx.last_kernel(), gpu_ctx.last_kernel()
    _ran_staged(gpu_ctx, 2)
    g.close()
