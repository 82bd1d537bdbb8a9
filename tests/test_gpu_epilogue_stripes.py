"""The STRIPED order of the lean early-break epilogue (csrc/eb_stripes.hpp, epilogue.hip EbPairLoc): the launch's columns in 2 X
stripes, XCD x owns stripes x and 2 X - 1 - x, a workgroup = two rows against one 64-column block of each of its XCD's stripes.
tests/test_eb_stripes_cpu.py checks the map itself on the CPU; here the kernel runs in that order.

Every case compares the WHOLE output with the oracle: bit-identical without a completeness correction, |delta| <= 1e-6 with
one, and the (1, 1) pattern exactly.  The sketches are random with PLANTED relatives, made as in tests/test_gpu_epilogue_chain.py
(the small generators are copied from there).  The order is forced with SKL_EB_STRIPES=1 -- by rule the library takes it where
the lean kernel stages its rows, which needs 3 % of the sampled pairs still in the running: at 4 096 bins chance alone gives
4.8 %, at fewer bins a cluster of relatives does -- and every case that should run striped asserts the marker in last_kernel()."""
import numpy as np
import pytest

from sketchlib.rust_amd import synth

pytestmark = pytest.mark.gpu

KMERS = [15, 19, 23, 27, 31]
NK = len(KMERS)
STAGED = "[row slices staged in LDS]"
STRIPED = "[column stripes folded onto the XCDs]"


def _plants(n):
    """Row 1 has 16 consecutive related columns (all five lengths); pairs leaving after 2, 3, 4 and 5 lengths near the start, in
    the middle (one of them across the first stripe boundary at column 64) and among the last rows."""
    out = [(1, c, 5) for c in range(8, 24)]
    out += [(0, 5, 2), (0, 6, 3), (0, 7, 4), (2, 30, 5), (62, 65, 4), (63, 64, 5), (n // 2, n // 2 + 3, 3), (n // 2, n - 2, 4)]
    out += [(n - 9, n - 4, 2), (n - 8, n - 3, 3), (n - 7, n - 2, 4), (n - 6, n - 1, 5), (n - 3, n - 1, 3)]
    return out


def _clustered(n, ss64, plants, clusters, seed=21):
    """Random 14-bit bins [n, NK, ss64 * 64]; clusters = [(first, count, m, keep, step)]: `count` samples, every step-th from `first`
    on, copy `keep` of one parent's bins at their first m lengths; plants = [(a, c, m)]: sample c shares ~60 % of a's bins at
    lengths 0 .. m - 1."""
    rng = np.random.default_rng(seed)
    nb = ss64 * 64
    vals = rng.integers(0, 1 << 14, size=(n, NK, nb), dtype=np.uint16)
    for first, count, m, keep, step in clusters:
        parent = rng.integers(0, 1 << 14, size=(m, nb), dtype=np.uint16)
        mask = rng.random((count, m, nb)) < keep
        members = first + step * np.arange(count)
        vals[members, :m] = np.where(mask, parent[None], vals[members, :m])
    for a, c, m in plants:
        keep = rng.random((m, nb)) < 0.6
        vals[c, :m] = np.where(keep, vals[a, :m], vals[c, :m])
    return np.ascontiguousarray(synth.bitslice(vals).reshape(n, NK * ss64 * synth.BBITS))


def _disjoint(n, ss64, seed):
    """Unrelated for certain: sample s holds only bin values = s (mod n), so no two samples share a bin at any length."""
    rng = np.random.default_rng(seed)
    nb = ss64 * 64
    r = rng.integers(0, (1 << 14) // n, size=(n, NK, nb)).astype(np.uint16)
    return (r * np.uint16(n) + np.arange(n, dtype=np.uint16)[:, None, None]).astype(np.uint16)


def _passed_lengths(oracle, o, ss64):
    """The oracle's own bin-match counts: how many leading lengths pass the reference's test (bimodal data only, asserted)."""
    same = oracle.self_binmatch(o, threads=8)
    nb, expected = ss64 * 64, (ss64 * 64) >> 14
    assert not ((same > 24 + expected) & (same < nb // 8)).any()
    return np.cumprod(same > expected, axis=1).sum(axis=1)


def _check(got, exp, comp=False):
    if comp:
        assert np.max(np.abs(got.astype(np.float64) - exp.astype(np.float64))) <= 1e-6
    else:
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), np.argwhere(got != exp)[:5]
    assert np.array_equal((got[:, 0] == 1.0) & (got[:, 1] == 1.0), (exp[:, 0] == 1.0) & (exp[:, 1] == 1.0))


_REF = {}


def _cluster(n):
    """A cluster that keeps the share of pairs still in the running above 3 % whatever chance gives.  n = 256 is ONE block of the
    sampler (eb_plan.hpp: 256 x 256 sample ids): 40 neighbours, 780 pairs, 2.4 %.  Above, every 8th sample from 36 on is a member
    (about 1.3 % of the pairs of every block alike; none of them is a planted sample): the blocks must stay of one mind, or the
    plan is block by block and the general kernel runs."""
    return [(150, 40, 5, 0.8, 1)] if n <= 256 else [(36, (n - 9 - 36) // 8, 5, 0.8, 8)]


def _self_case(oracle, n, ss64, clusters=None):
    """(bins, oracle sketches, expected matrix), computed once per shape and shared (read-only)."""
    clusters = _cluster(n) if clusters is None else clusters
    key = (n, ss64, tuple(clusters))
    if key not in _REF:
        bins = _clustered(n, ss64, _plants(n), clusters)
        o = oracle.Sketches(bins, n, KMERS, ss64)
        exp = oracle.self_dists_all(o, oracle.COREACC, threads=8).reshape(-1, 2)
        exp.setflags(write=False)
        _REF[key] = (bins, o, exp)
    return _REF[key]


def _force(gpu_ctx, monkeypatch, stripes="1", xcds=None):
    monkeypatch.setenv("SKL_EB_STRIPES", stripes)
    if xcds is not None:
        monkeypatch.setenv("SKL_XCDS", str(xcds))
    gpu_ctx.reload_env()


def _ran_striped(gpu_ctx):
    name = gpu_ctx.last_kernel()
    assert "[lean epilogue" in name and STAGED in name and STRIPED in name, name
    assert "early break: " in name, name


@pytest.mark.parametrize("n", [256, 257, 272, 321])
def test_self_sizes(oracle, skl, gpu_ctx, monkeypatch, n):
    """4 096 bins on 8 XCDs: W = 64, stripes 0 ... 15.  n = 256: stripes 4 ... 15 hold no column (XCDs 4 ... 7 hold nothing); 272: a
    partial stripe of 16 columns; 321: six stripes, the last with ONE column, an odd number of rows.  Every wave on the diagonal
    straddles it.  Pairs leave after 2, 3, 4 and 5 lengths.
    n = 257 cannot run striped in this library: the sampler's block (1, 1) holds one sample and no pair, and a live block without
    a sample makes eb_decide (eb_plan.hpp, pinned by tests/native/eb_plan_check.cpp) answer block by block, which the general
    kernel takes.  The case stays for its results, and asserts that the order was NOT taken; its one-column stripe is n = 321's."""
    bins, o, exp = _self_case(oracle, n, 64)
    assert {2, 3, 4, 5} <= set(np.unique(_passed_lengths(oracle, o, 64)).tolist())
    _force(gpu_ctx, monkeypatch)
    g = gpu_ctx.sketches(bins, n, KMERS, 64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    if n % 256 == 1:
        assert "block by block" in gpu_ctx.last_kernel() and STRIPED not in gpu_ctx.last_kernel(), gpu_ctx.last_kernel()
    else:
        _ran_striped(gpu_ctx)
    g.close()


@pytest.mark.parametrize("first_row", [1, 2])
def test_row_bands(oracle, skl, gpu_ctx, monkeypatch, first_row):
    """A band that starts at an odd and at an even row and ends five rows short: the workgroups' row pairs start at the band's
    first row, the output at the band's first pair."""
    n = 272
    bins, o, exp = _self_case(oracle, n, 64)
    _force(gpu_ctx, monkeypatch)
    g = gpu_ctx.sketches(bins, n, KMERS, 64)
    part = skl.self_dists_rows(gpu_ctx, g, g.set_k(), first_row, n - 5)
    lo = first_row * n - first_row * (first_row + 1) // 2
    assert part.shape[0] == (n - 5) * n - (n - 5) * (n - 4) // 2 - lo
    _check(part, exp[lo:lo + part.shape[0]])
    _ran_striped(gpu_ctx)
    g.close()


@pytest.mark.parametrize("rows,cols", [(256, 256), (520, 130), (1100, 60)])
def test_cross_forms(oracle, skl, gpu_ctx, monkeypatch, rows, cols):
    """Cross matrices (p = i * columns + j): 130 columns = two full stripes and one of two columns; 60 columns: fewer than one
    block, seven of eight XCDs hold nothing."""
    key = ("cross", rows, cols)
    if key not in _REF:
        big = _clustered(max(rows, cols), 64, _plants(60), [(30, 20, 5, 0.8, 1)], seed=5)
        o_r, o_q = oracle.Sketches(big[:rows], rows, KMERS, 64), oracle.Sketches(big[:cols], cols, KMERS, 64)
        want = oracle.cross_dists_all(o_r, o_q, oracle.COREACC, threads=8).reshape(-1, 2)
        want.setflags(write=False)
        _REF[key] = (big, want)
    big, want = _REF[key]
    assert ((want[:, 0] != 1.0) | (want[:, 1] != 1.0)).sum() >= 100
    _force(gpu_ctx, monkeypatch)
    g_r, g_q = gpu_ctx.sketches(big[:rows], rows, KMERS, 64), gpu_ctx.sketches(big[:cols], cols, KMERS, 64)
    _check(skl.cross_dists_all(gpu_ctx, g_r, g_q, g_r.set_k()).reshape(-1, 2), want)
    _ran_striped(gpu_ctx)
    g_r.close()
    g_q.close()


@pytest.mark.parametrize("ss64", [32, 65, 157])
def test_sketch_sizes(oracle, skl, gpu_ctx, monkeypatch, ss64):
    """1 trip per slice (2 048 bins: 64 relatives keep the share above 3 %), 3 trips with the last one partial; at 157 chunks the
    two rows do not fit the LDS the launch may ask for: nothing is staged, so the order must not be taken."""
    n = 256
    bins, o, exp = _self_case(oracle, n, ss64, [(150, 64, 5, 0.8, 1)])
    _force(gpu_ctx, monkeypatch)
    g = gpu_ctx.sketches(bins, n, KMERS, ss64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    if ss64 <= 73:
        _ran_striped(gpu_ctx)
    else:
        assert STRIPED not in gpu_ctx.last_kernel() and STAGED not in gpu_ctx.last_kernel(), gpu_ctx.last_kernel()
    g.close()


@pytest.mark.parametrize("xcds", [1, 2, 4])
def test_fewer_xcds(oracle, skl, gpu_ctx, monkeypatch, xcds):
    """SKL_XCDS = 1 / 2 / 4: W = 192 / 128 / 64 at n = 272: stripes of three and two blocks, one XCD that owns both of two stripes."""
    n = 272
    bins, o, exp = _self_case(oracle, n, 64)
    _force(gpu_ctx, monkeypatch, xcds=xcds)
    g = gpu_ctx.sketches(bins, n, KMERS, 64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    _ran_striped(gpu_ctx)
    g.close()


@pytest.mark.parametrize("above_one", [False, True])
def test_completeness(oracle, skl, gpu_ctx, monkeypatch, above_one):
    """A completeness vector in (0, 1]: coreacc_epilogue_lean_kernel<.., COMP = true> in the striped order.  With a value above 1 the
    lean kernel declines the launch: no marker, the same results."""
    n = 256
    bins, o, exp = _self_case(oracle, n, 64)
    comp = np.random.default_rng(11).uniform(0.4, 1.0, n)
    comp[::5] = 1.0
    if above_one:
        comp[3] = 1.25
    oc = oracle.Sketches(bins, n, KMERS, 64, completeness=comp)
    want = oracle.self_dists_all(oc, oracle.COREACC, cutoff=0.3, threads=8).reshape(-1, 2)
    _force(gpu_ctx, monkeypatch)
    g = gpu_ctx.sketches(bins, n, KMERS, 64, completeness=comp)
    got = skl.self_dists_all(gpu_ctx, g, g.set_k(cutoff=0.3))
    _check(got, want, comp=True)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if above_one:
        assert STRIPED not in gpu_ctx.last_kernel() and "[lean epilogue" not in gpu_ctx.last_kernel(), gpu_ctx.last_kernel()
    else:
        _ran_striped(gpu_ctx)
    g.close()


def test_workgroups_that_complete_nothing(oracle, skl, gpu_ctx, monkeypatch):
    """1 024 bins, disjoint bin values, the first 64 of 256 samples relatives of one another (6.2 % of the pairs): every workgroup
    that holds a pair stages its rows, and those of the rows and columns from 64 on complete nothing."""
    n, ss64, relatives = 256, 16, 64
    vals = _disjoint(n, ss64, seed=13)
    keep = np.random.default_rng(17).random((relatives, NK, ss64 * 64)) < 0.7
    vals[:relatives] = np.where(keep, vals[0], vals[:relatives])
    bins = np.ascontiguousarray(synth.bitslice(vals).reshape(n, NK * ss64 * synth.BBITS))
    o = oracle.Sketches(bins, n, KMERS, ss64)
    exp = oracle.self_dists_all(o, oracle.COREACC, threads=8).reshape(-1, 2)
    first_unrelated = relatives * n - relatives * (relatives + 1) // 2
    assert np.all(exp[first_unrelated:] == 1.0) and np.any(exp[:first_unrelated] != 1.0)
    _force(gpu_ctx, monkeypatch)
    g = gpu_ctx.sketches(bins, n, KMERS, ss64)
    _check(skl.self_dists_all(gpu_ctx, g, g.set_k()), exp)
    _ran_striped(gpu_ctx)
    g.close()


def test_flat_and_striped_agree_byte_for_byte(oracle, skl, gpu_ctx, monkeypatch):
    """The same matrix with SKL_EB_STRIPES=0 and =1."""
    n = 321
    bins, o, exp = _self_case(oracle, n, 64)
    g = gpu_ctx.sketches(bins, n, KMERS, 64)
    _force(gpu_ctx, monkeypatch, "0")
    flat = skl.self_dists_all(gpu_ctx, g, g.set_k())
    name = gpu_ctx.last_kernel()
    assert STAGED in name and STRIPED not in name, name
    _force(gpu_ctx, monkeypatch, "1")
    striped = skl.self_dists_all(gpu_ctx, g, g.set_k())
    _ran_striped(gpu_ctx)
    assert flat.tobytes() == striped.tobytes()
    _check(striped, exp)
    g.close()
