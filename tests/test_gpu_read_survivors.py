"""skl_reads_survivors (csrc/read_survivors.hip behind csrc/capi_reads.cpp) at the ABI, exactly: for every stream
(sample, k) and every range of window starts [lo, hi), the records the kernel appends must be the windows of
tests/reads_reference.py's window_table with lo <= start < hi and sign < thr[sample, ki, sign // bin_size],
bin_size = ceil(SIGN_MOD / num_bins) -- the counts equal, the (start, sign) records equal once sorted by start,
nothing written past a stream's count.  window_table is the oracle's non-rolling hash (pinned on the reference's
.skd files) under a searchsorted mask; tests/test_sketch_reads_cpu.py ties it to the literal restatement of the
reference's iterator.  Integer arithmetic throughout; equality is the only assertion.

Covered: many samples in one handle (span -> sample search with empty samples and empty ranges, per-sample word /
offset / code bases, the stream index), range shapes around a wave and a workgroup and around a break, k from 1 to
200 on both strands, bin counts from 1 to 100 032, the strict compare, and the call shapes of one handle.

Not covered: the `++bin` branch of the kernel's bin correction.  The reciprocal estimate is below the true bin
only for a sign within about 2^-20 of a bin's upper edge in relative terms, which no input of this size produces;
dropping that branch fails no case here.

Before every GPU call the reference alone must show that the case can fail: every stream with a window in range has
at least one survivor and at least one window that is not.  A range of one window cannot show both under one table,
and one of a few windows often does not under a random one, so a range of fewer than 20 windows is called under two
more tables: the threshold of its first window's bin at that window's sign (absent) and one above it (present)."""
import functools

import numpy as np
import pytest

import reads_reference as R

pytestmark = pytest.mark.gpu
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def sample(rng, lengths, n_frac):
    """(codes, offsets) of records of `lengths` bases, a fraction n_frac of them invalid: an offset per invalid base
    and one at every record's end, in valid-base coordinates (as tests/test_gpu_sketch.py builds them)."""
    codes, offsets, pos = [], [], 0
    for ln in lengths:
        seq = rng.integers(0, 4, size=ln, dtype=np.uint8)
        invalid = rng.random(ln) < n_frac
        keep = ~invalid
        before = np.cumsum(keep) - keep
        offsets.append(pos + before[invalid])
        codes.append(seq[keep])
        pos += int(keep.sum())
        offsets.append(np.array([pos]))
    return np.concatenate(codes).astype(np.uint8), np.concatenate(offsets).astype(np.int64)


@functools.lru_cache(maxsize=None)
def samples():
    """The samples of this module, built once and never written to."""
    rng = np.random.default_rng(20260)
    out = {
        "big": sample(rng, [40000], 0.002),                   # more than two workgroups of 16 384 starts
        "w4104": sample(rng, [4096 + 8], 0.0),                # one wave of spans and eight starts
        "b17": sample(rng, [17], 0.0),                        # a ragged last word; no window at k = 31
        "empty": (np.zeros(0, np.uint8), np.zeros(1, np.int64)),
        "nooffs": (rng.integers(0, 4, size=3000, dtype=np.uint8), np.zeros(0, np.int64)),
        "rec64": sample(rng, [64] * 9, 0.0),                  # a break on every lane's span boundary
        "ks": sample(rng, [300, 5000, 1200, 700], 0.001),     # every k up to 200 has windows
        "s150": sample(rng, [150], 0.0),                      # none at k = 200
        "bins": sample(rng, [10000, 20100], 0.001),           # about 30 000 windows at k = 21
    }
    assert len(out["w4104"][0]) == 4104 and len(out["b17"][0]) == 17 and len(out["s150"][0]) == 150
    for codes, offsets in out.values():
        codes.flags.writeable = False
        offsets.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def table(name, k, rc):
    starts, signs = R.window_table(*samples()[name], k, rc)
    starts.flags.writeable = False
    signs.flags.writeable = False
    return starts, signs


def bin_size_of(num_bins):
    return -(-R.SIGN_MOD // num_bins)


def random_thresholds(rng, n_streams, num_bins):
    """[n_streams, num_bins] uint64, every one in [0, SIGN_MOD) and every stream's its own: the odd bins anywhere in
    that range, the even bins inside their own bin's interval, where a sign filed one bin off changes its fate."""
    bs = bin_size_of(num_bins)
    thr = rng.integers(0, R.SIGN_MOD, size=(n_streams, num_bins), dtype=np.uint64)
    lo = np.arange(num_bins, dtype=np.uint64) * np.uint64(bs)
    assert int(lo[-1]) < R.SIGN_MOD
    width = np.minimum(np.uint64(bs), np.uint64(R.SIGN_MOD) - lo)   # the last bin is short
    own = lo + rng.integers(0, np.broadcast_to(width, thr.shape), dtype=np.uint64)
    thr[:, ::2] = own[:, ::2]
    assert int(thr.max()) < R.SIGN_MOD
    return thr


class Want:
    def __init__(self, n_in, recs):
        self.n_in, self.recs = n_in, recs   # windows in range; the survivors [m, 2] uint64 in start order


class Batch:
    """One skl.Reads handle over named samples and the expectation of any call on it."""

    def __init__(self, skl, ctx, names, kmers, num_bins, rc=True):
        parts = [samples()[n] for n in names]
        cb = np.cumsum([0] + [len(c) for c, _ in parts])
        ob = np.cumsum([0] + [len(o) for _, o in parts])
        codes = np.concatenate([c for c, _ in parts])
        offs = np.concatenate([o for _, o in parts])
        self.names, self.kmers, self.num_bins, self.rc = names, list(kmers), num_bins, rc
        self.n, self.nk, self.bin_size = len(names), len(kmers), bin_size_of(num_bins)
        self.lengths = [len(c) for c, _ in parts]
        self.reads = skl.Reads(ctx, skl.pack_codes(codes, cb), cb, offs, ob, self.kmers, num_bins, rc)

    def close(self):
        self.reads.close()

    def expected(self, lo, hi, thr):
        """[Want] per stream sample * nk + ki."""
        thr = np.asarray(thr, dtype=np.uint64).reshape(self.n, self.nk, self.num_bins)
        out = []
        for s, name in enumerate(self.names):
            for ki, k in enumerate(self.kmers):
                starts, signs = table(name, k, self.rc)
                in_range = (starts >= lo[s]) & (starts < hi[s])
                bins = (signs // np.uint64(self.bin_size)).astype(np.int64)
                keep = in_range & (signs < thr[s, ki][bins])
                out.append(Want(int(in_range.sum()), np.stack([starts[keep].astype(np.uint64), signs[keep]], axis=1)))
        return out

    def call_equals(self, lo, hi, thr, want=None):
        """One call with room for every survivor: exact counts, exact records, nothing behind them."""
        want = self.expected(lo, hi, thr) if want is None else want
        cap = max(len(w.recs) for w in want)
        recs, counts = self.reads.survivors(lo, hi, thr, cap)
        assert counts.tolist() == [len(w.recs) for w in want]
        for st, w in enumerate(want):
            m = len(w.recs)
            got = recs[st, :m]
            got = got[np.argsort(got[:, 0], kind="stable")]
            assert np.array_equal(got, w.recs), (st, self.names[st // self.nk], self.kmers[st % self.nk])
            assert not recs[st, m:].any(), st
        return want


def assert_can_fail(want, all_or_nothing=()):
    """On the reference alone: a stream with a window in range has a survivor and a window that is not one."""
    for st, w in enumerate(want):
        if w.n_in and st not in all_or_nothing:
            assert 0 < len(w.recs) < w.n_in, (st, len(w.recs), w.n_in)


FEW = 20   # windows; below this one random table leaves a range all-in or all-out too often to demand both


def check_range(b, lo, hi, thr):
    """A single-stream batch on [lo, hi) -> the number of windows in range.  A range of FEW windows or more must
    show a survivor and a window that is not one under `thr`; a smaller one is also called under two tables made for
    it: the threshold of its first window's bin at that window's sign (absent), then one above it (present)."""
    want = b.expected([lo], [hi], thr)
    n_in = want[0].n_in
    if n_in >= FEW:
        assert_can_fail(want)
    b.call_equals([lo], [hi], thr, want)
    if 0 < n_in < FEW:
        starts, signs = table(b.names[0], b.kmers[0], b.rc)
        first = np.nonzero((starts >= lo) & (starts < hi))[0][0]
        start, sign = int(starts[first]), int(signs[first])
        for t, present in ((sign, False), (sign + 1, True)):
            thr2 = thr.copy()
            thr2[0, sign // b.bin_size] = t
            want = b.expected([lo], [hi], thr2)
            assert ([start, sign] in want[0].recs.tolist()) == present
            b.call_equals([lo], [hi], thr2, want)
    return n_in


MANY = ["big", "w4104", "b17", "empty", "nooffs", "rec64"]


def test_many_samples_in_one_handle(skl, gpu_ctx):
    """Six samples, k = 9 and 31, 256 bins, a range of its own per sample; an empty range on a middle sample in the
    first call and on the last sample in the second, and in each call one range wholly past its sample.  Every stream
    has its own thresholds, three bins at u64::MAX and three at 0 among them, so a transposed stream index fails."""
    rng = np.random.default_rng(11)
    b = Batch(skl, gpu_ctx, MANY, [9, 31], 256)
    n = b.lengths
    assert n[3] == 0 and len(samples()["nooffs"][1]) == 0
    assert samples()["rec64"][1].tolist() == list(range(64, 577, 64))
    thr = random_thresholds(rng, b.n * b.nk, b.num_bins)
    for st in range(b.n * b.nk):
        special = rng.choice(b.num_bins, size=6, replace=False)
        thr[st, special[:3]] = U64_MAX
        thr[st, special[3:]] = 0
    assert len({row.tobytes() for row in thr}) == b.n * b.nk
    calls = [
        # big            w4104         b17       empty    nooffs        rec64
        ([37, 5000, 0, 0, 1000, 3], [33000, 6000, 17, 0, 1000, 570]),       # past: w4104; empty: nooffs (middle)
        ([0, 8, 17, 0, 130, 100], [n[0] + 50, 4104, 40, 9, 2900, 100]),     # past: b17; empty: rec64 (last)
    ]
    idle = [{1, 3, 4}, {2, 3, 5}]   # samples the reference gives no window in range
    for (lo, hi), none in zip(calls, idle):
        want = b.expected(lo, hi, thr)
        for s in range(b.n):
            for ki, k in enumerate(b.kmers):
                has = want[s * b.nk + ki].n_in > 0
                assert has == (s not in none and not (MANY[s] == "b17" and k == 31)), (s, k)
        assert_can_fail(want)
        b.call_equals(lo, hi, thr, want)
    assert "read_survivors_kernel" in gpu_ctx.last_kernel()
    b.close()


@pytest.mark.parametrize("length", [1, 63, 64, 65, 4095, 4096, 4097, 16384, 16385])
def test_range_shapes(skl, gpu_ctx, length):
    """Ranges of `length` starts beginning at 0, 5, 16, 63, 64 and 1000 of one 40 000-base sample with breaks: a lane's
    span, a wave (4096 starts) and a workgroup (16 384 starts), one less and one more."""
    b = Batch(skl, gpu_ctx, ["big"], [15], 64)
    thr = random_thresholds(np.random.default_rng(12), 1, 64)
    n_in = [check_range(b, lo, lo + length, thr) for lo in (0, 5, 16, 63, 64, 1000)]
    assert max(n_in) >= min(length, 2) and (length > 1 or 1 in n_in)
    b.close()


def test_ranges_at_a_break(skl, gpu_ctx):
    """k = 15; ranges of 1, 2, 70 and 200 starts that begin one before, at and one after an offset: the window at o - 1
    has the break inside it, those at o and o + 1 do not (the first-break search is `> p0`, the seed is at p0)."""
    b = Batch(skl, gpu_ctx, ["big"], [15], 64)
    thr = random_thresholds(np.random.default_rng(13), 1, 64)
    offs = np.unique(samples()["big"][1])
    gaps = np.diff(offs)
    lone = offs[1:-1][(gaps[:-1] > 40) & (gaps[1:] > 40)]   # offsets with no other break within 40 bases
    assert lone.size >= 3
    starts = table("big", 15, True)[0]
    for o in (int(lone[0]), int(lone[lone.size // 2]), int(lone[-1])):
        assert o - 1 not in starts and o in starts and o + 1 in starts
        for lo in (o - 1, o, o + 1):
            got = [check_range(b, lo, lo + ln, thr) for ln in (1, 2, 70, 200)]
            assert got[0] == (0 if lo == o - 1 else 1)
    b.close()


def test_ranges_past_the_last_window(skl, gpu_ctx):
    """Ends past len - k + 1 (the kernel's own bound) and past len (the host's clamp); begins at and past them too."""
    b = Batch(skl, gpu_ctx, ["big"], [15], 64)
    thr = random_thresholds(np.random.default_rng(14), 1, 64)
    n = b.lengths[0]
    last = n - 15 + 1
    assert check_range(b, last - 300, last + 5, thr) > 100
    assert check_range(b, last - 300, n + 1000, thr) > 100
    assert check_range(b, 1000, 2 ** 62, thr) > 30000
    assert check_range(b, last - 1, n, thr) == 1
    assert check_range(b, last, n + 7, thr) == 0       # inside the sample, behind its last window
    assert check_range(b, n, n + 64, thr) == 0
    assert check_range(b, n + 100, n + 5000, thr) == 0
    b.close()


KS = [1, 31, 32, 33, 64, 65, 129, 200]


@pytest.mark.parametrize("rc", [True, False])
def test_kmer_lengths(skl, gpu_ctx, rc):
    """k of 1, around 32 and 64 (one and two words of codes, the lane's span of 64 starts), 129 and 200 (a seed longer
    than the span) on records of 300 to 5000 bases, and on a 150-base sample that has no window at k = 200."""
    b = Batch(skl, gpu_ctx, ["ks", "s150"], KS, 64, rc)
    thr = random_thresholds(np.random.default_rng(21), b.n * b.nk, 64)   # (k = 1 has two or four signs: many seeds fail)
    lo, hi = [7, 0], [b.lengths[0], 150]
    want = b.expected(lo, hi, thr)
    assert [st for st, w in enumerate(want) if w.n_in == 0] == [1 * b.nk + KS.index(200)]
    assert_can_fail(want)
    b.call_equals(lo, hi, thr, want)
    b.close()


@pytest.mark.parametrize("num_bins", [1, 64, 1000, 4096, 100032])
def test_bin_counts(skl, gpu_ctx, num_bins):
    """About 30 000 windows at k = 21 filed into one bin, a power of two, 1000 bins (a short last bin) and 100 032."""
    b = Batch(skl, gpu_ctx, ["bins"], [21], num_bins)
    thr = random_thresholds(np.random.default_rng(17), 1, num_bins)
    starts, signs = table("bins", 21, True)
    assert starts.size > 29000
    bins = signs // np.uint64(b.bin_size)
    assert np.unique(bins).size > min(num_bins, 20000) * 0.9
    if num_bins <= 4096:   # the first and the (short) last bin are in use
        assert int(bins.min()) == 0 and int(bins.max()) == num_bins - 1
    assert check_range(b, 0, b.lengths[0], thr) == starts.size
    b.close()


def test_compare_is_strict(skl, gpu_ctx):
    """In every one of 64 bins the threshold is a sign m of that bin that is not its smallest: m is absent, every
    smaller sign of the bin present; with m + 1 in its place m is present too."""
    b = Batch(skl, gpu_ctx, ["bins"], [21], 64)
    starts, signs = table("bins", 21, True)
    bins = (signs // np.uint64(b.bin_size)).astype(np.int64)
    thr = np.zeros((1, 64), dtype=np.uint64)
    for bi in range(64):
        in_bin = np.unique(signs[bins == bi])
        assert in_bin.size >= 2
        thr[0, bi] = in_bin[in_bin.size // 2]   # never the smallest
    lo, hi = [0], [b.lengths[0]]
    at = b.expected(lo, hi, thr)
    above = b.expected(lo, hi, thr + np.uint64(1))
    for bi in range(64):
        m = thr[0, bi]
        below = np.unique(signs[(bins == bi) & (signs < m)])
        assert below.size >= 1
        assert m not in at[0].recs[:, 1] and np.isin(below, at[0].recs[:, 1]).all()
        assert m in above[0].recs[:, 1]
    assert len(above[0].recs) >= len(at[0].recs) + 64
    b.call_equals(lo, hi, thr, at)
    b.call_equals(lo, hi, thr + np.uint64(1), above)
    b.close()


def test_call_shapes_on_one_handle(skl, gpu_ctx):
    """Room for everything, then none (counts only, a null record pointer), then half the smallest count, then the
    first shape again under thresholds that let fewer through: the call buffer only grows and nothing of an earlier
    call may show."""
    b = Batch(skl, gpu_ctx, ["w4104", "nooffs"], [9, 31], 128)
    streams = b.n * b.nk
    thr = random_thresholds(np.random.default_rng(18), streams, 128)
    lo, hi = [3, 0], [4104, 3000]
    want = b.expected(lo, hi, thr)
    assert_can_fail(want)
    full = max(len(w.recs) for w in want)
    b.call_equals(lo, hi, thr, want)
    assert "read_survivors_kernel" in gpu_ctx.last_kernel()

    recs, counts = b.reads.survivors(lo, hi, thr, 0)
    assert recs.size == 0 and counts.tolist() == [len(w.recs) for w in want]

    cap = min(len(w.recs) for w in want) // 2
    assert cap >= 100
    recs, counts = b.reads.survivors(lo, hi, thr, cap)
    assert counts.tolist() == [len(w.recs) for w in want]
    for st, w in enumerate(want):
        got = set(map(tuple, recs[st].tolist()))
        assert len(got) == cap and got <= set(map(tuple, w.recs.tolist())), st

    floor = np.arange(128, dtype=np.uint64) * np.uint64(b.bin_size)
    lower = np.where(thr >= floor, floor + (thr - np.minimum(thr, floor)) // np.uint64(4), thr // np.uint64(4))
    fewer = b.expected(lo, hi, lower)
    assert_can_fail(fewer)
    assert all(len(f.recs) < len(w.recs) for f, w in zip(fewer, want))
    recs, counts = b.reads.survivors(lo, hi, lower, full)
    assert counts.tolist() == [len(f.recs) for f in fewer]
    for st, f in enumerate(fewer):
        m = len(f.recs)
        got = recs[st, :m]
        assert np.array_equal(got[np.argsort(got[:, 0], kind="stable")], f.recs), st
        assert not recs[st, m:].any(), st
    b.close()
