"""Inputs for skl_sketch_signs in which single windows decide their bins, and their expectation.  Pure numpy, no GPU:
tests/test_sketch_edge_cases_cpu.py checks the properties claimed here on any machine, tests/test_gpu_sketch_edges.py
runs the kernels of csrc/sketch_kernel.hip on the same inputs.

The output of the operation is a bin minimum, so on an ordinary input a kernel that drops, adds or mis-hashes ONE
window is caught only when that window happens to decide its bin.  Two constructions make it decide:

  * quiet background: a random word of period 7 (all four codes in it) tiled to the sample's length, random bases over
    [e - k - 4, e + k + 4) around every edge position e of the case (a span or workgroup boundary, a break, the last
    start).  The background has at most 7 distinct windows per strand, so nearly every window that touches a random
    stretch is alone in its bin, while the rolling hash still sees all four codes everywhere;
  * wide bins: a fully random sample at 2^20 bins, where nearly every window is alone in its bin.

Expectation: reads_reference.window_table(codes, offsets, k, rc) -- the oracle's non-rolling hash, tied to the literal
restatement of the reference's iterator by tests/test_sketch_reads_cpu.py -- reduced with np.minimum.at at
bin_size = ceil(SIGN_MOD / num_bins).  Integers only.

A Case is one sample at one k and one strand setting with its NAMED starts:
  * valid: around every edge e the starts e - k, e - k + 1, e - 1, e, e + 1 that are valid windows.  Each must be the
    only window of its bin that has the bin's minimum: dropping or mis-hashing it changes the output;
  * invalid: those of them that span a break (s < o < s + k, s + k <= len).  The sign such a window would have -- the
    hash of codes[s : s + k] -- must lie strictly below its bin's expected value (or the bin be empty): admitting it
    changes the output;
  * watch: the whole run p - k .. p + 1 before a span boundary p.  At 4096 bins not all of its up to 131 starts can be
    single holders at once: a case has W <= 3 (3 k + 8) windows that touch a random stretch, one of them shares its
    bin with a smaller one with probability below W / (2 * 4096) < 0.16 at k = 129, so at least three quarters of the
    valid ones are demanded.
check() asserts all of this from the reference alone; build() draws seeds (fixed base, the case's name, attempt 0, 1,
...) until it holds at every bin count the case is run at, so everything is deterministic.  A wide-bins case has no
named starts: at least 90 % of ALL its valid windows must be single holders (about 97 % are).

Not covered: k = 1, 2, 3 have at most 4^k / 2 canonical signs, so no window can be alone in its bin; the small-k
inputs (small_k_samples) and the bin-count inputs (random_sample) are compared for plain equality only.  Nor is the
`++bin` branch of the kernels' bin correction reached by inputs of this size (tests/test_gpu_read_survivors.py
explains why).  And no input can tell the staged kernel's strict first-break search (`offs[mid] > p0`) from `>=`: with
`>=` a break at p0 gives next_rel = 0, and the walk's `next_rel <= j` refresh steps over it at j = 0 before the first
window is judged -- the samples with a break exactly at p0 pass under either."""
import functools
import zlib

import numpy as np

import reads_reference as R

U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
BASE_SEED = 20261018
SPAN, WG_STARTS = 128, 512 * 128     # the staged kernel: starts per thread, starts per workgroup
USPAN = 256                          # the unstaged kernel: starts per thread (256 threads: 65 536 starts too)
LDS_BINS = (4096, 4097)              # the staged kernel with the minima in LDS / in global memory
WIDE = 1 << 20
MAX_ATTEMPTS = 400


def bin_size_of(num_bins):
    return -(-R.SIGN_MOD // num_bins)


class Case:
    def __init__(self, name, codes, offsets, k, rc, edges=(), watch=()):
        self.name, self.k, self.rc = name, k, rc
        self.codes = np.ascontiguousarray(codes, dtype=np.uint8)
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.codes.flags.writeable = False
        self.offsets.flags.writeable = False
        n = len(self.codes)
        breaks = np.unique(self.offsets)
        spans = lambda s: bool(np.any((breaks > s) & (breaks < s + k)))
        near = sorted({s for e in edges for s in (e - k, e - k + 1, e - 1, e, e + 1) if 0 <= s and s + k <= n})
        self.valid = [s for s in near if not spans(s)]
        self.invalid = [s for s in near if spans(s)]
        self.watch = [s for s in watch if 0 <= s and s + k <= n and not spans(s)]
        # whether a break lies where named starts can span it
        self.has_inner_break = k >= 2 and bool(edges) and any(0 < o < n and (o - k + 1 >= 0 or o - 1 + k <= n) for o in breaks.tolist())

    @functools.cached_property
    def table(self):
        starts, signs = R.window_table(self.codes, self.offsets, self.k, self.rc)
        return starts, signs

    def would_be_sign(self, s):
        """The sign of codes[s : s + k] with the offsets removed."""
        starts, signs = R.window_table(self.codes[s:s + self.k], np.zeros(0, np.int64), self.k, self.rc)
        assert starts.tolist() == [0]
        return signs[0]

    def expectation(self, num_bins, drop=None, admit=None):
        """[num_bins] uint64; `drop`: without the valid start `drop`; `admit`: with the invalid start `admit`."""
        starts, signs = self.table
        if drop is not None:
            keep = starts != drop
            assert keep.sum() == starts.size - 1
            signs = signs[keep]
        if admit is not None:
            assert admit not in starts
            signs = np.append(signs, self.would_be_sign(admit))
        out = np.full(num_bins, U64_MAX, dtype=np.uint64)
        if signs.size:
            np.minimum.at(out, (signs // np.uint64(bin_size_of(num_bins))).astype(np.int64), signs)
        return out

    def single_holders(self, num_bins):
        """bool per window of the table: the only window of its bin with the bin's minimum."""
        starts, signs = self.table
        bins = (signs // np.uint64(bin_size_of(num_bins))).astype(np.int64)
        holds = signs == self.expectation(num_bins)[bins]
        per_bin = np.bincount(bins[holds], minlength=num_bins)
        return holds & (per_bin[bins] == 1)

    def problems(self, num_bins):
        """What keeps the case from being able to fail at its named starts ([] when nothing does)."""
        starts, _ = self.table
        single = self.single_holders(num_bins)
        exp = self.expectation(num_bins)
        bs = np.uint64(bin_size_of(num_bins))
        out = []
        if not self.valid:
            out.append("no named valid start")
        if self.has_inner_break and not self.invalid:
            out.append("no named invalid start")
        for s in self.valid:
            i = int(np.searchsorted(starts, s))
            if i >= starts.size or starts[i] != s:
                out.append(f"start {s} is not a window of the reference")
            elif not single[i]:
                out.append(f"valid start {s} does not decide its bin")
        for s in self.invalid:
            if s in starts:
                out.append(f"start {s} is a window of the reference")
            else:
                w = self.would_be_sign(s)
                if not w < exp[int(w // bs)]:
                    out.append(f"invalid start {s} would not lower its bin")
        if self.watch:
            idx = np.searchsorted(starts, self.watch)
            if not np.array_equal(starts[idx], self.watch):
                out.append("a watched start is not a window of the reference")
            elif 4 * int(single[idx].sum()) < 3 * len(self.watch):
                out.append(f"only {int(single[idx].sum())} of {len(self.watch)} watched starts decide their bins")
        return out

    def check(self, num_bins):
        assert not self.problems(num_bins), (self.name, self.k, self.rc, num_bins, self.problems(num_bins))


def _rng(name, attempt):
    return np.random.default_rng([BASE_SEED, zlib.crc32(name.encode()), attempt])


def build(name, bins, make):
    """make(rng) -> Case, with the first seed at which the case holds at every bin count of `bins`."""
    for attempt in range(MAX_ATTEMPTS):
        case = make(_rng(name, attempt))
        if not any(case.problems(nb) for nb in bins):
            break
    return case   # (after MAX_ATTEMPTS the last one: check() then says what fails)


def quiet_codes(rng, length, edges, k):
    word = rng.integers(0, 4, size=7, dtype=np.uint8)
    while np.unique(word).size < 4:
        word = rng.integers(0, 4, size=7, dtype=np.uint8)
    codes = np.resize(word, length)
    for e in edges:
        lo, hi = max(e - k - 4, 0), min(e + k + 4, length)
        if lo < hi:
            codes[lo:hi] = rng.integers(0, 4, size=hi - lo, dtype=np.uint8)
    return codes


def quiet_case(name, bins, length, k, rc, offsets, edges, watch=()):
    offsets = np.asarray(offsets, dtype=np.int64)
    edges = sorted(set(edges) | {int(o) for o in offsets if 0 < o < length})
    return build(f"{name}/k{k}/rc{int(rc)}", bins,
                 lambda rng: Case(name, quiet_codes(rng, length, edges, k), offsets, k, rc, edges, watch))


# ---- thread boundary ----------------------------------------------------------------------------------------------

def boundary_offsets(p, k, length):
    """name -> offsets of one sample each around the span boundary p."""
    out = {f"break@p{d:+d}" if d <= 1 else f"break@p+k{d - k:+d}": [p + d] for d in (-1, 0, 1, k - 1, k, k + 1)}
    out["40N@p"] = [p] * 40
    out["40N@p+5"] = [p + 5] * 40
    out["offset@0"] = [0]
    out["no offsets"] = []
    out["offset@len"] = [length]
    return out


@functools.lru_cache(maxsize=None)
def thread_boundary(k, rc, span=SPAN, bins=LDS_BINS, length=3000, p=None):
    """[Case]: the eleven samples of boundary_offsets around p (a multiple of `span`; default: the first one that leaves
    room for the random stretches)."""
    if p is None:
        p = -(-(k + 8) // span) * span
    assert p % span == 0 and p - k - 4 >= 0 and p + 2 * k + 5 + k <= length
    watch = tuple(range(p - k, p + 2))
    return [quiet_case(f"boundary{p}:{name}", bins, length, k, rc, offs, [p] + ([length - k] if name == "offset@len" else []) +
                       ([0 + k] if name == "offset@0" else []), watch)
            for name, offs in boundary_offsets(p, k, length).items()]


def last_thread(k, rc):
    """The same eleven samples around p = 65 536 - 128 of 65 836 bases: the windows of a workgroup's last thread read the
    extra staged row."""
    return thread_boundary(k, rc, length=WG_STARTS + 300, p=WG_STARTS - SPAN)


# ---- workgroup boundary and sample end ----------------------------------------------------------------------------

def end_lengths(k):
    return [WG_STARTS - 1, WG_STARTS, WG_STARTS + 1, WG_STARTS + k - 2, WG_STARTS + k - 1, WG_STARTS + k,
            WG_STARTS + SPAN, WG_STARTS + SPAN + 1, 2 * WG_STARTS + 1]


@functools.lru_cache(maxsize=None)
def sample_ends(k, rc, bins=LDS_BINS, lengths=None):
    """[Case] without breaks: random stretches at 65 536 and at len - k; named 65 535, 65 536, len - k - 1, len - k."""
    out = []
    for length in (lengths or end_lengths(k)):
        edges = [WG_STARTS, length - k]
        make = lambda rng, length=length, edges=edges: _ends_case(rng, length, k, rc, edges)
        out.append(build(f"ends{length}/k{k}/rc{int(rc)}", bins, make))
    return out


def _ends_case(rng, length, k, rc, edges):
    case = Case(f"ends{length}", quiet_codes(rng, length, edges, k), [], k, rc)
    case.valid = [s for s in sorted({WG_STARTS - 1, WG_STARTS, length - k - 1, length - k}) if 0 <= s and s + k <= length]
    return case


# ---- short and empty samples, then a long one -----------------------------------------------------------------------

SHORT_K = 21
SHORT_LENGTHS = [0, 1, SHORT_K - 1, SHORT_K, SHORT_K + 1, 15, 16, 17, 0, 0, 200, 0]


@functools.lru_cache(maxsize=None)
def short_and_empty(rc=True, bins=LDS_BINS, trailing_empty=0):
    """[Case] of SHORT_LENGTHS random bases each (the first and last start of those with a window are named), a quiet
    70 000-base sample with a break (named around 65 536, the break and its last start), `trailing_empty` empty ones."""
    k = SHORT_K
    out = []
    for i, n in enumerate(SHORT_LENGTHS + [0] * trailing_empty):
        name = f"short{i}:{n}"
        if n < k:
            out.append(Case(name, _rng(name, 0).integers(0, 4, size=n, dtype=np.uint8), [], k, rc))
        else:
            make = lambda rng, n=n, name=name: Case(name, rng.integers(0, 4, size=n, dtype=np.uint8), [], k, rc, [k, n - k])
            out.append(build(f"{name}/rc{int(rc)}", bins, make))
    long_one = quiet_case("long70000", bins, 70000, k, rc, [66000], [WG_STARTS, 70000 - k])
    return out[:len(SHORT_LENGTHS)] + [long_one] + out[len(SHORT_LENGTHS):]


# ---- several samples for the batches ------------------------------------------------------------------------------------

BATCH_LENGTHS = [2000, 70000, 16 * 300, 33333, 2001, 65536, 4099]


@functools.lru_cache(maxsize=None)
def batch_samples(k=31, rc=True, bins=LDS_BINS):
    """[Case]: seven quiet samples of 2 000 to 70 000 bases, each with a break in its second span-aligned stretch, named
    around a span boundary, the break and the last start -- in the later batches `first_span != 0` decides them."""
    out = []
    for i, n in enumerate(BATCH_LENGTHS):
        p = SPAN * (3 + i)
        out.append(quiet_case(f"batch{i}:{n}", bins, n, k, rc, [p + 7], [p, n - k]))
    return out


# ---- wide bins ------------------------------------------------------------------------------------------------------------

def random_sample(rng, lengths, n_frac):
    """(codes, offsets) of records of `lengths` bases, a fraction n_frac of them N: an offset per N and one at every
    record's end, in valid-base coordinates (as tests/test_gpu_sketch.py builds them)."""
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
def wide_sample():
    codes, offsets = random_sample(_rng("wide", 0), [30000, 25000, 15000], 0.001)
    assert 69800 < len(codes) < 70000 and 50 < len(offsets) < 100
    return codes, offsets


@functools.lru_cache(maxsize=None)
def wide_case(k, rc):
    """One random sample of about 70 000 bases, three records, 0.1 % Ns; run at 2^20 bins."""
    return Case("wide", *wide_sample(), k, rc)


def check_wide(case, num_bins=WIDE):
    single = case.single_holders(num_bins)
    assert single.size > 50000 and 10 * int(single.sum()) >= 9 * single.size, (case.k, case.rc, int(single.sum()), single.size)


# ---- plain equality ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bins_sample():
    """(codes, offsets): 3 000 random bases in three records with a few Ns."""
    return random_sample(_rng("bins", 0), [1500, 1000, 500], 0.002)


def plain_case(codes, offsets, k, rc):
    return Case("plain", codes, offsets, k, rc)


def small_k_samples(k, rc):
    """The thread-boundary samples of k = 16 (codes and offsets), to be hashed at k = 1, 2, 3."""
    return [plain_case(c.codes, c.offsets, k, rc) for c in thread_boundary(16, True)]


# ---- every group of named cases ---------------------------------------------------------------------------------------------

STAGED_KS = (16, 17, 31, 32, 33, 128, 129)
STREAM_KS = (16, 17, 32, 33, 128, 129)     # pa = 30 and 0 at 16 / 17 and 32 / 33; da = 8, the look-ahead dword clamped, at 129
STREAM_K_RC = tuple((k, True) for k in STREAM_KS) + ((17, False), (129, False))
END_KS = (31, 129)
UNSTAGED_KS = (130, 256, 257, 300)         # 257 and 300: a window longer than a span
UNSTAGED_RC = {130: (True, False), 256: (True,), 257: (True, False), 300: (True,)}


def unstaged_boundary(k, rc):
    return thread_boundary(k, rc, span=USPAN, bins=(WIDE,))


def unstaged_ends(k, rc):
    lengths = (WG_STARTS - 1, WG_STARTS, WG_STARTS + 1, WG_STARTS + k - 1, WG_STARTS + k, WG_STARTS + USPAN + 1)
    return sample_ends(k, rc, bins=(WIDE,), lengths=lengths)


def groups():
    """{id: (bin counts, builder of [Case])} of every group of named cases the GPU tests run."""
    out = {}
    for rc in (True, False):
        for k in STAGED_KS:
            out[f"boundary-k{k}-rc{int(rc)}"] = (LDS_BINS, functools.partial(thread_boundary, k, rc))
        for k in END_KS:
            out[f"ends-k{k}-rc{int(rc)}"] = (LDS_BINS, functools.partial(sample_ends, k, rc))
        out[f"short-rc{int(rc)}"] = (LDS_BINS, functools.partial(short_and_empty, rc))
    for k, rc in STREAM_K_RC:
        out[f"lastthread-k{k}-rc{int(rc)}"] = (LDS_BINS, functools.partial(last_thread, k, rc))
    out["short-trailing"] = (LDS_BINS, functools.partial(short_and_empty, True, LDS_BINS, 2))
    out["batches"] = (LDS_BINS, batch_samples)
    for k in UNSTAGED_KS:
        for rc in UNSTAGED_RC[k]:
            out[f"unstaged-boundary-k{k}-rc{int(rc)}"] = ((WIDE,), functools.partial(unstaged_boundary, k, rc))
            out[f"unstaged-ends-k{k}-rc{int(rc)}"] = ((WIDE,), functools.partial(unstaged_ends, k, rc))
    return out


WIDE_K_RC = tuple((k, rc) for k in (15, 31, 129, 130) for rc in (True, False))


# ---- the flat arrays of a call --------------------------------------------------------------------------------------------

def pack(cases):
    """(codes, code_begin, offsets, offset_begin) of skl.sketch_signs for the samples of `cases`."""
    codes = np.concatenate([c.codes for c in cases]) if cases else np.zeros(0, np.uint8)
    cb = np.cumsum([0] + [len(c.codes) for c in cases])
    offs = np.concatenate([c.offsets for c in cases]) if cases else np.zeros(0, np.int64)
    ob = np.cumsum([0] + [len(c.offsets) for c in cases])
    return codes, cb, offs, ob
