"""Inputs for skl_sketch_signs_aa in which single windows decide their bins, and their expectation.  Pure numpy, no GPU:
tests/test_aa_edge_cases_cpu.py checks the properties claimed here on any machine, tests/test_gpu_sketch_aa_edges.py runs
the kernels of csrc/aa_sketch_kernel.hip on the same inputs.  The amino-acid counterpart of tests/sketch_edge_cases.py.

The output of the operation is a bin minimum, so on an ordinary input a kernel that drops, admits or mis-hashes ONE window
is caught only when that window happens to decide its bin.  Two constructions make it decide:

  * quiet background: a random word of period 7 over 7 distinct letters tiled to the sample's length, random residues
    over [e - k - 4, e + k + 4) around every edge position e of the case (a span or chunk boundary, a separator, the
    last start).  The background has at most 7 distinct windows, so nearly every window that touches a random stretch is
    alone in its bin;
  * wide bins: a fully random protein at 2^20 bins, where nearly every window is alone in its bin.

A sample is one byte string of the 20 letters with `*` for a separator (an invalid residue or a record end).

Expectation: window_table(seq, k, level) -- a NON-ROLLING hash, the XOR of srol^(k-1-i)(seed[c_i]) over the window, mod
SIGN_MOD, srol written as the rotation and bit swap of the reference's src/hashing/mod.rs:99-103 -- reduced with
np.minimum.at at bin_size = ceil(SIGN_MOD / num_bins).  tests/test_aa_edge_cases_cpu.py ties it to
aa_reference.natural_signs / signs_or_max (the rolling iterator with its split 31 / 33-bit tables) on every case.
Integers only.

A separator at position o breaks window s iff s <= o < s + k.  Under the END RULE (concat_end_rule = 1: the reference's
iterator as it is) the window at len - k is removed when len == k or residue len - k - 1 is a separator; when no window
is left the sample is all-max.

A Case is one sample at one k, one level and one end-rule setting with its NAMED starts: around every edge e and every
separator the starts e - k, e - k + 1, e - 1, e, e + 1, and under the end rule len - k.
  * valid: the named starts that are windows of the expectation.  Each must be the only window of its bin that has the
    bin's minimum: dropping or mis-hashing it changes the output;
  * invalid: those that hold a separator or are removed by the end rule.  The sign such a window would have -- the hash
    rolled straight through it, a separator contributing 0 as in the kernels -- must lie strictly below its bin's
    expected value (or the bin be empty): admitting it changes the output.
check() asserts all of this from the expectation alone; build() draws seeds (fixed base, the case's name, attempt 0, 1,
...) until it holds at every bin count the case is run at, so everything is deterministic.  Letters of a group share a
seed at levels 2 and 3, so equal signs of different windows are likelier there and build() simply draws again.  A
wide-bins case has no named starts: at least 90 % of ALL its windows must be single holders.

Not covered: k = 1 has 20 signs, so no window can be alone in its bin; the group-1 samples are compared for plain
equality there."""
import functools
import zlib

import numpy as np

import aa_reference as R

U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
SIGN_MOD = R.SIGN_MOD
BASE_SEED = 20261020
LETTERS = np.frombuffer(R.LETTERS.encode(), dtype=np.uint8)
SEP = ord("*")
# the shapes of csrc/aa_plan.hpp (tests/test_gpu_sketch_aa_edges.py asserts them against skl.sketch_aa_shape())
SPAN = 64                    # window starts per thread of the staged kernel
WG_LDS = 256                 # its threads per workgroup
CHUNK = SPAN * WG_LDS        # window starts per workgroup: 16 384
K_STAGED_MAX = 256
LDS_BINS_MAX = 4096
LONG_MIN = 8192
WG_SHORT = 256               # threads per workgroup of the unstaged kernel
LDS_BINS = (LDS_BINS_MAX, LDS_BINS_MAX + 1)      # the staged kernel with the minima in LDS / in global memory
UNSTAGED_BINS = (4096,)
WIDE = 1 << 20
MAX_ATTEMPTS = 400


def short_span(kmax):
    """Window starts per thread of the unstaged kernel: the longest k of the call in steps of 16, 16 to 256."""
    return min(256, (max(kmax, 1) + 15) // 16 * 16)


def bin_size_of(num_bins):
    return -(-SIGN_MOD // num_bins)


# ---- the non-rolling hash -------------------------------------------------------------------------------------------

_CODE = np.zeros(256, dtype=np.uint8)
for _i, _ch in enumerate(R.LETTERS):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i + 1


def codes_of(seq):
    """Class codes of a byte string: 1..20 for the letters, 0 for a separator."""
    return _CODE[np.frombuffer(bytes(seq), dtype=np.uint8)]


def srol(v):
    """One left rotation of the 64-bit word, then bits 0 and 33 swapped."""
    v = ((v << 1) | (v >> 63)) & 0xFFFFFFFFFFFFFFFF
    x = (v ^ (v >> 33)) & 1
    return v ^ (x | (x << 33))


_POWERS = {}


def seed_powers(level, k):
    """[k, 21] uint64: row n = srol^n(seed[code]); code 0, the separator, is 0 throughout."""
    rows = _POWERS.setdefault(level, [[0] + [R.SEED_TABLES[level][ch] for ch in R.LETTERS.encode()]])
    while len(rows) < k:
        rows.append([srol(v) for v in rows[-1]])
    return np.array(rows[:k], dtype=np.uint64)


def through_signs(codes, k, level=1):
    """[len - k + 1] uint64: the sign of EVERY start, a separator inside the window contributing 0."""
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64)
    powers = seed_powers(level, k)
    h = np.zeros(n, dtype=np.uint64)
    for i in range(k):
        h ^= powers[k - 1 - i][codes[i:i + n]]
    return h % np.uint64(SIGN_MOD)


def valid_starts(codes, k):
    """bool [len - k + 1]: no separator in the window (s <= o < s + k for no separator o)."""
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=bool)
    seps = np.concatenate([[0], np.cumsum(codes == 0)])
    return seps[k:k + n] == seps[:n]


def window_table(seq, k, level=1):
    """(starts, signs) of every window of k valid residues of the byte string `seq`."""
    codes = codes_of(seq)
    ok = valid_starts(codes, k)
    return np.flatnonzero(ok), through_signs(codes, k, level)[ok]


def reduce_to_bins(signs, num_bins):
    out = np.full(num_bins, U64_MAX, dtype=np.uint64)
    if signs.size:
        np.minimum.at(out, (signs // np.uint64(bin_size_of(num_bins))).astype(np.int64), signs)
    return out


# ---- a case -----------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, name, seq, k, level=1, end_rule=False, edges=(), named=True):
        self.name, self.seq, self.k, self.level, self.end_rule = name, bytes(seq), k, level, bool(end_rule)
        self.codes = codes_of(self.seq)
        self.codes.flags.writeable = False
        n = len(self.seq)
        self.breaks = np.flatnonzero(self.codes == 0)
        self.edges = sorted(set(edges) | set(self.breaks.tolist())) if named else []
        self.attempts = 1
        ok = valid_starts(self.codes, k)
        # the end rule takes the window at len - k away when nothing rolls into it
        self.ruled_out = self.end_rule and n >= k and (n == k or self.codes[n - k - 1] == 0)
        if self.ruled_out:
            ok = ok.copy()
            ok[n - k] = False
        self._ok = ok
        near = {s for e in self.edges for s in (e - k, e - k + 1, e - 1, e, e + 1)}
        if named and self.end_rule:
            near.add(n - k)
        near = sorted(s for s in near if 0 <= s <= n - k)
        self.valid = [s for s in near if ok[s]]
        self.invalid = [s for s in near if not ok[s]]
        self.named = named

    @functools.cached_property
    def through(self):
        return through_signs(self.codes, self.k, self.level)

    @functools.cached_property
    def table(self):
        """(starts, signs) of the windows of the expectation: window_table, less what the end rule removes."""
        return np.flatnonzero(self._ok), self.through[self._ok]

    def would_be_sign(self, s):
        """The sign a kernel that admitted start `s` would file: the hash rolled straight through its window."""
        return self.through[s]

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
        return reduce_to_bins(signs, num_bins)

    def single_holders(self, num_bins):
        """bool per window of the table: the only window of its bin with the bin's minimum."""
        starts, signs = self.table
        bins = (signs // np.uint64(bin_size_of(num_bins))).astype(np.int64)
        holds = signs == self.expectation(num_bins)[bins]
        per_bin = np.bincount(bins[holds], minlength=num_bins)
        return holds & (per_bin[bins] == 1)

    def problems(self, num_bins):
        """What keeps the case from being able to fail at its named starts ([] when nothing does)."""
        if not self.named:
            return []
        starts, _ = self.table
        single = self.single_holders(num_bins)
        exp = self.expectation(num_bins)
        bs = np.uint64(bin_size_of(num_bins))
        out = []
        if not self.valid and starts.size:
            out.append("no named valid start")
        if (self.breaks.size or self.ruled_out) and len(self.seq) >= self.k and not self.invalid:
            out.append("no named invalid start")
        for s in self.valid:
            i = int(np.searchsorted(starts, s))
            if not single[i]:
                out.append(f"valid start {s} does not decide its bin")
        for s in self.invalid:
            w = self.would_be_sign(s)
            if not w < exp[int(w // bs)]:
                out.append(f"invalid start {s} would not lower its bin")
        return out

    def check(self, num_bins):
        assert not self.problems(num_bins), (self.name, self.k, self.level, self.end_rule, num_bins, self.problems(num_bins))


def plain_case(name, seq, k, level=1, end_rule=False):
    """A sample without named starts: compared for plain equality."""
    return Case(name, seq, k, level, end_rule, named=False)


def _rng(name, attempt):
    return np.random.default_rng([BASE_SEED, zlib.crc32(name.encode()), attempt])


ATTEMPTS = {}      # name -> attempts build() needed (profiles/aa_edge_cases.md)


def build(name, bins, make):
    """make(rng) -> Case, with the first seed at which the case holds at every bin count of `bins`."""
    for attempt in range(MAX_ATTEMPTS):
        case = make(_rng(name, attempt))
        case.attempts = attempt + 1
        if not any(case.problems(nb) for nb in bins):
            break
    ATTEMPTS[name] = case.attempts
    return case   # (after MAX_ATTEMPTS the last one: check() then says what fails)


def random_letters(rng, n):
    return LETTERS[rng.integers(0, 20, size=n)]


def quiet_seq(rng, length, edges, k, breaks=()):
    word = LETTERS[rng.choice(20, size=7, replace=False)]
    seq = np.resize(word, length)
    for e in sorted(set(edges) | set(breaks)):
        lo, hi = max(e - k - 4, 0), min(e + k + 4, length)
        if lo < hi:
            seq[lo:hi] = random_letters(rng, hi - lo)
    for o in breaks:
        seq[o] = SEP
    return seq.tobytes()


def quiet_case(name, bins, length, k, breaks, edges, level=1, end_rule=False, stretch_k=None):
    """`edges` and the separators `breaks` get random stretches (sized by stretch_k, default k) and named starts."""
    breaks = [int(o) for o in breaks]
    assert all(0 <= o < length for o in breaks)
    all_edges = list(edges) + ([length - k] if end_rule else [])
    return build(f"{name}/k{k}/l{level}/e{int(end_rule)}/{'+'.join(map(str, bins))}", bins,
                 lambda rng: Case(name, quiet_seq(rng, length, all_edges, stretch_k or k, breaks), k, level, end_rule, all_edges))


# ---- break patterns ---------------------------------------------------------------------------------------------------

def break_patterns(p, k):
    """B(p, k): name -> separator positions of one sample each around the boundary p.  p - 1 is the last residue before
    the boundary, p the first window start behind it, p + k - 2 the last residue a window starting before p reads,
    p + k - 1 the first that none of them reads.  (At small k some coincide: the first name is kept.)"""
    named = {"none": [], "p-1": [p - 1], "p": [p], "p+1": [p + 1], "p-k": [p - k], "p+k-2": [p + k - 2],
             "p+k-1": [p + k - 1], "p+k": [p + k]}
    out, seen = {}, set()
    for name, pos in named.items():
        if tuple(pos) not in seen:
            seen.add(tuple(pos))
            out[name] = pos
    return out


def boundary_cases(tag, bins, p, length, k, level=1, end_rule=False, extra_edges=(), stretch_k=None):
    """One sample per pattern of B(p, k) that lies inside the sample ({p - k} does not at p = 128, k = 256)."""
    return [quiet_case(f"{tag}{p}:{name}", bins, length, k, pos, [p, *extra_edges], level, end_rule, stretch_k)
            for name, pos in break_patterns(p, k).items() if all(0 <= o < length for o in pos)]


# ---- group 1: staged thread boundary ------------------------------------------------------------------------------------

STAGED_THREAD_KS = (2, 5, 7, 8, 64, 65, 256)
THREAD_P = 2 * SPAN


@functools.lru_cache(maxsize=None)
def staged_thread_boundary(k):
    """Samples of 192 + k + 40 residues, the patterns B(128, k): the boundary between the second and third thread."""
    return boundary_cases("thread", LDS_BINS, THREAD_P, 3 * SPAN + k + 40, k)


@functools.lru_cache(maxsize=None)
def k1_samples():
    """The group-1 samples of k = 5, to be hashed at k = 1: plain equality."""
    return [plain_case(c.name, c.seq, 1) for c in staged_thread_boundary(5)]


# ---- group 2: staged chunk boundary -------------------------------------------------------------------------------------

CHUNK_KS = (2, 5, 64, 253, 254, 255, 256)     # 253 .. 256: the four byte lags of the entering residue at the far end of the extension
TWO_CHUNK_KS = (5, 256)


@functools.lru_cache(maxsize=None)
def chunk_boundary(k, level=1):
    """Samples of 16 384 + 64 + k + 9 residues, the patterns B(16 384, k): the windows of chunk 0's last thread read up to
    k - 1 residues past the chunk; {p + k - 2} is the last residue one of them reads, {p + k - 1} the first none reads."""
    return boundary_cases("chunk", LDS_BINS, CHUNK, CHUNK + SPAN + k + 9, k, level)


@functools.lru_cache(maxsize=None)
def two_chunk_boundaries(k):
    """One sample of 2 * 16 384 + 100 residues with edges at both chunk boundaries: chunk 0 is clipped by the staging
    limit, not by the sample's end."""
    return quiet_case("chunks2", LDS_BINS, 2 * CHUNK + 100, k, [], [CHUNK, 2 * CHUNK])


# ---- group 3: sample end ----------------------------------------------------------------------------------------------

END_KS = (3, 5, 20, 64)
END_PLACES = ("staged2", "chunk", "unstaged2")


def end_shape(place, k):
    """(span, m, bins) of a sample-end group."""
    return {"staged2": (SPAN, 2, LDS_BINS), "chunk": (SPAN, WG_LDS, LDS_BINS), "unstaged2": (short_span(k), 2, UNSTAGED_BINS)}[place]


def end_lengths(place, k):
    """m * span + k - 1 + {0, 1, 2}: the last window is a thread's last, first or second window."""
    span, m, _ = end_shape(place, k)
    return [m * span + k - 1 + d for d in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def sample_ends(place, k, end_rule):
    """[Case]: each length of end_lengths with residue len - k - 1 valid, then with a separator there."""
    _, _, bins = end_shape(place, k)
    out = []
    for length in end_lengths(place, k):
        for breaks in ([], [length - k - 1]):
            out.append(quiet_case(f"end-{place}{length}:{'sep' if breaks else 'valid'}", bins, length, k, breaks, [length - k],
                                  end_rule=end_rule))
    return out


# ---- group 4: unstaged thread boundary ----------------------------------------------------------------------------------

UNSTAGED_KS = (2, 5, 16, 17, 64, 257, 300)     # 257 and 300: past what the staged kernel takes, the span capped at 256
TWO_K_CALLS = ((3, 40), (5, 300))              # k = 3 at the span of 48, k = 5 at the span of 256


@functools.lru_cache(maxsize=None)
def unstaged_thread_boundary(k, kmax=None):
    """The patterns B(2 span, k) in samples of 3 span + kmax + 40 residues, span = short_span(kmax): named at k."""
    kmax = kmax or k
    span = short_span(kmax)
    return boundary_cases(f"uthread-kmax{kmax}-", UNSTAGED_BINS, 2 * span, 3 * span + kmax + 40, k)


def companions(cases, k):
    """The samples of `cases` at another k of the same call: plain equality."""
    return [plain_case(c.name, c.seq, k, c.level, c.end_rule) for c in cases]


# ---- group 5: unstaged packing ------------------------------------------------------------------------------------------

PACK_K = 5
PACK_FILLER_THREADS = (100, 1, 0, 100, 54)      # 255 threads in front of the first case
PACK_PATTERN_P = (16, 32)


@functools.lru_cache(maxsize=None)
def packed_samples():
    """([Case], indices of the named ones): samples of 48 residues (three spans of 16 at k = 5) with the patterns B(16, 5)
    and B(32, 5), each behind fillers that leave it the LAST thread of a workgroup: its first span boundary is the
    workgroup boundary, its second lies in the next workgroup."""
    span = short_span(PACK_K)
    assert sum(PACK_FILLER_THREADS) == WG_SHORT - 1
    named = [c for p in PACK_PATTERN_P for c in boundary_cases("packed", UNSTAGED_BINS, p, 3 * span, PACK_K, extra_edges=PACK_PATTERN_P)]
    out, at, threads = [], [], 0
    for i, c in enumerate(named):
        want = PACK_FILLER_THREADS if i == 0 else (WG_SHORT - 3 - 101, 1, 100)      # 253 threads behind a case of three
        for j, t in enumerate(want):
            n = max(t * span - (i + j) % span, (t - 1) * span + 1, 0)      # t threads: (t - 1) span < n <= t span
            out.append(plain_case(f"fill{i}.{j}:{n}", random_letters(_rng(f"fill{i}.{j}", 0), n).tobytes(), PACK_K))
            threads += t
        assert threads % WG_SHORT == WG_SHORT - 1
        at.append(len(out))
        out.append(c)
        threads += 3
    return out, at


# ---- group 6: levels ------------------------------------------------------------------------------------------------------

LEVEL_K = 5


def level_case(level):
    """The chunk-boundary sample with a separator at p + k - 2, at level 2 or 3."""
    return [c for c in chunk_boundary(LEVEL_K, level) if c.name.endswith(":p+k-2")]


# ---- group 7: wide bins -----------------------------------------------------------------------------------------------------

WIDE_KS = (5, 256)
WIDE_LENGTH, WIDE_SEPARATORS = 40000, 40


@functools.lru_cache(maxsize=None)
def wide_seq():
    rng = _rng("wide", 0)
    seq = random_letters(rng, WIDE_LENGTH)
    seq[rng.choice(WIDE_LENGTH, size=WIDE_SEPARATORS, replace=False)] = SEP
    return seq.tobytes()


@functools.lru_cache(maxsize=None)
def wide_case(k):
    """One random protein of 40 000 residues (three chunks) with 40 separators; run at 2^20 bins.  (One sample at a time:
    the signs are 8 MiB per sample and k.)"""
    return plain_case("wide", wide_seq(), k)


def wide_share(case, num_bins=WIDE):
    single = case.single_holders(num_bins)
    return int(single.sum()), single.size


def check_wide(case, num_bins=WIDE):
    holders, windows = wide_share(case, num_bins)
    assert windows > 10000 and 10 * holders >= 9 * windows, (case.k, holders, windows)


# ---- every group of named cases -----------------------------------------------------------------------------------------------

def groups():
    """{id: (bin counts, builder of [Case])} of every group of named cases the GPU tests run."""
    out = {}
    for k in STAGED_THREAD_KS:
        out[f"thread-k{k}"] = (LDS_BINS, functools.partial(staged_thread_boundary, k))
    for k in CHUNK_KS:
        out[f"chunk-k{k}"] = (LDS_BINS, functools.partial(chunk_boundary, k))
    for k in TWO_CHUNK_KS:
        out[f"chunks2-k{k}"] = (LDS_BINS, lambda k=k: [two_chunk_boundaries(k)])
    for place in END_PLACES:
        for k in END_KS:
            for end_rule in (False, True):
                out[f"end-{place}-k{k}-e{int(end_rule)}"] = (end_shape(place, k)[2], functools.partial(sample_ends, place, k, end_rule))
    for k in UNSTAGED_KS:
        out[f"uthread-k{k}"] = (UNSTAGED_BINS, functools.partial(unstaged_thread_boundary, k))
    for k, kmax in TWO_K_CALLS:
        out[f"uthread-k{k}-kmax{kmax}"] = (UNSTAGED_BINS, functools.partial(unstaged_thread_boundary, k, kmax))
    out["packed"] = (UNSTAGED_BINS, lambda: [packed_samples()[0][i] for i in packed_samples()[1]])
    for level in (2, 3):
        out[f"level{level}"] = (LDS_BINS, functools.partial(level_case, level))
    return out


# ---- the flat arrays of a call --------------------------------------------------------------------------------------------

def pack(cases):
    """(residue codes, res_begin) of skl.sketch_signs_aa for the samples of `cases`."""
    codes = np.concatenate([c.codes for c in cases]) if cases else np.zeros(0, np.uint8)
    return codes, np.cumsum([0] + [len(c.codes) for c in cases]).astype(np.uint64)


def misaligned(cases):
    """([Case], indices of the copies): every case four times, each copy behind a filler of 8 to 11 residues that puts its
    first residue at byte offset 0, 1, 2, 3 mod 4 of the call's residues (the staged kernel realigns such a sample)."""
    out, at, pos = [], [], 0
    for i, c in enumerate(cases):
        for r in range(4):
            n = 8 + (r - pos - 8) % 4
            out.append(plain_case(f"pad{i}.{r}", random_letters(_rng(f"pad{i}.{r}", 0), n).tobytes(), c.k, c.level, c.end_rule))
            pos += n
            assert pos % 4 == r
            at.append(len(out))
            out.append(c)
            pos += len(c.seq)
    return out, at
