"""An independent Python restatement of the reference's read sketching, written from its Rust sources
(src/hashing/nthash_iterator.rs, src/hashing/bloom_filter.rs, src/sketch/mod.rs): the bit-packed sequence
with its offsets, the iterator's `next` / `next_iterator` / roll, the blocked Bloom filter with its count
map, bin_sign, densification, the 14-plane transpose and the read-set length estimate.  Slow and literal;
used by tests/test_sketch_reads_cpu.py and tests/test_gpu_sketch_reads.py on small inputs."""
import functools
import gzip
import math

import numpy as np

M64 = (1 << 64) - 1
SIGN_MOD = (1 << 61) - 1
BBITS = 14
HASH_LOOKUP = [0x3c8bfbb395c60474, 0x3193c18562a02b4c, 0x295549f54be24456, 0x20323ed082572324]
RC_HASH_LOOKUP = [0x295549f54be24456, 0x20323ed082572324, 0x3c8bfbb395c60474, 0x3193c18562a02b4c]


def rotl1(v):
    return ((v << 1) | (v >> 63)) & M64


def rotr1(v):
    return ((v >> 1) | (v << 63)) & M64


def swapbits033(v):
    x = (v ^ (v >> 33)) & 1
    return v ^ (x | (x << 33))


def swapbits3263(v):
    x = ((v >> 32) ^ (v >> 63)) & 1
    return v ^ ((x << 32) | (x << 63))


@functools.lru_cache(maxsize=None)
def ms_tab(seed, k):
    """MS_TAB_31L[..k % 31] | MS_TAB_33R[..k % 33]: the seed split-rotated k times."""
    for _ in range(k):
        seed = swapbits033(rotl1(seed))
    return seed


def valid_base(b):
    return (b | 0x20) in b"acgtu"


def encode_base(b):
    return (b >> 1) & 3


def read_fastx(path):
    """[(seq bytes, qual bytes or None)] of a FASTA or four-line FASTQ file (gz or plain)."""
    with open(path, "rb") as fh:
        raw = fh.read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    lines = [l.rstrip(b"\r") for l in raw.split(b"\n")]
    recs = []
    if raw.lstrip()[:1] == b"@":
        lines = [l for l in lines if l]
        assert len(lines) % 4 == 0
        for i in range(0, len(lines), 4):
            assert lines[i][:1] == b"@" and lines[i + 2][:1] == b"+" and len(lines[i + 1]) == len(lines[i + 3])
            recs.append((lines[i + 1], lines[i + 3]))
        return recs, True
    seq = None
    for l in lines:
        if l[:1] == b">":
            if seq is not None:
                recs.append((bytes(seq), None))
            seq = bytearray()
        elif seq is not None:
            seq += l
    if seq is not None:
        recs.append((bytes(seq), None))
    return recs, False


class Packed:
    """NtHashIterator's sequence state after NtHashIterator::new (nthash_iterator.rs:94-141, 205-251)."""

    def __init__(self, files, min_qual):
        self.seq, self.offsets, self.acgt, self.non_acgt = [], [], [0, 0, 0, 0], 0
        self.reads = read_fastx(files[0])[1]
        if self.reads and len(files) > 2:
            raise ValueError("Input files are reads, but there are more than two input files")
        for f in files:
            self.add_dna_seq(f, min_qual)

    def add_dna_seq(self, path, min_qual):
        b, i = 0, 0
        for seq, qual in read_fastx(path)[0]:
            for idx, base in enumerate(seq):
                if valid_base(base) and (qual is None or qual[idx] >= min_qual):
                    e = encode_base(base)
                    self.acgt[e] += 1
                    b |= e
                    i += 1
                    if i > 3:
                        i = 0
                        self.seq.append(b)
                        b = 0
                    else:
                        b = (b << 2) & 0xFF
                else:
                    self.non_acgt += 1
                    self.offsets.append(len(self.seq) * 4 + i)
            self.offsets.append(len(self.seq) * 4 + i)
        if i != 0:
            self.seq.append((b << ((3 - i) * 2)) & 0xFF)

    def seq_len(self):
        return sum(self.acgt)


def unpack_byte(byte):
    return [(byte >> (6 - 2 * j)) & 3 for j in range(4)]


class NtHash:
    """The iterator (nthash_iterator.rs:325-388, 470-520) for one k."""

    def __init__(self, p, k, rc):
        self.p, self.k, self.rc = p, k, rc
        self.offset_idx = 0
        self.fh, self.rh, self.index = 0, None, 0
        if self.next_iterator(0) is None:
            raise ValueError("K-mer larger than smallest valid sequence")

    def next_iterator(self, start):
        p, k = self.p, self.k
        self.fh = 0
        end = start + k
        if self.offset_idx >= len(p.offsets):
            return None
        while self.offset_idx < len(p.offsets):
            cur = p.offsets[self.offset_idx]
            if cur < start or cur >= end:
                break
            self.offset_idx += 1
            start = cur
            end = start + k
        if start + k > p.seq_len():
            return None
        bases = []
        for h in range(k):
            bases.append(unpack_byte(p.seq[(start + h) // 4])[(start + h) % 4])
        fh = 0
        for base in bases:
            fh = swapbits033(rotl1(fh)) ^ HASH_LOOKUP[base]
        self.fh = fh
        if self.rc:
            h = 0
            for base in reversed(bases):
                h = swapbits033(rotl1(h)) ^ RC_HASH_LOOKUP[base]
            self.rh = h
        else:
            self.rh = None
        self.front = unpack_byte(p.seq[end // 4])
        self.back = unpack_byte(p.seq[start // 4])
        self.index = end
        return True

    def curr(self):
        return min(self.fh, self.rh) if self.rh is not None else self.fh

    def roll_fwd(self, old, new):
        k = self.k
        self.fh = swapbits033(rotl1(self.fh)) ^ HASH_LOOKUP[new] ^ ms_tab(HASH_LOOKUP[old], k)
        if self.rh is not None:
            h = self.rh ^ ms_tab(HASH_LOOKUP[new ^ 2], k)   # rc_base(new) = new ^ 2 (hashing/mod.rs:88-90)
            h ^= RC_HASH_LOOKUP[old]
            self.rh = swapbits3263(rotr1(h))

    def __iter__(self):
        p, k = self.p, self.k
        L = p.seq_len()
        while True:
            if self.index < L:
                cur = self.curr()
                if self.offset_idx < len(p.offsets) and p.offsets[self.offset_idx] == self.index:
                    if self.next_iterator(self.index) is None:
                        self.index = L + 1
                else:
                    new = self.front[self.index % 4]
                    old = self.back[(self.index - k) % 4]
                    self.roll_fwd(old, new)
                    self.index += 1
                    if self.index % 4 == 0 and self.index < L:
                        self.front = unpack_byte(p.seq[self.index // 4])
                    if (self.index - k) % 4 == 0:
                        self.back = unpack_byte(p.seq[(self.index - k) // 4])
                yield cur
            elif self.index == L:
                self.index += 1
                yield self.curr()
            else:
                return


class KmerFilter:
    """bloom_filter.rs: blocked Bloom filter (sparse here), then a count map from 2."""

    BUF_SIZE = round((1 << 27) * (12 / 8) / 64)

    def __init__(self, min_count):
        self.min_count = min_count
        self.clear()

    def clear(self):
        self.buffer, self.counts = {}, {}

    def bloom_add_and_check(self, key):
        fp = 0
        for sh in (0, 6, 12, 18, 24):
            fp |= 1 << ((key >> sh) & 63)
        mixed = ((key ^ (key >> 31)) * 0x85D059AA333121CF) & M64
        loc = (mixed * self.BUF_SIZE) >> 64
        word = self.buffer.get(loc, 0)
        if word & fp == fp:
            return True
        self.buffer[loc] = word | fp
        return False

    def equal(self, h):
        if self.min_count in (0, 1):
            return True
        if self.min_count == 2:
            return self.bloom_add_and_check(h)
        if not self.bloom_add_and_check(h):
            return False
        count = min(self.counts[h] + 1, 0xFFFF) if h in self.counts else 2
        self.counts[h] = count
        return count == self.min_count


def universal_hash(s, t):
    x = (s * 1009 + t * (1000 * 1000 + 3)) & M64
    return ((x * 48271 + 11) & M64) % ((1 << 31) - 1)


def densify(signs):
    if max(signs) != M64:
        return False
    for i in range(len(signs)):
        j, n = i, 0
        while signs[j] == M64:
            j = universal_hash(i, n) % len(signs)
            n += 1
        signs[i] = signs[j]
    return True


def fill_usigs(signs):
    out = [0] * (len(signs) // 64 * BBITS)
    for idx, s in enumerate(signs):
        for b in range(BBITS):
            out[idx // 64 * BBITS + b] |= ((s >> b) & 1) << (idx % 64)
    return out


def sketch_sample(files, kmers, sketch_size, rc=True, min_count=5, min_qual=20):
    """Sketch::new for one sample -> (usigs list, metadata dict)."""
    p = Packed(files, min_qual)
    num_bins = (sketch_size + 63) // 64 * 64
    bin_size = (SIGN_MOD + num_bins - 1) // num_bins
    filt = KmerFilter(min_count) if p.reads else None
    usigs, minhash_sum, densified = [], 0.0, False
    for k in kmers:
        signs = [M64] * num_bins
        if filt is not None:
            filt.clear()
        for h in NtHash(p, k, rc):
            sign = h % SIGN_MOD
            b = sign // bin_size
            if filt is not None:
                if sign < signs[b] and filt.equal(sign):
                    signs[b] = sign
            else:
                signs[b] = min(signs[b], sign)
        densified |= densify(signs)
        minhash_sum += signs[0] / SIGN_MOD
        usigs += fill_usigs(signs)
    if p.reads:
        v = len(kmers) / minhash_sum if minhash_sum else math.inf
        seq_length = 0 if math.isnan(v) else (M64 if v >= 2.0 ** 64 else int(v))
    else:
        seq_length = p.seq_len()
    return usigs, dict(seq_length=seq_length, reads=p.reads, densified=densified, acgt=p.acgt, non_acgt=p.non_acgt)


def sketch_skd(samples, kmers, sketch_size, rc=True, min_count=5, min_qual=20):
    """The .skd bytes of `samples` ([files] each) and their metadata."""
    words, metas = [], []
    for files in samples:
        u, m = sketch_sample(files, kmers, sketch_size, rc, min_count, min_qual)
        words += u
        metas.append(m)
    return np.array(words, dtype="<u8").tobytes(), metas


def window_signs(files, k, rc=True, min_qual=20):
    """[(window start in the padded coordinates, sign)] of every valid window, in stream order, with the packed
    codes / offsets the device takes (codes cut at seq_len, offsets past it dropped)."""
    p = Packed(files, min_qual)
    L = p.seq_len()
    codes = np.array([unpack_byte(b)[j] for b in p.seq for j in range(4)][:L], dtype=np.uint8)
    it = NtHash(p, k, rc)
    out = []
    for h in it:
        out.append(h % SIGN_MOD)
    # starts: the windows the iterator yields are exactly those with no offset strictly inside, s + k <= L
    offs = [o for o in p.offsets if o <= L]
    starts = [s for s in range(0, L - k + 1) if not any(s < o < s + k for o in offs)]
    assert len(starts) == len(out)
    return list(zip(starts, out)), codes, np.array(offs, dtype=np.uint64)


def window_table(codes, offsets, k, rc=True):
    """(starts int64[], signs uint64[]) of every valid window of one sample given as arrays, in start order: start s is
    valid iff s + k <= len(codes) and no offset o has s < o < s + k; the signs are the oracle's non-rolling hashes
    (oracle/sketcher.py kmer_hashes, pinned on the reference's .skd files) mod SIGN_MOD.  The vectorised counterpart
    of window_signs; tests/test_sketch_reads_cpu.py ties the two together."""
    from oracle.sketcher import kmer_hashes

    codes = np.asarray(codes, dtype=np.uint8)
    offs = np.sort(np.asarray(offsets, dtype=np.int64))
    cand = np.arange(max(len(codes) - k + 1, 0), dtype=np.int64)
    first_after = np.searchsorted(offs, cand, side="right")      # the first offset strictly above s ...
    nxt = np.append(offs, np.iinfo(np.int64).max)[first_after]
    starts = cand[nxt >= cand + k]                               # ... must not lie below s + k
    signs = kmer_hashes(codes, offs, k, rc) % np.uint64(SIGN_MOD)
    assert starts.size == signs.size
    return starts, signs


def random_genome(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes()


def write_fastq(path, reads):
    """reads: [(seq bytes, qual bytes)] -> a gzip'd four-line FASTQ file."""
    with gzip.open(path, "wb", compresslevel=1) as fh:
        for i, (s, q) in enumerate(reads):
            fh.write(b"@r%d\n%s\n+\n%s\n" % (i, s, q))


def synthetic_reads(rng, genome, n_reads, read_len, sub_rate=0.01, n_rate=0.0, lowq_rate=0.0, low_q=b"#", high_q=b"I"):
    """Reads sampled from both strands of `genome` (bytes of ACGT) with substitutions, N and low-quality bases."""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    out = []
    for _ in range(n_reads):
        ln = int(read_len) if np.isscalar(read_len) else int(rng.integers(read_len[0], read_len[1] + 1))
        p = int(rng.integers(0, len(genome) - ln + 1))
        s = bytearray(genome[p:p + ln])
        if rng.random() < 0.5:
            s = bytearray(bytes(s).translate(comp)[::-1])
        for i in np.nonzero(rng.random(ln) < sub_rate)[0]:
            s[i] = b"ACGT"[int(rng.integers(0, 4))]
        for i in np.nonzero(rng.random(ln) < n_rate)[0]:
            s[i] = ord("N")
        q = bytearray(high_q * ln)
        for i in np.nonzero(rng.random(ln) < lowq_rate)[0]:
            q[i] = low_q[0]
        out.append((bytes(s), bytes(q)))
    return out


def kept_bases(reads, min_qual):
    return sum(1 for s, q in reads for b, x in zip(s, q) if valid_base(b) and x >= min_qual)


def pad_to_residue(reads, min_qual, residue):
    """Append one high-quality read so that the kept bases number `residue` mod 4 (1, 2 or 3)."""
    extra = (residue - kept_bases(reads, min_qual)) % 4 or 4
    return reads + [(b"ACGTACGT"[:extra], b"I" * extra)]
