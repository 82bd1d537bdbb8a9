"""Amino-acid sketching as the reference does it, restated in Python (TEST INFRASTRUCTURE ONLY).

This file RESTATES the reference; NO REFERENCE BINARY HAS CONFIRMED IT (the reference cannot be built where these tests run,
and its own test of the mode, tests/sketch.rs:102-140, only checks that the runs succeed).  It is a line-by-line
transliteration, kept as close to the Rust as Python allows so that it can be read side by side with it:

  * valid_aa, srol                               src/hashing/aahash_iterator.rs:9-21
  * AaHashIterator::new (FASTA loading)          src/hashing/aahash_iterator.rs:84-124
  * AaHashIterator::new_iterator / set_k         src/hashing/aahash_iterator.rs:35-46,138-166
  * roll_fwd, Iterator::next                     src/hashing/aahash_iterator.rs:169-210
  * aa_seed_table / aa_roll_table                src/hashing/aahash_tables.rs:9-35
  * get_signs_no_densify / get_signs, Sketch::new, sketch_files (names, "has no valid sequence")
                                                 src/sketch/mod.rs:74-176,330-375

The seeds are the published aaHash constants (doi:10.1093/bioadv/vbad162).  The roll tables are built HERE the way the
reference's tables are laid out -- a 33-bit right half and a 31-bit left half, each rotated within itself, indexed by k % 33
and k % 31 and OR-ed -- while the C++ under test applies srol k times to the whole word.  The two derivations check each other.
densify_bin and fill_usigs are oracle/sketcher.py's (pinned against the reference's committed .skd files)."""
import gzip

import numpy as np

from oracle import sketcher as S

SIGN_MOD = S.SIGN_MOD
U64 = (1 << 64) - 1
SEQSEP = 5                       # src/hashing/mod.rs:14
LETTERS = "ACDEFGHIKLMNPQRSTVWY"

_L1 = dict(A=0xf56d6192468323df, C=0x9b0b2fd724e1e1d2, D=0xe8c583296b03c7af, E=0x6d8186850ee2f67, F=0x921e1da156b717ad,
           G=0xa70dc450015e3ffe, H=0x2242263a9d5638ff, I=0x2469ca06d519cdef, K=0xd4e7f06ac0593d3b, L=0xa5e19c0b1b40a97f,
           M=0xfab3d6d4dd74c000, N=0x4b363f2cf7bc5200, P=0x21ac8af2adb65ce4, Q=0x1d3baae9ab7cd800, R=0x49015253a9dbedf,
           S=0x5bf1f1d7ae699000, T=0xdb0c63dd7282cf90, V=0x7df64ddf78874000, W=0xee9e700cae6aa279, Y=0x5852ffb781a97610)
_L2_GROUPS = {"C": 0x1d07fd644abe9962, "G": 0xf59c50929bdf4360, "A": 0x6f735c82fe9c6c03, "TS": 0xe7392f0ba1dbc3b0,
              "N": 0x956ddcfcd4b3961f, "DE": 0x4ec0ef1bac4f5efa, "QKR": 0x1cd6ca491872ed78, "VILM": 0x547ef17894921035,
              "WFY": 0x419722edb87bf79f, "H": 0xdd5cce5bfdc32de1, "P": 0x90e0c5e0c07d6598}
_L3_GROUPS = {"C": 0x5713e4c10cebbfa3, "G": 0xbe084b869537379b, "ATS": 0x985fd9efa0fe5b82, "NDE": 0x9aca6c4f4ef69df0,
              "QKR": 0x917de473b721df0e, "VILM": 0x37cdd84aa07c5bd7, "WFY": 0x51a7955f1a67a896, "H": 0x1d2a0ba493708fbf,
              "P": 0xfe4c47da16611245}


def _seed_table(by_letter):
    """[u64; 256]: both cases of a letter, 0 everywhere else (aahash_tables.rs:60-125)."""
    t = [0] * 256
    for letter, seed in by_letter.items():
        t[ord(letter)] = t[ord(letter.lower())] = seed
    return t


SEED_TABLES = {1: _seed_table(_L1),
               2: _seed_table({ch: v for g, v in _L2_GROUPS.items() for ch in g}),
               3: _seed_table({ch: v for g, v in _L3_GROUPS.items() for ch in g})}
for _t in SEED_TABLES.values():
    assert sorted(chr(i) for i in range(256) if _t[i] and chr(i).isupper()) == sorted(LETTERS)


def _rotl_within(v, bits, by):
    by %= bits
    return ((v << by) | (v >> (bits - by))) & ((1 << bits) - 1)


def _split_roll_tables(seed):
    """(RIGHT_33BITS_ROLL_TABLE[33], LEFT_31BITS_ROLL_TABLE[31]) of one seed: entry i = that half rotated left by i within
    itself, the left half kept in bits 33..63 (aahash_tables.rs:127-194)."""
    right, left = seed & ((1 << 33) - 1), seed >> 33
    return [_rotl_within(right, 33, i) for i in range(33)], [_rotl_within(left, 31, i) << 33 for i in range(31)]


_ROLL = {lvl: {seed: _split_roll_tables(seed) for seed in set(tab)} for lvl, tab in SEED_TABLES.items()}


_VALID = frozenset((LETTERS + LETTERS.lower()).encode())


def valid_aa(aa):
    return aa in _VALID


def srol(x):
    m = ((x & 0x8000000000000000) >> 30) | ((x & 0x100000000) >> 32)
    return ((x << 1) & 0xFFFFFFFDFFFFFFFF & U64) | m


def aa_seed_table(level, aa):
    return SEED_TABLES[level][aa]


def aa_roll_table(level, aa, k):
    rot_31 = k if k < 31 else k % 31
    rot_33 = k if k < 33 else k % 33
    right, left = _ROLL[level][SEED_TABLES[level][aa]]
    return left[rot_31] | right[rot_33]


class ReferencePanic(Exception):
    pass


def read_fasta_records(path):
    """[(sequence bytes, has quality)] of a FASTA / FASTQ file as needletail yields them (line ends stripped)."""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        data = f.read()
    if data.lstrip()[:1] == b"@":
        return [(b"", True)]
    records = []
    for rec in data.split(b">")[1:]:
        nl = rec.find(b"\n")
        body = rec[nl + 1:] if nl >= 0 else b""
        records.append((body.replace(b"\n", b"").replace(b"\r", b""), False))
    return records


class AaHashIterator:
    def __init__(self, level):
        self.k = 0
        self.level = level
        self.fh = 0
        self.index = 0
        self.seq = []
        self.invalid_count = 0

    @staticmethod
    def new(files, level, concat_fasta, records_of=read_fasta_records):
        hash_vec = []
        seq_hash_it = AaHashIterator(level)
        for file in files:
            for seq, has_qual in records_of(file):
                if has_qual:
                    raise ReferencePanic(f"Unexpected quality information with AA sequences in {file}. Correct sequence type set?")
                for aa in seq:
                    if valid_aa(aa):
                        seq_hash_it.seq.append(aa)
                    else:
                        seq_hash_it.invalid_count += 1
                        seq_hash_it.seq.append(SEQSEP)
                if concat_fasta:
                    hash_vec.append(seq_hash_it)
                    seq_hash_it = AaHashIterator(level)
                else:
                    seq_hash_it.seq.append(SEQSEP)
        if not concat_fasta:
            hash_vec.append(seq_hash_it)
        return hash_vec

    @staticmethod
    def new_iterator(start, level, seq, k):
        if len(seq) < k:
            raise ReferencePanic("attempt to subtract with overflow")     # seq.len() - k on usize
        fh = 0
        while start < len(seq) - k:
            restart = False
            for i, v in enumerate(seq[start:start + k]):
                if not valid_aa(v):
                    start += i + 1
                    if start >= len(seq):
                        return None
                    fh = 0
                    restart = True
                    break
                fh = srol(fh)
                fh ^= aa_seed_table(level, v)
            if restart:
                continue
            break
        if start >= len(seq) - k:
            return None
        return fh, start + k

    def set_k(self, k):
        self.k = k
        new_it = self.new_iterator(0, self.level, self.seq, k)
        if new_it is None:
            raise ReferencePanic("K-mer larger than smallest valid sequence, which is:\n" + bytes(self.seq).decode("latin-1"))
        self.fh, self.index = new_it

    def roll_fwd(self, old_aa, new_aa):
        self.fh = srol(self.fh)
        self.fh ^= aa_seed_table(self.level, new_aa)
        self.fh ^= aa_roll_table(self.level, old_aa, self.k)

    def next(self):
        if self.index < len(self.seq):
            current = self.fh
            new_aa = self.seq[self.index]
            if not valid_aa(new_aa):
                new_it = self.new_iterator(self.index + 1, self.level, self.seq, self.k)
                if new_it is not None:
                    self.fh, self.index = new_it
                else:
                    self.index = len(self.seq)
            else:
                self.roll_fwd(self.seq[self.index - self.k], new_aa)
                self.index += 1
            return current
        if self.index == len(self.seq):
            self.index += 1
            return self.fh
        return None

    def hashes(self, k):
        """Every hash the iterator yields at k, in order (set_k, then next() until None)."""
        self.set_k(k)
        out = []
        while True:
            h = self.next()
            if h is None:
                return out
            out.append(h)


def get_signs_no_densify(it, k, num_bins):
    """sketch/mod.rs:156-176: u64 [num_bins], u64::MAX for an empty bin."""
    bin_size = -(-SIGN_MOD // num_bins)
    signs = [U64] * num_bins
    for h in it.hashes(k):
        sign = h % SIGN_MOD
        b = sign // bin_size
        signs[b] = min(signs[b], sign)
    return np.array(signs, dtype=np.uint64)


def iterator_of(seq, level=1):
    """An iterator over stored residues given as bytes / str (anything that is not one of the 20 letters is stored as a
    separator, as `new` stores it)."""
    it = AaHashIterator(level)
    for aa in (seq.encode() if isinstance(seq, str) else bytes(seq)):
        if valid_aa(aa):
            it.seq.append(aa)
        else:
            it.invalid_count += 1
            it.seq.append(SEQSEP)
    return it


def signs_or_max(seq, k, num_bins, level=1):
    """get_signs_no_densify of stored residues; all-max where the reference panics in set_k (no seedable window, a sequence
    shorter than k): what skl_sketch_signs_aa documents for such a sample under the end rule."""
    try:
        return get_signs_no_densify(iterator_of(seq, level), k, num_bins)
    except ReferencePanic:
        return np.full(num_bins, U64, dtype=np.uint64)


def natural_signs(seq, k, num_bins, level=1):
    """Bin minima over EVERY window of k valid residues (concat_end_rule = 0): the iterator run on the sequence with one
    separator appended -- every window then starts before len - k, and the separator adds no window."""
    seq = seq.encode() if isinstance(seq, str) else bytes(seq)
    if len(seq) < k:
        return np.full(num_bins, U64, dtype=np.uint64)
    return signs_or_max(seq + b"*", k, num_bins, level)


def sketch_files(inputs, kmers, sketch_size, level=1, concat_fasta=False, rc=True):
    """sketch_files + Sketch::new for [(name, [files])]: (usigs [n_samples, nk * ss64 * 14] in .skd order,
    [(name, seq_length, non_acgt, densified)])."""
    ss64 = -(-sketch_size // 64)
    num_bins = ss64 * 64
    rows, meta = [], []
    for name, files in inputs:
        for idx, it in enumerate(AaHashIterator.new(files, level, concat_fasta)):
            sample_name = f"{name}_{idx + 1}" if concat_fasta else name
            if len(it.seq) == 0:
                raise ReferencePanic(f"{sample_name} has no valid sequence")
            words, densified = [], False
            for k in sorted(kmers):
                signs = get_signs_no_densify(it, k, num_bins)
                densified |= S.densify_bin(signs)
                words.append(S.fill_usigs(signs))
            rows.append(np.concatenate(words))
            meta.append((sample_name, len(it.seq), it.invalid_count, densified))
    return np.stack(rows), meta
