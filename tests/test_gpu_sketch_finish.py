"""The device-side finish of sketch streams (csrc/sketch_finish.hip, launch rules in csrc/finish_plan.hpp): densify_bin and the
14-plane transpose on the GPU through skl_sketch_finish, skl_sketch_usigs_packed and skl_sketch_usigs_aa, against
oracle/sketcher.py's sequential densify_bin + fill_usigs on the same signs.

The signs are random below 2^61 - 1 with some forced to 2^61 - 2 and some to low 14 bits all zero / all one
(tests/finish_patterns.py).  Every comparison also asserts the flag bytes, so that a stream the library quietly finished on
the host (FINISH_UNFINISHED) cannot pass for the kernel.  Streams are at most a few thousand bins but for one case of three
streams of 2^20, whose expectation is cheap because few of their bins are empty."""
import subprocess

import numpy as np
import pytest

import finish_patterns as P
from oracle import sketcher

pytestmark = pytest.mark.gpu
LDS_MAX = 8192            # finish_plan.hpp FINISH_LDS_BINS_MAX (tests/test_finish_plan_cpu.py pins it)
CAP = 2048                # ... FINISH_MAX_ATTEMPTS
U64 = P.U64


def finish_and_check(skl, ctx, streams, want_unfinished=()):
    """streams: list of equal-length sign arrays.  Every stream against the oracle: words, first sign, flag."""
    signs = np.stack(streams)
    usigs, first, flags = skl.sketch_finish(ctx, signs)
    for s, stream in enumerate(streams):
        words, first_want, flag_want = P.expect(sketcher, stream)
        if s in want_unfinished:
            flag_want |= P.UNFINISHED
        assert flags[s] == flag_want, (s, int(flags[s]), flag_want, ctx.last_kernel())
        assert np.array_equal(usigs[s], words), (s, ctx.last_kernel())
        assert first[s] == first_want, (s, hex(int(first[s])), hex(int(first_want)))
    return usigs, first, flags


def form_is(ctx, num_bins):
    name = ctx.last_kernel()
    assert "sketch_finish_kernel" in name
    assert ("targets in LDS" in name) == (num_bins <= LDS_MAX) and ("targets in global memory" in name) == (num_bins > LDS_MAX), name


@pytest.mark.parametrize("num_bins", [64, 128, 1024, 1088, LDS_MAX, LDS_MAX + 64])
def test_sizes_and_forms(skl, gpu_ctx, num_bins):
    rng = np.random.default_rng(100 + num_bins)
    finish_and_check(skl, gpu_ctx, [P.pattern(p, num_bins, rng) for p in ("empty_50pct", "full", "empty_1pct", "first_half_empty")])
    form_is(gpu_ctx, num_bins)


@pytest.mark.parametrize("num_bins", [64, 1024, LDS_MAX + 64])
def test_patterns(skl, gpu_ctx, num_bins):
    """Full (densified clear, a plain transpose), one empty bin at either end, either half empty, half and 99 % of the bins
    empty: none of them falls back under the default cap."""
    rng = np.random.default_rng(200 + num_bins)
    streams = [P.pattern(p, num_bins, rng) for p in P.PATTERNS]
    usigs, _first, flags = finish_and_check(skl, gpu_ctx, streams)
    form_is(gpu_ctx, num_bins)
    assert flags[0] == 0 and np.array_equal(usigs[0], sketcher.fill_usigs(streams[0]))
    assert (flags[1:] == P.DENSIFIED).all()


@pytest.mark.parametrize("num_bins", [64, 128, 1024])
def test_single_non_empty_bin(skl, gpu_ctx, num_bins):
    """Worst probe counts 44, 108 and 918: below the cap of 2 048, so the kernel itself finishes them (the cap exceeds 1 433)."""
    assert CAP > 1433
    rng = np.random.default_rng(300 + num_bins)
    _u, first, flags = finish_and_check(skl, gpu_ctx, [P.pattern(p, num_bins, rng) for p in P.SINGLES])
    assert (flags == P.DENSIFIED).all()


@pytest.mark.parametrize("num_bins", [64, 1024, LDS_MAX + 64])
def test_all_empty_streams(skl, gpu_ctx, num_bins):
    rng = np.random.default_rng(400 + num_bins)
    streams = [P.pattern("empty_50pct", num_bins, rng), P.pattern("all_empty", num_bins, rng), P.pattern("bin0_empty", num_bins, rng)]
    usigs, first, flags = finish_and_check(skl, gpu_ctx, streams)
    assert flags[1] == P.EMPTY and not usigs[1].any() and first[1] == U64
    usigs, first, flags = skl.sketch_finish(gpu_ctx, np.full((5, num_bins), U64, dtype=np.uint64))
    assert (flags == P.EMPTY).all() and not usigs.any() and (first == U64).all()


def test_probe_cap_falls_back_to_the_host(skl, gpu_ctx, set_switch):
    """SKL_FINISH_MAX_ATTEMPTS=8: the 99 %-empty stream of 1 024 bins (139 probes on the reference) comes back finished by
    the host, the same bytes with the flag set, and its full neighbour untouched.  A call has one bin count, so the 50 %-empty
    stream of 64 bins (4 probes) shares its batch with a 64-bin stream of one non-empty bin (44 probes): the first stays on
    the device, the second falls back."""
    rng = np.random.default_rng(500)
    sparse, full = P.pattern("empty_99pct", 1024, rng), P.pattern("full", 1024, rng)
    easy, single = P.pattern("empty_50pct", 64, rng), P.pattern("single_last", 64, rng)
    native = lambda cap, s: int(subprocess.run([P.native(), "capped", str(cap)], input=s.tobytes(), capture_output=True, check=True).stdout)
    assert native(8, sparse) & P.UNFINISHED and native(8, single) & P.UNFINISHED and native(8, easy) == P.DENSIFIED   # the inputs are what the case needs
    default_big = finish_and_check(skl, gpu_ctx, [sparse, full])
    default_small = finish_and_check(skl, gpu_ctx, [easy, single, easy])
    assert list(default_big[2]) == [P.DENSIFIED, 0] and list(default_small[2]) == [P.DENSIFIED] * 3
    set_switch("SKL_FINISH_MAX_ATTEMPTS", 8)
    capped_big = finish_and_check(skl, gpu_ctx, [sparse, full], want_unfinished=(0,))
    capped_small = finish_and_check(skl, gpu_ctx, [easy, single, easy], want_unfinished=(1,))
    assert list(capped_big[2]) == [P.DENSIFIED | P.UNFINISHED, 0]
    assert list(capped_small[2]) == [P.DENSIFIED, P.DENSIFIED | P.UNFINISHED, P.DENSIFIED]
    for default, capped in ((default_big, capped_big), (default_small, capped_small)):
        assert np.array_equal(default[0], capped[0]) and np.array_equal(default[1], capped[1])


def test_many_small_streams(skl, gpu_ctx):
    """4 097 streams of 64 bins, a workgroup each: stream indexing."""
    rng = np.random.default_rng(600)
    names = ["empty_50pct", "full", "bin0_empty", "second_half_empty", "all_empty"]
    finish_and_check(skl, gpu_ctx, [P.pattern(names[s % len(names)], 64, rng) for s in range(4097)])
    form_is(gpu_ctx, 64)


def test_three_streams_of_a_million_bins(skl, gpu_ctx):
    """2^20 bins, global form: the scratch stride between the workgroups' target arrays.  A few hundred empty bins each (the
    oracle's loop is Python), among them bin 0 and the last."""
    n = 1 << 20
    rng = np.random.default_rng(700)
    streams = []
    for s in range(3):
        v = P.random_signs(rng, n)
        v[rng.choice(n, size=300, replace=False)] = U64
        v[0] = v[n - 1] = v[n // 2 + s] = U64
        streams.append(v)
    _u, _f, flags = finish_and_check(skl, gpu_ctx, streams)
    form_is(gpu_ctx, n)
    assert (flags == P.DENSIFIED).all()


def test_refuses_bins_that_are_no_multiple_of_64(skl, gpu_ctx):
    with pytest.raises(skl.SklError) as e:
        skl.sketch_finish(gpu_ctx, np.zeros((2, 1000), dtype=np.uint64))
    assert e.value.code == skl.ERR_INVALID_ARG
    with pytest.raises(skl.SklError) as e:
        skl.sketch_usigs_aa(gpu_ctx, np.ones(50, dtype=np.uint8), [0, 50], [5], 1000)
    assert e.value.code == skl.ERR_INVALID_ARG
    with pytest.raises(skl.SklError) as e:
        skl.sketch_usigs_packed(gpu_ctx, np.zeros(4, dtype=np.uint32), [0, 50], np.array([50]), [0, 1], [5], 1000)
    assert e.value.code == skl.ERR_INVALID_ARG


# ---- the sketching calls with the finish behind their bin minima ----

def dna_inputs():
    """Seven samples of 2 000 to 50 000 bases in a few records with some Ns, and one of 12 bases (shorter than either k)."""
    rng = np.random.default_rng(800)
    samples = []
    for length in (2000, 3100, 9000, 17000, 50000, 12, 26000, 4400):
        seq = rng.integers(0, 4, size=length, dtype=np.uint8)
        invalid = rng.random(length) < 0.001
        keep = ~invalid
        before = np.cumsum(keep) - keep
        offsets = np.concatenate([before[invalid], [int(keep.sum())]]).astype(np.int64)
        samples.append((seq[keep], offsets))
    codes = np.concatenate([c for c, _ in samples])
    cb = np.cumsum([0] + [len(c) for c, _ in samples])
    offs = np.concatenate([o for _, o in samples])
    ob = np.cumsum([0] + [len(o) for _, o in samples])
    return codes, cb, offs, ob


def aa_inputs(skl):
    """Proteins of 5 to 5 000 residues (most streams densified at 1 024 bins), one of 4 (shorter than either k)."""
    rng = np.random.default_rng(801)
    letters = np.frombuffer(skl.AA_LETTERS.encode(), dtype=np.uint8)
    lengths = [5, 9, 70, 300, 4, 1200, 5000, 41, 640, 2500]
    codes = [skl.aa_codes(letters[rng.integers(0, 20, size=n)].tobytes()) for n in lengths]
    return np.concatenate(codes), np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


def against_signs(signs, usigs, first, flags, empty_samples):
    for s in range(signs.shape[0]):
        for ki in range(signs.shape[1]):
            words, first_want, flag_want = P.expect(sketcher, signs[s, ki])
            assert flags[s, ki] == flag_want, (s, ki, int(flags[s, ki]), flag_want)
            assert np.array_equal(usigs[s, ki], words), (s, ki)
            assert first[s, ki] == first_want, (s, ki)
    assert [s for s in range(signs.shape[0]) if (flags[s] & P.EMPTY).any()] == list(empty_samples)


@pytest.mark.parametrize("batches", ["one_batch", "several_batches"])
def test_usigs_packed_equals_signs_then_oracle(skl, gpu_ctx, set_switch, batches):
    codes, cb, offs, ob = dna_inputs()
    packed = skl.pack_codes(codes, cb)
    kmers, num_bins = [17, 31], 1024
    signs = skl.sketch_signs_packed(gpu_ctx, packed, cb, offs, ob, kmers, num_bins, True)
    if batches == "several_batches":
        set_switch("SKL_SKETCH_BATCH_WORDS", 700)
    usigs, first, flags = skl.sketch_usigs_packed(gpu_ctx, packed, cb, offs, ob, kmers, num_bins, True)
    assert "nthash_binmin" in gpu_ctx.last_kernel() and "sketch_finish_kernel" in gpu_ctx.last_kernel() and "targets in LDS" in gpu_ctx.last_kernel()
    against_signs(signs, usigs, first, flags, empty_samples=[5])
    assert (flags[[0, 1]] & P.DENSIFIED).all()           # 2 000 and 3 100 bases leave empty bins among 1 024


@pytest.mark.parametrize("batches", ["one_batch", "several_batches"])
def test_usigs_aa_equals_signs_then_oracle(skl, gpu_ctx, set_switch, batches):
    residues, res_begin = aa_inputs(skl)
    kmers, num_bins = [5, 7], 1024
    signs = skl.sketch_signs_aa(gpu_ctx, residues, res_begin, kmers, num_bins)
    if batches == "several_batches":
        set_switch("SKL_AA_BATCH_SIGN_BYTES", 3 * 2 * 1024 * 8)      # three samples' worth of signs
    usigs, first, flags = skl.sketch_usigs_aa(gpu_ctx, residues, res_begin, kmers, num_bins)
    assert "aahash_binmin" in gpu_ctx.last_kernel() and "sketch_finish_kernel" in gpu_ctx.last_kernel()
    against_signs(signs, usigs, first, flags, empty_samples=[0, 4])        # 5 residues give no window at k = 7, 4 none at all
    assert flags[0, 0] == P.DENSIFIED and flags[0, 1] == P.EMPTY


def test_host_finish_gives_the_same_bytes(skl, gpu_ctx, set_switch):
    """SKL_SKETCH_FINISH=host on one mixed batch through all three calls."""
    rng = np.random.default_rng(900)
    streams = np.stack([P.pattern(p, 1024, rng) for p in P.PATTERNS + ["all_empty", "single_middle"]])
    codes, cb, offs, ob = dna_inputs()
    packed = skl.pack_codes(codes, cb)
    residues, res_begin = aa_inputs(skl)
    device = (skl.sketch_finish(gpu_ctx, streams), skl.sketch_usigs_packed(gpu_ctx, packed, cb, offs, ob, [17, 31], 1024, True),
              skl.sketch_usigs_aa(gpu_ctx, residues, res_begin, [5, 7], 1024))
    set_switch("SKL_SKETCH_FINISH", "host")
    host = (skl.sketch_finish(gpu_ctx, streams), skl.sketch_usigs_packed(gpu_ctx, packed, cb, offs, ob, [17, 31], 1024, True),
            skl.sketch_usigs_aa(gpu_ctx, residues, res_begin, [5, 7], 1024))
    assert "host" in gpu_ctx.last_kernel() and "sketch_finish_kernel" not in gpu_ctx.last_kernel()
    for d, h in zip(device, host):
        for a, b in zip(d, h):
            assert np.array_equal(a, b)
