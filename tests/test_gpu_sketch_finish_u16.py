"""The u16 form of the device-side finish (csrc/sketch_finish.hip, launch rules in csrc/finish_plan.hpp): densify_bin and `sign as
u16` for ANY bin count through skl_sketch_finish_u16 and skl_sketch_bins_u16_packed, against oracle/sketcher.py's sequential
densify_bin cut to 16 bits (tests/finish_u16_patterns.py).

Every comparison also asserts the flag byte and last_kernel, so that a stream the library quietly finished on the host
(FINISH_UNFINISHED, or SKL_SKETCH_FINISH=host) cannot pass for the kernel.  The probe counts the cases rely on are asserted on
the inputs first, on the CPU, with finish_plan_check's `capped` mode (finish_target's rule under a cap)."""
import subprocess

import numpy as np
import pytest

import finish_patterns as P
import finish_u16_patterns as Q
from test_gpu_sketch_finish import dna_inputs

pytestmark = pytest.mark.gpu
LDS_MAX = 8192            # finish_plan.hpp FINISH_LDS_BINS_MAX
CAP = 2048                # ... FINISH_MAX_ATTEMPTS
U64 = P.U64


def capped(cap, signs):
    """The flag the two steps give this stream when a bin may probe `cap` times (CPU)."""
    return int(subprocess.run([P.native(), "capped", str(cap)], input=np.ascontiguousarray(signs, dtype=np.uint64).tobytes(),
                              capture_output=True, check=True).stdout)


def form_is(ctx, num_bins):
    name = ctx.last_kernel()
    assert "sketch_finish_kernel" in name and "u16 bins" in name and "host" not in name, name
    assert ("targets in LDS" in name) == (num_bins <= LDS_MAX) and ("targets in global memory" in name) == (num_bins > LDS_MAX), name


def finish_and_check(skl, ctx, streams, want_unfinished=()):
    signs = np.stack(streams)
    bins, flags = skl.sketch_finish_u16(ctx, signs)
    form_is(ctx, signs.shape[1])
    assert bins.shape == signs.shape and bins.dtype == np.uint16
    for s, stream in enumerate(streams):
        row, flag_want = Q.expect(stream)
        if s in want_unfinished:
            flag_want |= P.UNFINISHED
        assert flags[s] == flag_want, (s, int(flags[s]), flag_want, ctx.last_kernel())
        assert np.array_equal(bins[s], row), (s, np.nonzero(bins[s] != row)[0][:8])
    return bins, flags


@pytest.mark.parametrize("num_bins", [1, 2, 10, 63, 64, 65, 1000, 1001, LDS_MAX, LDS_MAX + 1])
def test_sizes_and_patterns(skl, gpu_ctx, num_bins):
    """Targets in LDS up to 8 192 bins, in global scratch at 8 193.  At most 54 probes per bin (CPU count below a cap of 54), so
    the kernel finishes every stream itself: the flag is DENSIFIED exactly wherever a bin was empty."""
    rng = np.random.default_rng(1100 + num_bins)
    streams, names = [], []
    for name in Q.PATTERNS:
        v = P.pattern(name, num_bins, rng)
        if not Q.is_all_empty(v):                 # (bin0_empty at one bin is the all-empty stream: test_all_empty_streams)
            streams.append(v)
            names.append(name)
    assert len(streams) >= 3
    for v in streams:
        assert not capped(54, v) & P.UNFINISHED
    _bins, flags = finish_and_check(skl, gpu_ctx, streams)
    for name, v, flag in zip(names, streams, flags):
        assert flag == (P.DENSIFIED if (v == U64).any() else 0), name


def test_three_streams_of_a_million_bins(skl, gpu_ctx):
    """2^20 bins, global targets, workgroups of 1 024 threads: a few hundred empty bins each, among them bin 0 and the last."""
    n = 1 << 20
    rng = np.random.default_rng(1200)
    streams = []
    for s in range(3):
        v = P.random_signs(rng, n)
        v[rng.choice(n, size=300, replace=False)] = U64
        v[0] = v[n - 1] = v[n // 2 + s] = U64
        streams.append(v)
    _bins, flags = finish_and_check(skl, gpu_ctx, streams)
    assert (flags == P.DENSIFIED).all()


@pytest.mark.parametrize("num_bins", [10, 63, 65, 1001])
def test_single_non_empty_bin_on_the_device(skl, gpu_ctx, num_bins):
    """12, 45, 78 and 568 probes at these sizes: under the cap, the device finishes them."""
    rng = np.random.default_rng(1300 + num_bins)
    streams = [P.pattern(p, num_bins, rng) for p in P.SINGLES]
    for v in streams:
        assert capped(CAP, v) == P.DENSIFIED
    _bins, flags = finish_and_check(skl, gpu_ctx, streams)
    assert (flags == P.DENSIFIED).all()


@pytest.mark.parametrize("num_bins", [100, 1000])
def test_single_non_empty_bin_past_the_cap_falls_back_to_the_host(skl, gpu_ctx, num_bins):
    """The universal hash covers multiples of ten badly: 4 662 - 11 662 probes at 100 bins, 12 894 - 21 574 at 1 000, over the
    cap of 2 048.  The stream comes back DENSIFIED | UNFINISHED with the host's bytes, its full neighbour untouched."""
    rng = np.random.default_rng(1400 + num_bins)
    full = P.pattern("full", num_bins, rng)
    assert capped(CAP, full) == 0
    for name in P.SINGLES:
        single = P.pattern(name, num_bins, rng)
        assert capped(CAP, single) & P.UNFINISHED and capped(0, single) == P.DENSIFIED    # the inputs are what the case needs
        _bins, flags = finish_and_check(skl, gpu_ctx, [single, full], want_unfinished=(0,))
        assert list(flags) == [P.DENSIFIED | P.UNFINISHED, 0]


@pytest.mark.parametrize("num_bins", [10, 65, 1000, LDS_MAX + 1])
def test_low_16_bits_all_one_are_a_value(skl, gpu_ctx, num_bins):
    """Signs whose low 16 bits are 0xFFFF next to empty bins: they are filled from, never filled."""
    rng = np.random.default_rng(1500 + num_bins)
    v = P.random_signs(rng, num_bins) | np.uint64(0xFFFF)
    v[::2] = U64
    w = P.random_signs(rng, num_bins)
    w[1::3] |= np.uint64(0xFFFF)
    w[2::3] = U64
    bins, flags = finish_and_check(skl, gpu_ctx, [v, w])
    assert (bins[0] == 0xFFFF).all() and (flags == P.DENSIFIED).all()


@pytest.mark.parametrize("num_bins", [1, 10, 1000, LDS_MAX + 1])
def test_all_empty_streams(skl, gpu_ctx, num_bins):
    rng = np.random.default_rng(1600 + num_bins)
    streams = [P.pattern("full", num_bins, rng), P.pattern("all_empty", num_bins, rng), P.pattern("empty_50pct", num_bins, rng)]
    bins, flags = finish_and_check(skl, gpu_ctx, streams)
    assert flags[1] == P.EMPTY and not bins[1].any()
    bins, flags = skl.sketch_finish_u16(gpu_ctx, np.full((5, num_bins), U64, dtype=np.uint64))
    form_is(gpu_ctx, num_bins)
    assert (flags == P.EMPTY).all() and not bins.any()


def test_many_short_streams(skl, gpu_ctx):
    """4 097 streams of 10 bins, a workgroup each: stream indexing at a 20-byte row stride."""
    rng = np.random.default_rng(1700)
    names = ["empty_50pct", "full", "bin0_empty", "second_half_empty", "all_empty", "empty_90pct"]
    finish_and_check(skl, gpu_ctx, [P.pattern(names[s % len(names)], 10, rng) for s in range(4097)])


def against_signs(signs, bins, flags, empty_samples):
    for s in range(signs.shape[0]):
        row, flag_want = Q.expect(signs[s, 0])
        assert flags[s] == flag_want, (s, int(flags[s]), flag_want)
        assert np.array_equal(bins[s], row), s
    assert [s for s in range(signs.shape[0]) if flags[s] & P.EMPTY] == list(empty_samples)


@pytest.mark.parametrize("batches", ["one_batch", "several_batches"])
@pytest.mark.parametrize("num_bins", [10, 1000])
def test_bins_u16_packed_equals_signs_then_oracle(skl, gpu_ctx, set_switch, num_bins, batches):
    codes, cb, offs, ob = dna_inputs()
    packed = skl.pack_codes(codes, cb)
    signs = skl.sketch_signs_packed(gpu_ctx, packed, cb, offs, ob, [17], num_bins, True)
    if batches == "several_batches":
        set_switch("SKL_SKETCH_BATCH_WORDS", 700)
    bins, flags = skl.sketch_bins_u16_packed(gpu_ctx, packed, cb, offs, ob, 17, num_bins, True)
    name = gpu_ctx.last_kernel()
    assert "nthash_binmin" in name and "sketch_finish_kernel" in name and "u16 bins" in name and "targets in LDS" in name and "host" not in name
    against_signs(signs, bins, flags, empty_samples=[5])
    if num_bins == 1000:
        assert (flags[[0, 1]] & P.DENSIFIED).all()           # 2 000 and 3 100 bases leave empty bins among 1 000


def test_host_finish_gives_the_same_bytes(skl, gpu_ctx, set_switch):
    """SKL_SKETCH_FINISH=host on one mixed batch through both calls."""
    rng = np.random.default_rng(1800)
    streams = np.stack([P.pattern(p, 1001, rng) for p in Q.PATTERNS + ["all_empty", "single_middle"]])
    codes, cb, offs, ob = dna_inputs()
    packed = skl.pack_codes(codes, cb)
    device = (skl.sketch_finish_u16(gpu_ctx, streams), skl.sketch_bins_u16_packed(gpu_ctx, packed, cb, offs, ob, 17, 1000, True))
    set_switch("SKL_SKETCH_FINISH", "host")
    host = (skl.sketch_finish_u16(gpu_ctx, streams), skl.sketch_bins_u16_packed(gpu_ctx, packed, cb, offs, ob, 17, 1000, True))
    assert "host" in gpu_ctx.last_kernel() and "sketch_finish_kernel" not in gpu_ctx.last_kernel()
    for d, h in zip(device, host):
        for a, b in zip(d, h):
            assert np.array_equal(a, b)
    for s in range(streams.shape[0]):
        row, flag = Q.expect(streams[s])
        assert np.array_equal(host[0][0][s], row) and host[0][1][s] == flag
