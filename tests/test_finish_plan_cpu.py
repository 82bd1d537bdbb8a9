"""csrc/finish_plan.hpp on the CPU: the launch rules of the finish kernel (sketch_finish.hip) -- form by num_bins, workgroup
shape, probe cap -- and the two-step restatement of densify_bin the kernel runs (a target per bin, then a resolve along the
targets), which the kernel shares with the host through finish_universal_hash / finish_target.  tests/native/
finish_plan_check.cpp compares the two steps with the host sketcher's sequential loop on every pattern and size; the same
program's output is compared with oracle/sketcher.py from here.  Built with the host compiler alone."""
import subprocess

import numpy as np
import pytest

import finish_patterns as P
from oracle import sketcher

LDS_MAX, CAP = 8192, 2048


def run(*args, stdin=None):
    res = subprocess.run([P.native(), *map(str, args)], input=stdin, capture_output=True)
    assert res.returncode == 0, (res.stdout + res.stderr).decode(errors="replace")
    return res.stdout


def test_constants_and_knob():
    lds_max, cap, rounds, forced, unforced = map(int, run("consts").split())
    assert (lds_max, cap) == (LDS_MAX, CAP)
    assert lds_max % 64 == 0 and lds_max * 4 + lds_max // 8 <= 64 * 1024        # targets + emptiness bits: no opt-in for dynamic LDS
    assert 4 * (lds_max * 4 + lds_max // 8) <= 160 * 1024                     # four workgroups of 256 threads per CU
    assert rounds >= 33                                                          # halving a chain of < 2^32 targets
    assert forced == 8 and unforced == cap
    assert 1433 < cap                                                            # the single-bin sketches up to 1 088 bins stay on the device


def test_plan_at_the_lds_bound_and_the_extremes():
    sizes = [64, 128, 192, 256, 1024, 1088, LDS_MAX - 64, LDS_MAX, LDS_MAX + 64, 1 << 20]
    rows = {int(r.split()[0]): list(map(int, r.split()[1:])) for r in run("plan", *sizes).decode().splitlines()}
    for n in sizes:
        lds, threads, lds_bytes, wgs, words = rows[n]
        assert words == n // 64 * 14
        assert threads % 64 == 0
        if n <= LDS_MAX:
            assert lds == 1 and threads == min(n, 256) and lds_bytes == 4 * n + n // 8 and wgs == 5000      # a workgroup per stream
        else:
            assert lds == 0 and threads == 1024 and lds_bytes == 0
            assert 1 <= wgs <= 1024 and wgs * n * 4 <= max(256 << 20, n * 4)     # the target scratch stays within its budget
    assert rows[LDS_MAX + 64][3] == 1024 and rows[1 << 20][3] == 64


@pytest.mark.parametrize("num_bins", [64, 128, 1024, 1088, 4096, 32768])
def test_two_steps_equal_the_sequential_loop(num_bins):
    """Every pattern against skl_host::densify_bin + fill_usigs; the probes a bin needed stay below the cap for every pattern
    but the single non-empty bin of a sketch beyond 1 088 bins."""
    seen = {}
    for line in run("patterns", num_bins).decode().splitlines():
        name, flag, worst = line.split()
        seen[name] = (int(flag), int(worst))
    assert set(seen) == set(P.PATTERNS) | set(P.SINGLES) | {"empty_1pct"}
    assert seen["full"] == (0, 0)
    for name, (flag, worst) in seen.items():
        if name != "full":
            assert flag == P.DENSIFIED
        if name not in P.SINGLES or num_bins <= 1088:
            assert 0 < worst < CAP or name == "full", (name, worst)
    if num_bins >= 4096:
        assert max(seen[s][1] for s in P.SINGLES) > CAP       # what the fall-back is for


@pytest.mark.parametrize("num_bins", [64, 128, 1024, 1088])
def test_two_steps_equal_the_oracle(num_bins):
    rng = np.random.default_rng(num_bins)
    for name in P.PATTERNS + P.SINGLES + ["empty_1pct", "all_empty"]:
        signs = P.pattern(name, num_bins, rng)
        out = run("stream", stdin=signs.tobytes())
        flag = out[0]
        got = np.frombuffer(out[1:], dtype=np.uint64)
        words, first, want_flag = P.expect(sketcher, signs)
        assert flag == want_flag, name
        assert np.array_equal(got[num_bins:], words), name
        if want_flag != P.EMPTY:
            assert got[0] == first, name
            dense = signs.copy()
            sketcher.densify_bin(dense)
            assert np.array_equal(got[:num_bins], dense), name


def test_cap_leaves_a_stream_to_the_fall_back():
    """8 probes: the 99 %-empty stream of 1 024 bins is unfinished and untouched, the 50 %-empty one of 64 bins is not."""
    rng = np.random.default_rng(5)
    assert int(run("capped", 8, stdin=P.pattern("empty_99pct", 1024, rng).tobytes())) & P.UNFINISHED
    assert int(run("capped", 8, stdin=P.pattern("empty_50pct", 64, rng).tobytes())) == P.DENSIFIED
    assert int(run("capped", CAP, stdin=P.pattern("empty_99pct", 1024, rng).tobytes())) == P.DENSIFIED
