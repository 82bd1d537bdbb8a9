"""The u16 finish on the CPU (csrc/finish_plan.hpp): the launch rules for ragged bin counts -- whole-wave workgroups, the LDS
bytes, the old values at multiples of 64 -- and finish_stream_host_u16 (densify by the two steps, then `sign as u16`) against
the host sketcher's sequential densify_bin (inside tests/native/finish_u16_check.cpp) and against oracle/sketcher.py.  Built
with the host compiler alone."""
import subprocess

import numpy as np
import pytest

import finish_patterns as P
import finish_u16_patterns as Q

LDS_MAX = 8192
SIZES = [1, 2, 10, 63, 64, 65, 1000, 1001, 8192, 8193, 1 << 20]


def run(*args, stdin=None):
    res = subprocess.run([Q.native(), *map(str, args)], input=stdin, capture_output=True)
    assert res.returncode == 0, (args, (res.stdout[:200] + res.stderr).decode(errors="replace"))
    return res.stdout


def test_plan_rules_for_ragged_bin_counts():
    rows = {int(r.split()[0]): list(map(int, r.split()[1:])) for r in run("plan", *SIZES).decode().splitlines()}
    assert set(rows) == set(SIZES)
    for n in SIZES:
        lds, threads, lds_bytes, old_threads, old_lds_bytes, wgs = rows[n]
        assert threads % 64 == 0 and threads >= 64, (n, threads)          # whole waves: n_waves = threads >> 6 is never 0
        if n <= LDS_MAX:
            assert lds == 1 and threads == min((n + 63) // 64 * 64, 256), (n, threads)
            assert lds_bytes == 4 * n + 4 * ((n + 31) // 32), (n, lds_bytes)
            assert lds_bytes <= 64 * 1024 and wgs == 5000
        else:
            assert lds == 0 and threads == 1024 and lds_bytes == 0, (n, threads, lds_bytes)
        if n % 64 == 0:                                                    # the values tests/test_finish_plan_cpu.py pins do not move
            assert (threads, lds_bytes) == (old_threads, old_lds_bytes), n
            if n <= LDS_MAX:
                assert threads == min(n, 256) and lds_bytes == 4 * n + n // 8
    assert rows[10][2 + 1] == 10        # what the plane rule gives at 10 bins: fewer threads than a wave, why the u16 form has its own


@pytest.mark.parametrize("num_bins", [n for n in SIZES if n <= 8193])
def test_host_form_equals_the_sequential_loop_and_the_oracle(num_bins):
    rng = np.random.default_rng(7000 + num_bins)
    done = 0
    for name in P.PATTERNS + P.SINGLES + ["empty_90pct", "all_empty"]:
        signs = P.pattern(name, num_bins, rng)
        if name != "all_empty" and Q.is_all_empty(signs):
            continue                                                       # the same stream as all_empty at this size
        out = run("stream", stdin=signs.tobytes())                         # (exit 1: differs from skl_host::densify_bin)
        row, flag = Q.expect(signs)
        assert out[0] == flag, (name, out[0], flag)
        assert np.array_equal(np.frombuffer(out[1:], dtype=np.uint16), row), name
        done += 1
    assert done >= (3 if num_bins == 1 else 8)


def test_low_16_bits_all_one_is_a_value_and_all_empty_is_flagged():
    """A sign whose low 16 bits are 0xFFFF is filled FROM; u64::MAX alone is empty.  An all-empty stream: zero row, the flag."""
    signs = np.array([P.U64, 0x1234_0000_FFFF, P.U64, 0x0FFF_FFFF_FFFF_FFFF, P.U64], dtype=np.uint64)
    out = run("stream", stdin=signs.tobytes())
    row = np.frombuffer(out[1:], dtype=np.uint16)
    assert out[0] == P.DENSIFIED and (row == 0xFFFF).all()
    want, flag = Q.expect(signs)
    assert flag == P.DENSIFIED and np.array_equal(row, want)
    out = run("stream", stdin=np.full(10, P.U64, dtype=np.uint64).tobytes())
    assert out[0] == P.EMPTY and not np.frombuffer(out[1:], dtype=np.uint16).any()
