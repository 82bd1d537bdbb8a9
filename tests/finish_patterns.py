"""Streams of bin minima for the tests of the device-side finish (csrc/finish_plan.hpp, csrc/sketch_finish.hip), the
expectation from the oracle's sequential densify_bin + fill_usigs, and the builder of tests/native/finish_plan_check.cpp."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import aa_native
from conftest import ROOT

U64 = np.uint64(0xFFFFFFFFFFFFFFFF)
SIGN_MOD = (1 << 61) - 1
BBITS = 14
DENSIFIED, EMPTY, UNFINISHED = 1, 2, 4
PATTERNS = ["full", "bin0_empty", "last_empty", "first_half_empty", "second_half_empty", "empty_50pct", "empty_99pct"]
SINGLES = ["single_first", "single_middle", "single_last"]

_DIR = tempfile.TemporaryDirectory(prefix="finish_check_")


@functools.lru_cache(maxsize=None)
def native():
    """tests/native/finish_plan_check.cpp with the host sketcher, built once per session with the host compiler alone."""
    exe = os.path.join(_DIR.name, "finish_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", os.path.join(ROOT, "tests", "native", "finish_plan_check.cpp"),
                           *aa_native.HOST_SRC, "-lz", "-lpthread", "-o", exe])
    return exe


def random_signs(rng, n):
    """Signs below 2^61 - 1; some at 2^61 - 2, some with their low 14 bits all zero or all one: keeping 14 bits before the
    resolve, or transposing the wrong plane, shows."""
    v = rng.integers(0, SIGN_MOD, size=n, dtype=np.uint64)
    pick = rng.random(n)
    v[pick < 0.05] = np.uint64(SIGN_MOD - 1)
    lo = (pick >= 0.05) & (pick < 0.10)
    v[lo] &= ~np.uint64((1 << BBITS) - 1)
    hi = (pick >= 0.10) & (pick < 0.15)
    v[hi] |= np.uint64((1 << BBITS) - 1)
    return v


def pattern(name, n, rng):
    v = random_signs(rng, n)
    if name == "full":
        return v
    if name in SINGLES:
        at = {"single_first": 0, "single_middle": n // 2, "single_last": n - 1}[name]
        out = np.full(n, U64, dtype=np.uint64)
        out[at] = v[at]
        return out
    if name == "all_empty":
        return np.full(n, U64, dtype=np.uint64)
    if name == "bin0_empty":
        v[0] = U64
    elif name == "last_empty":
        v[-1] = U64
    elif name == "first_half_empty":
        v[:n // 2] = U64
    elif name == "second_half_empty":
        v[n // 2:] = U64
    elif name.startswith("empty_"):
        frac = int(name[len("empty_"):-len("pct")]) / 100.0
        gone = rng.random(n) < frac
        if gone.all():
            gone[n // 3] = False
        v[gone] = U64
    else:
        raise ValueError(name)
    return v


def expect(sketcher, signs):
    """(words, first sign, flag) of one stream as the oracle's sequential densify_bin and fill_usigs give them."""
    s = np.array(signs, dtype=np.uint64)
    if (s == U64).all():
        return np.zeros(s.size // 64 * BBITS, dtype=np.uint64), U64, EMPTY
    densified = sketcher.densify_bin(s)
    return sketcher.fill_usigs(s), s[0], DENSIFIED if densified else 0
