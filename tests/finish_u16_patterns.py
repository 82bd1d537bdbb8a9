"""Shared by the tests of the u16 finish (csrc/finish_plan.hpp finish_*_u16, csrc/sketch_finish.hip): the builder of
tests/native/finish_u16_check.cpp and the expectation of one stream from the oracle's sequential densify_bin, cut to 16 bits."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import aa_native
import finish_patterns as P
from conftest import ROOT

_DIR = tempfile.TemporaryDirectory(prefix="finish_u16_check_")
# the issue's patterns: full, bin 0 empty, last empty, either half empty, 50 % and 90 % empty
PATTERNS = ["full", "bin0_empty", "last_empty", "first_half_empty", "second_half_empty", "empty_50pct", "empty_90pct"]


@functools.lru_cache(maxsize=None)
def native():
    exe = os.path.join(_DIR.name, "finish_u16_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", os.path.join(ROOT, "tests", "native", "finish_u16_check.cpp"),
                           *aa_native.HOST_SRC, "-lz", "-lpthread", "-o", exe])
    return exe


def is_all_empty(signs):
    return bool((np.asarray(signs) == P.U64).all())


@functools.lru_cache(maxsize=None)
def _expect_cached(key):
    s = np.frombuffer(key, dtype=np.uint64).copy()
    if is_all_empty(s):
        return np.zeros(s.size, dtype=np.uint16).tobytes(), P.EMPTY
    filled = s[s != P.U64]
    if filled.size == 1:
        # a single non-empty bin: densify_bin's loop for an empty bin ends only on a bin that holds a value, and this is the
        # only one, so every bin takes its sign (the oracle's Python loop would take ~num_bins probes per bin)
        return np.full(s.size, filled[0], dtype=np.uint64).astype(np.uint16).tobytes(), P.DENSIFIED if s.size > 1 else 0
    from oracle import sketcher
    densified = sketcher.densify_bin(s)
    return (s & np.uint64(0xFFFF)).astype(np.uint16).tobytes(), P.DENSIFIED if densified else 0


def expect(signs):
    """(u16 row, flag) of one stream: oracle/sketcher.py's sequential densify_bin, then & 0xFFFF.  Computed once per stream."""
    row, flag = _expect_cached(np.ascontiguousarray(signs, dtype=np.uint64).tobytes())
    return np.frombuffer(row, dtype=np.uint16), flag
