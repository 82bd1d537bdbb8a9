"""csrc/host/multi_plan.hpp decides how the C++ host layer shares one call among several devices -- row shards, the column
windows and dealt bands of the one-evaluation kNN, which kNN form runs first and which follows when it gives up, the sizes they
move -- as pure functions of plain values.  Here that is checked on the CPU: tests/native/multi_plan_check.cpp includes the header
alone, is built with the host compiler (once plain, once under AddressSanitizer and UndefinedBehaviorSanitizer) and never loads the
library.  The pinned values are derived by hand; the partitions are also held against multi_gpu.py, which states them for the
Python drivers, over one grid."""
import functools
import math
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT
from sketchlib.rust_amd import multi_gpu

SRC = os.path.join(ROOT, "tests", "native", "multi_plan_check.cpp")
GRID_N = list(range(2, 300)) + [1000, 2829, 16000, 100003]
GRID_W = range(1, 9)
GRID_BAND_ROWS = (1, 2, 3, 16, 64, 100, 256, 1024)
_DIR = tempfile.TemporaryDirectory(prefix="multi_plan_check_")


@functools.lru_cache(maxsize=None)
def _build(kind):
    exe = os.path.join(_DIR.name, f"multi_plan_check_{kind}")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if kind == "sanitized" else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def check(request):
    return _build(request.param)


def _run(exe, *args):
    res = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout + res.stderr
    return int(res.stdout.split()[1])


def test_pinned_cuts_deal_sizes_and_form_order(check):
    assert _run(check, "pinned") >= 45


def test_partitions_hold_their_properties(check):
    assert _run(check, "grid") >= len(GRID_N) * len(GRID_W) * (4 * len(GRID_BAND_ROWS) + 2)


def _cut_rules_may_differ(n, band_rows, world):
    """Where multi_plan.hpp says its cuts differ from multi_gpu.knn_window_cuts: a quotient with fractional part exactly 0.5
    (away from zero there, to even here), or a cut that rounds past the last band boundary at or below n (clamped to n there, to
    that boundary here)."""
    last = n // band_rows * band_rows
    for r in range(1, world):
        q = n * math.sqrt(r / world) / band_rows
        frac = q - math.floor(q)
        if frac == 0.5 or (math.floor(q) + (frac >= 0.5)) * band_rows > last:
            return True
    return False


def test_partitions_equal_the_python_drivers():
    out = subprocess.run([_build("plain"), "print"], capture_output=True, text=True, check=True).stdout
    cuts, self_b, even_b, deal = {}, {}, {}, {}
    for line in out.splitlines():
        kind, *v = line.split()
        v = [int(x) for x in v]
        if kind == "C":
            cuts[tuple(v[:3])] = v[3:]
        elif kind == "D":
            deal[tuple(v[:3])] = v[3:]
        else:
            (self_b if kind == "S" else even_b)[tuple(v[:2])] = v[2:]
    grid = [(n, b, w) for n in GRID_N for w in GRID_W for b in GRID_BAND_ROWS]
    assert sorted(cuts) == sorted(grid)
    excluded = 0
    for n, band_rows, world in grid:
        if _cut_rules_may_differ(n, band_rows, world):
            excluded += 1
        else:
            assert cuts[n, band_rows, world] == multi_gpu.knn_window_cuts(n, band_rows, world), (n, band_rows, world)
    assert excluded <= 0.15 * len(grid), excluded     # (2 465 of 19 328)
    for n in GRID_N:
        for world in GRID_W:
            assert self_b[n, world] == multi_gpu.self_row_bounds(n, world), (n, world)
            assert even_b[n, world] == multi_gpu.even_row_bounds(n, world), (n, world)
    bands = sorted({((n + b - 1) // b, w) for n, b, w in grid})
    assert sorted({k[:2] for k in deal}) == bands
    for n_bands, world in bands:
        want = multi_gpu.knn_band_deal(n_bands, world)
        for d in range(world):
            assert deal[n_bands, world, d] == want[d], (n_bands, world, d)
