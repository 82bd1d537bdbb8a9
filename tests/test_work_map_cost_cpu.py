"""The cost order of csrc/work_map.hpp: in self mode a tile that walks one of its two 64-column blocks costs half, so the
active tiles are numbered in two classes and every XCD takes a share of each, its full tiles first and its half tiles last.
tests/native/work_map_cost_check.cpp runs the plan against the decode on the CPU, as tests/test_work_map_cpu.py does for the
present order (which stays the order of every other launch and is checked here slot for slot against its restatement).  The
program is built with the host compiler alone, under AddressSanitizer and UBSan: a wrong run of the half numbering shows as an
index past the tile grid."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "work_map_cost_check.cpp")
GXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("work_map_cost") / "work_map_cost_check")
    subprocess.check_call(GXX + [SRC, "-o", exe])
    return exe


def _run(exe, mode):
    res = subprocess.run([exe, mode], capture_output=True, text=True)
    last = res.stdout.strip().splitlines()[-1] if res.stdout.strip() else ""
    assert res.returncode == 0 and last.startswith("ok "), res.stdout + res.stderr
    return int(last.split()[1])


def test_pinned_cases(check):
    """The 1 000-genome launch by hand: 256 full and 31 half tiles, 32 + 3 or 4 per XCD, 36 slots."""
    assert _run(check, "pinned") >= 25


def test_cost_order_over_every_shape(check):
    """n = 2 ... 700 x six row bands x tile heights 16 / 32 x 1 / 2 / 4 / 8 XCDs x group spans 1 ... 4: every active tile at exactly
    one (XCD, slot) and forward o inverse the identity; every owed pair in exactly one tile; the classes are the kernel's skip
    tests and say which tiles hold a pair in both blocks; full before half on every XCD; per-class counts within one and the
    heaviest XCD within one full tile of the mean; the grid is the largest share << xcd_shift; with tail slices 2 / 4 / 8 and
    2 ... 5 lengths every (tile, k, slice) once; with the order off, the present numbering slot for slot."""
    assert _run(check, "order") >= 40_000_000


def test_which_launches_take_the_order(check):
    """plan_pair_shape(): cfg 2's counts launch takes the order; the interleaved order, one XCD, cross mode, single-k keys, no half
    tiles, SKL_TILE_COST_ORDER=0, a launch past the size bound and 32-row tiles do not; =1 lifts the size bound alone."""
    assert _run(check, "rule") >= 11
