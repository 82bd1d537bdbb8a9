"""The unit table of csrc/unit_table.hpp: what every workgroup of a k-sliced launch of the chunk-split kernel computes, decoded
once on the host into one 16-byte descriptor per workgroup instead of by every wave at the kernel's head.
tests/native/unit_table_check.cpp builds the table with the header and compares it, workgroup by workgroup and field by field,
with the head of pair_kernel_kslice restated in the check program -- `none` (every early return of the head) included -- as
tests/test_work_map_cpu.py does for the map itself.  Host compiler alone, under AddressSanitizer and UBSan: a descriptor built
from a wrong tile shows as an index past the check's own tile grid."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "unit_table_check.cpp")
GXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unit_table") / "unit_table_check")
    subprocess.check_call(GXX + [SRC, "-o", exe])
    return exe


def _run(exe, mode):
    res = subprocess.run([exe, mode], capture_output=True, text=True)
    last = res.stdout.strip().splitlines()[-1] if res.stdout.strip() else ""
    assert res.returncode == 0 and last.startswith("ok "), res.stdout + res.stderr
    return int(last.split()[1])


def test_table_equals_the_kernels_decode(check):
    """n = 2 ... 700, self mode (all rows, the band [37, n - 50), one row) and cross mode (nA != nB), tile heights 16 / 32, 1 / 2 /
    4 / 8 XCDs, counts and single-k; lengths 1 ... 5, tail slices 0 / 4 / 8, uniform slices 1 / 2, cost order on / off, group spans
    1 ... 3 and the inline prefix go round with n on coprime periods, and meet in full product at n = 2, 17, 65, 129, 193, 257, 413,
    700; a block_ke table with two values (tiles dealt in turns) from n = 257; uneven chunk slices (56 chunks).  Entry b equals
    the decode of workgroup b, none included; every (tile, k index, slice) once, the slices of a (tile, k) partition the sketch,
    every active tile has every k index; cfg 2's table by hand: 2 304 workgroups, 8 of them none."""
    assert _run(check, "table") >= 100_000_000


def test_key_and_cache(check):
    """The same key hits; a key with any one field changed -- 25 launch fields, the tile height, the form, the grid, the block
    table's geometry or one of its values -- misses; four shapes in turn are all kept; a fifth evicts the one unused longest and
    is itself kept; the evicted one is built anew; a failed fill leaves nothing."""
    assert _run(check, "cache") >= 500
