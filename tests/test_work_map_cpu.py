"""csrc/work_map.hpp says which workgroup of a pair-kernel launch computes what: the host's plan (tiles per column group, the
super-group prefix, the share of each XCD, the chunk-split kernel's units, slices and grid size) and the kernels' decode of their
workgroup index, as plain functions of the launch's fields.  Here the two sides are run against each other on the CPU:
tests/native/work_map_check.cpp includes the header alone, is built with the host compiler (no ROCm include path: the header must
not need one) and never loads the library.  The GPU parity suites see the same map at the shapes they happen to run."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "work_map_check.cpp")
HEADER = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "work_map.hpp")
GXX = ["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("work_map") / "work_map_check")
    subprocess.check_call(GXX + [SRC, "-o", exe])
    return exe


def _run(exe, mode):
    res = subprocess.run([exe, mode], capture_output=True, text=True)
    last = res.stdout.strip().splitlines()[-1] if res.stdout.strip() else ""
    assert res.returncode == 0 and last.startswith("ok "), res.stdout + res.stderr
    return int(last.split()[1]), res.stdout


def test_pinned_cases(check):
    assert _run(check, "pinned")[0] >= 150


def test_every_tile_once_and_every_owed_pair_in_one(check):
    """Three tile shapes x 15 sizes x up to six row bands x self / cross x group spans 1-4 x 1-8 XCDs x contiguous / interleaved x the
    prefix table inline / searched: the slots of the planned grid yield n_active_tiles distinct tiles that hold every owed pair, a
    tile without one lies past the launch's last column, none of the kernels' defensive returns fires, the grid is
    tiles_per_xcd << xcd_shift."""
    checks, out = _run(check, "tiles")
    assert checks >= 3_000_000
    assert "tiles without an owed pair" in out


def test_every_unit_once_and_its_slices_partition_the_sketch(check):
    """The chunk-split grid over 9 tile maps x 1-6 lengths x 6 sketch sizes x uniform and tail slices x the three kernel forms: every
    workgroup index below n_wg is one (tile slot, k index, slice), none is "no unit", whole units once, sliced ones once per
    slice, the slices of a unit partition [0, ss64) in whole stages."""
    assert _run(check, "units")[0] >= 20_000_000


def test_the_header_needs_no_device_toolchain(tmp_path):
    text = open(HEADER).read()
    assert "#include <hip" not in text and "hipError_t" not in text
    tu = tmp_path / "alone.cpp"
    tu.write_text('#include "%s"\nint main() { return skl::KSL_TILE_BLOCK == 32 ? 0 : 1; }\n' % HEADER)
    subprocess.check_call(GXX + [str(tu), "-o", str(tmp_path / "alone")])
