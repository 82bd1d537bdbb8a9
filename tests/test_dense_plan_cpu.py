"""csrc/dense_plan.hpp decides HOW a dense distance call is launched -- fused kernel or counts + epilogue, the counts' record
width, chunk slices and planes, the epilogue's order, the row bands and whether they overlap, each pair-kernel launch's tile shape
and name, the bands of a host-destined call -- as pure functions of plain data.
Here that decision is checked on the CPU: tests/native/dense_plan_check.cpp includes the header alone, is built with the host
compiler (no ROCm include path: the header must not need one) and never loads the library.  The expected values of the pinned
regimes are derived by hand from the rules; the GPU suites assert the same decisions through the kernel names they produce."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "dense_plan_check.cpp")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dense_plan") / "dense_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe])
    return exe


def _run(exe, *args):
    res = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout + res.stderr
    return int(res.stdout.split()[1])


def test_pinned_regimes(check):
    assert _run(check, "pinned") >= 140


def test_band_cuts_hold_their_properties(check):
    assert _run(check, "bands", "4000") >= 4000 * 8


def test_planes_and_bytes_are_consistent(check):
    assert _run(check, "consistency", "20000") >= 20000


def test_pair_kernel_shapes_and_names(check):
    assert _run(check, "shape") >= 70


def test_host_bands_hold_their_properties(check):
    assert _run(check, "hostbands", "4000") >= 4000 * 8
