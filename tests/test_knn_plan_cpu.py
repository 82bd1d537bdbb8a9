"""csrc/knn_plan.hpp decides HOW the kNN drivers cut and feed their bands -- band heights, symmetric or row by row, column panels,
each band's view of the columns, the sizes of the scratch buffers, what a band is eligible for and its two merges in the order
of the tie mode -- as pure functions of plain data.  Here that decision is checked on the CPU: tests/native/knn_plan_check.cpp
includes the header alone, is built with the host compiler (no ROCm include path: the header must not need one) and never loads
the library.  The pinned heights and panels are derived by hand from the rules; coverage, arrival order and buffer sizes are
exact properties over seeded calls of all three forms.  The GPU kNN suites check the same drivers against the oracle."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "knn_plan_check.cpp")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("knn_plan") / "knn_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe])
    return exe


def _run(exe, *args):
    res = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout + res.stderr
    return int(res.stdout.split()[1])


def test_pinned_heights_and_panels(check):
    assert _run(check, "pinned") >= 60


def test_every_pair_once_ascending_within_the_buffers(check):
    # per case: three forms, each with "once" and "ascending" and the per-band buffer checks
    assert _run(check, "coverage", "1500") >= 1500 * 6


def test_shared_band_rows_agree_with_the_symmetric_height(check):
    assert _run(check, "agreement", "20000") >= 20000
