"""csrc/eb_plan.hpp decides the EARLY BREAK of the core/accessory calls -- whether a slab pair gets a decision at all, how its pair
space is cut into blocks and sampled, and what the sampled histograms decide, pooled and block by block -- as pure functions of
plain data.  Here that decision is checked on the CPU: tests/native/eb_plan_check.cpp includes the header alone, is built with the
host compiler (no ROCm include path: the header must not need one) and never loads the library.  The expected values of the pinned
cases are derived by hand from the rules; tests/test_gpu_early_break_r6.py sees the same decisions on sampled data."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "eb_plan_check.cpp")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eb_plan") / "eb_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe])
    return exe


def _run(exe, *args):
    res = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout + res.stderr
    return int(res.stdout.split()[1])


def test_pinned_decisions(check):
    assert _run(check, "pinned") >= 200


def test_decisions_hold_their_properties(check):
    """20 000 seeded histograms: every block counts 2, 3, 4 or all lengths, mixed <=> two live blocks differ, no table unless
    mixed, the self-mode table is symmetric."""
    assert _run(check, "properties", "20000") >= 20000 * 6


def test_the_header_needs_no_device_toolchain():
    text = open(os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "eb_plan.hpp")).read()
    assert "#include <hip" not in text and "hipError_t" not in text and "#ifdef" not in text
