"""csrc/eb_stripes.hpp says which workgroup of the early-break epilogue's STRIPED order holds which pairs: the launch's columns in
2 X stripes, XCD x owns stripes x and 2 X - 1 - x, a workgroup = two rows against one 64-column block of each.  Here the host's
grid and the kernel's decode are run against each other on the CPU, and the rule that picks the order (dense_plan.hpp
counts_striped) against cases derived by hand: tests/native/eb_stripes_check.cpp includes the two headers alone, is built with
the host compiler (no ROCm include path: the headers must not need one) and never loads the library.
tests/test_gpu_epilogue_stripes.py runs the kernel in this order against the oracle."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "eb_stripes_check.cpp")
HEADER = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "eb_stripes.hpp")
GXX = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eb_stripes") / "eb_stripes_check")
    subprocess.check_call(GXX + [SRC, "-o", exe])
    return exe


def _run(exe, mode):
    res = subprocess.run([exe, mode], capture_output=True, text=True)
    last = res.stdout.strip().splitlines()[-1] if res.stdout.strip() else ""
    assert res.returncode == 0 and last.startswith("ok "), res.stdout + res.stderr
    return int(last.split()[1])


def test_every_pair_in_exactly_one_thread(check):
    """Self mode with 2 ... 300 and 1 000 columns -- every row band up to n = 40, a seeded sample of bands above -- and cross shapes
    up to 70 x 300, on 1, 2, 4 and 8 XCDs: every pair of the launch is owned by exactly one (workgroup, thread), at its own index
    of the launch's counts and output; a workgroup touches columns of its XCD's two stripes only; a wave's pairs are consecutive; a
    workgroup leaves exactly when it holds no pair; the grid is what the forward side says and nothing lies past it."""
    assert _run(check, "map") >= 50_000_000


def test_the_fold_balances_the_triangle(check):
    """n = 1 000 on 8 XCDs: XCD 0 holds 41 196 pairs, every other one 65 472; the heaviest is within 1.05 x the mean (1.049)."""
    assert _run(check, "balance") >= 15


def test_the_rule(check):
    """cfg 2 at a sampled share of 0.048 takes the stripes; at 0.011, in the blocked order and under a mixed plan it does not; the
    bound on the slices' bytes and the bound on the heaviest XCD's share (n = 1 500: 1.86 x the mean, not taken), also for a
    row band; the knob; the launches the lean kernel does not take."""
    assert _run(check, "rule") >= 60


def test_the_header_needs_no_device_toolchain(tmp_path):
    text = open(HEADER).read()
    assert "#include <hip" not in text and "hipError_t" not in text
    tu = tmp_path / "alone.cpp"
    tu.write_text('#include "%s"\nint main() { return skl::eb_stripe_width(1000, 3) == 64 ? 0 : 1; }\n' % HEADER)
    subprocess.check_call(GXX + [str(tu), "-o", str(tmp_path / "alone")])
