"""csrc/inv_top_plan.hpp on the CPU: the numbers the best-hit selection of `inverted query --top` launches with (digits of
the radix select, padded list length, LDS bytes) and inv_top_select_host(), the host restatement of the kernel's three steps
(csrc/inv_top.hip: threshold by radix select, collect from the high end, bitonic sort), against a plain sort of the keys
(count << 32) | index.  tests/native/inv_top_check.cpp is a program of its own, built with the host compiler under
AddressSanitizer and UBSan and run directly."""
import functools
import os
import subprocess
import tempfile

from conftest import ROOT

_DIR = tempfile.TemporaryDirectory(prefix="inv_top_check_")
FIXED = 1056   # LDS beside the keys and the histogram: the walk's per-wave totals, the scan's, a pass's result


@functools.lru_cache(maxsize=None)
def native():
    exe = os.path.join(_DIR.name, "inv_top_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "sketchlib.rust_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "inv_top_check.cpp"), "-o", exe])
    return exe


def run(*args):
    res = subprocess.run([native(), *map(str, args)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stderr == "", res.stderr          # no sanitizer report
    return res.stdout


def test_constants_and_knob():
    top_max, threads, bits, unforced, forced3, too_wide, negative = map(int, run("consts").split())
    assert (top_max, threads, bits) == (1024, 256, 11)
    assert (unforced, forced3, too_wide, negative) == (11, 3, 11, 11)     # SKL_INVQ_TOP_DIGIT_BITS: 1..11, else the default
    # the public header and the binding state the same limit
    header = open(os.path.join(ROOT, "include", "sketchlib_dist.h")).read()
    assert "#define SKL_INVQ_TOP_MAX 1024\n" in header
    from sketchlib.rust_amd import capi
    assert capi.INVQ_TOP_MAX == top_max


def test_plan_numbers():
    # (S, w, top) -> digits, list length, LDS bytes
    want = {
        (1, 11, 1): (1, 1, 8 + 8192 + FIXED),
        (1, 1, 1): (1, 1, 8 + 8 + FIXED),
        (10, 11, 5): (1, 8, 64 + 8192 + FIXED),
        (10, 3, 64): (2, 64, 512 + 32 + FIXED),
        (1000, 11, 10): (1, 16, 128 + 8192 + FIXED),
        (1000, 8, 700): (2, 1024, 8192 + 1024 + FIXED),
        (1000, 3, 64): (4, 64, 512 + 32 + FIXED),
        (1000, 1, 1): (10, 1, 8 + 8 + FIXED),
        (2047, 11, 1024): (1, 1024, 8192 + 8192 + FIXED),     # the usual sketch sizes: one pass
        (2048, 11, 1024): (2, 1024, 8192 + 8192 + FIXED),
        (5000, 11, 3): (2, 4, 32 + 8192 + FIXED),
        (5000, 1, 2): (13, 2, 16 + 8 + FIXED),
        (65535, 11, 1): (2, 1, 8 + 8192 + FIXED),
        (4294967295, 1, 1): (32, 1, 8 + 8 + FIXED),
    }
    args = [x for key in want for x in key]
    got = {}
    for line in run("plan", *args).splitlines():
        S, w, top, digits, length, lds = map(int, line.split())
        got[(S, w, top)] = (digits, length, lds)
    assert got == want
    # the largest launch stays far below the 64 KiB of dynamic LDS that need no opt-in: 8 workgroups per CU by LDS
    assert max(v[2] for v in got.values()) == 16384 + FIXED


def test_host_selection_equals_a_sort_of_the_keys():
    """n in {1, 63, 64, 255, 256, 257, 700} x S in {1, 10, 1000, 2047, 2048, 5000} x w in {1, 3, 8, 11} x top in
    {1, 2, 64, n, n + 3, 1024}; rows random, all-equal, two-valued and with the threshold at 0."""
    out = run("grid").split()
    assert out[0] == "ok" and int(out[1]) == 7 * 6 * 4 * 6 * 4
