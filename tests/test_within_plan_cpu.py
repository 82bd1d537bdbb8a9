"""csrc/within_plan.hpp on the CPU: the numbers the pairs-within-a-cap filter (skl_self_dists_within / skl_cross_dists_within,
csrc/within.hip) launches with, its predicate, the (i, j) of a pair position, and within_select_host(), the host restatement of
the three kernels (count per chunk, scan with a carried total, scatter in position order), against a plain loop over the
array.  tests/native/within_check.cpp is a program of its own, built with the host compiler under AddressSanitizer and UBSan
and run directly."""
import functools
import os
import re
import subprocess
import tempfile

from conftest import ROOT

_DIR = tempfile.TemporaryDirectory(prefix="within_check_")


@functools.lru_cache(maxsize=None)
def native(sanitize=True):
    """The check program; sanitize=False: a plain build, for the GPU tests that only ask it for the plan's constants."""
    exe = os.path.join(_DIR.name, "within_check" if sanitize else "within_check_plain")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", *flags,
                           "-I", os.path.join(ROOT, "sketchlib.rust_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "within_check.cpp"), "-o", exe])
    return exe


def run(*args, sanitize=True):
    res = subprocess.run([native(sanitize), *map(str, args)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stderr == "", res.stderr          # no sanitizer report
    return res.stdout


def consts(sanitize=True):
    """chunk, wave span, scan step, threads, scan threads, band pair limit"""
    return tuple(map(int, run("consts", sanitize=sanitize).split()))


def test_constants_header_and_binding_agree():
    chunk, wave_span, scan_step, threads, scan_threads, limit = consts()
    assert chunk == 4 * wave_span and threads == 256 and scan_step == 4 * scan_threads and limit == 1 << 32
    # a wave's span is whole trips of 64 lanes x one 16-byte load (2 core/accessory pairs or 4 single values)
    assert wave_span % (64 * 4) == 0 and wave_span % (64 * 2) == 0
    from sketchlib.rust_amd import capi
    assert (capi.WITHIN_CHUNK, capi.WITHIN_SCAN_STEP) == (chunk, scan_step)
    # the public header declares the two calls with the argument list the binding passes
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sketchlib_dist.h")).read())
    tail = ("double max_first, double max_second, uint32_t *out_i, uint32_t *out_j, float *out_d, uint64_t capacity, "
            "int out_on_device, uint64_t *n_found);")
    assert "int skl_self_dists_within(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t row_begin, size_t row_end, " + tail in header
    assert ("int skl_cross_dists_within(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query, const skl_dist_params *p, "
            "size_t ref_begin, size_t ref_end, " + tail) in header
    sig = {name: args for name, _res, args in capi._SIG}
    assert len(sig["skl_self_dists_within"]) == 13 and len(sig["skl_cross_dists_within"]) == 14


def test_plan_numbers():
    chunk, _span, step, _t, _st, limit = consts()
    sizes = [0, 1, chunk - 1, chunk, chunk + 1, step * chunk - 1, step * chunk, step * chunk + 1, limit - 1, limit]
    got = {}
    for line in run("plan", *sizes).splitlines():
        m, chunks, steps, scratch, ok, bytes2, bytes1 = map(int, line.split())
        got[m] = (chunks, steps, scratch, ok, bytes2, bytes1)
    for m in sizes:
        chunks = -(-m // chunk)
        steps = -(-chunks // step)
        # the total's 16-byte slot, a u64 offset and a u32 count per chunk; the band rounded up to whole 16-byte loads
        assert got[m] == (chunks, steps, 16 + 12 * chunks, 1 if m < limit else 0, -(-m * 8 // 16) * 16, -(-m * 4 // 16) * 16), m
    assert got[0][:2] == (0, 0) and got[1][:2] == (1, 1) and got[chunk][:2] == (1, 1) and got[chunk + 1][:2] == (2, 1)
    assert got[step * chunk][:2] == (step, 1) and got[step * chunk + 1][:2] == (step + 1, 2)
    assert got[limit - 1][3] == 1 and got[limit][3] == 0          # a band of 2^32 pairs is refused


def test_host_selection_equals_a_plain_loop():
    """Self and cross shapes from one pair to several scan steps' worth of chunks, row ranges that start inside the triangle,
    1 and 2 columns; arrays random, all-pass, none-pass, NaN-bearing, with the cap equal to a stored value, and clustered (most
    chunks empty, a few full); capacities 0, found, found - 1, found + 100, found / 2 with the slots beyond left untouched."""
    out = run("select").split()
    assert out[0] == "ok" and int(out[1]) == 14 * 6 * 3


def test_pair_recovery():
    """(i, j) at position 0, the last position, every row start and end for n in {2, 3, 64, 65, 1000}, steps of up to a wave's
    span from anywhere, positions near 5e11 for n = 1 000 003, and cross rows of 1, 63, 64, 65 and 1 000 003 queries."""
    out = run("locate").split()
    assert out[0] == "ok" and int(out[1]) > 5000
