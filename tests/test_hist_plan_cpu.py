"""csrc/hist_plan.hpp on the CPU: the grid's validation, the cell rule and hist_host(), the sequential restatement of the two
kernels behind skl_self_dists_hist / skl_cross_dists_hist (csrc/hist.hip), against a plain loop over the array.
tests/native/hist_check.cpp is a program of its own, built with the host compiler under AddressSanitizer and UBSan and run
directly."""
import functools
import os
import re
import subprocess
import tempfile

from conftest import ROOT

_DIR = tempfile.TemporaryDirectory(prefix="hist_check_")
CSRC = os.path.join(ROOT, "sketchlib.rust_amd", "csrc")


@functools.lru_cache(maxsize=None)
def native(sanitize=True):
    exe = os.path.join(_DIR.name, "hist_check" + ("" if sanitize else "_plain"))
    flags = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-ffp-contract=off", *flags,
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "hist_check.cpp"), "-o", exe])
    return exe


def run(*args, sanitize=True):
    res = subprocess.run([native(sanitize), *map(str, args)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stderr == "", res.stderr          # no sanitizer report
    return res.stdout


def consts(sanitize=True):
    """(threads, chunk, LDS cells, cell limit, LDS workgroups, global workgroups, scratch head bytes, peel rounds)"""
    return tuple(map(int, run("consts", sanitize=sanitize).split()))


def test_constants_header_and_binding_agree():
    threads, chunk, lds_cells, max_cells, lds_groups, global_groups, head, peel = consts()
    assert threads % 64 == 0 and chunk % (threads * 4) == 0
    assert lds_cells * 4 * 2 <= 160 * 1024                    # two workgroups' private histograms in a CU's LDS
    assert lds_cells == 128 * 128 and max_cells == 1 << 20 and lds_cells < max_cells
    assert 0 < lds_groups <= global_groups and head == 16 and 1 <= peel <= 8
    from sketchlib.rust_amd import capi
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sketchlib_dist.h")).read())
    assert ("int skl_self_dists_hist(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t row_begin, size_t row_end, "
            "const skl_hist_grid *grid, uint64_t *counts, int counts_on_device, int flags, uint64_t *outside);") in header
    assert ("int skl_cross_dists_hist(skl_ctx *ctx, const skl_sketches *ref, const skl_sketches *query, const skl_dist_params *p, "
            "size_t ref_begin, size_t ref_end, const skl_hist_grid *grid, uint64_t *counts, int counts_on_device, int flags, uint64_t *outside);") in header
    assert re.search(r"#define SKL_HIST_ACCUMULATE 1\b", header) and capi.HIST_ACCUMULATE == 1
    assert re.search(r"#define SKL_ABI_VERSION 1\b", header)
    # the struct as the header lays it out: four doubles, two u32
    body = re.search(r"typedef struct skl_hist_grid \{(.*?)\} skl_hist_grid;", header).group(1)
    fields = re.findall(r"(double|uint32_t) ([^;]*);", body)
    assert [(t, [n.strip() for n in names.split(",")]) for t, names in fields] == [("double", ["lo0", "hi0"]), ("double", ["lo1", "hi1"]), ("uint32_t", ["n0", "n1"])]
    import ctypes as C
    assert [(n, t) for n, t in capi.HistGrid._fields_] == [("lo0", C.c_double), ("hi0", C.c_double), ("lo1", C.c_double), ("hi1", C.c_double),
                                                           ("n0", C.c_uint32), ("n1", C.c_uint32)]
    assert C.sizeof(capi.HistGrid) == 40
    sig = {name: (res, args) for name, res, args in capi._SIG}
    P = C.c_void_p
    assert sig["skl_self_dists_hist"] == (C.c_int, [P, P, C.POINTER(capi.DistParams), C.c_size_t, C.c_size_t, C.POINTER(capi.HistGrid), P, C.c_int, C.c_int, P])
    assert sig["skl_cross_dists_hist"] == (C.c_int, [P, P, P, C.POINTER(capi.DistParams), C.c_size_t, C.c_size_t, C.POINTER(capi.HistGrid), P, C.c_int,
                                                     C.c_int, P])
    assert callable(capi.dists_hist)


def test_the_plan_is_pure_and_built():
    """hist_plan.hpp has no HIP header and does not read the environment; the kernels and the driver are in the build, and
    within.hip / cluster.hip still take their loads from within_wave.hpp, which hist.hip leaves alone."""
    plan = open(os.path.join(CSRC, "hist_plan.hpp")).read()
    assert "hip/" not in plan and "getenv" not in plan
    make = open(os.path.join(CSRC, "Makefile")).read()
    dev_hdr = re.search(r"^DEV_HDR := (.*)$", make, flags=re.M).group(1).split()
    assert "hist_plan.hpp" in dev_hdr
    assert "$(OUT)/hist.o" in make and "$(OUT)/capi_hist.o" in make
    hist = open(os.path.join(CSRC, "hist.hip")).read()
    assert "hist_lds_kernel" in hist and "hist_global_kernel" in hist and "asm" not in hist        # plain HIP C++
    assert '#include "within_wave.hpp"' not in hist


def test_grid_refusals():
    """n0 == 0; n1 == 0 with two columns; a NaN or infinite bound in either column, as given or once rounded to float; hi <= lo as
    given and after rounding to float; a scale that is no finite float; more than 2^20 cells, in one column, in two, and as a
    product that would wrap; a refused grid leaves the output untouched.  Accepted: 1 024 x 1 024, 2^20 x 1, the two grids at
    the LDS boundary, and garbage in the second column's fields with one column."""
    out = run("grid").split()
    assert out[0] == "ok" and int(out[1]) >= 30


def test_cell_rule():
    """Eight axes, as the first column, as the only column and as the second: lo gives cell 0, hi the last cell, nextafter beyond
    either end is outside and inside either end is inside, +-inf is outside, NaN is NaN, and a sweep of 1e5 values is monotone
    from cell 0 to the last.  Two columns: the index is c0 * n1 + c1, a NaN in either column wins over off-grid in the other."""
    out = run("cell").split()
    assert out[0] == "ok" and int(out[1]) >= 8 * 3 + 6


def test_host_histogram_equals_a_plain_loop():
    """1 and 2 columns x six grids (1 x 1, 8 x 8, the narrow one, exactly HIST_LDS_CELLS, one column more, HIST_MAX_CELLS) x the
    lengths {0, 1, 2, chunk - 1, chunk, chunk + 1, 3 chunks + 7} x four fills (random values beyond both ends, all one cell, the
    grid's own ends, NaNs and infinities): identical counts, outside and nan; sum + outside + nan == m every time; nothing behind
    the counts is written; a second band is added."""
    out = run("host").split()
    assert out[0] == "ok" and int(out[1]) == 2 * 6 * 7 * 4
