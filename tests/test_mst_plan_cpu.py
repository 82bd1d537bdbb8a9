"""csrc/mst_plan.hpp on the CPU: mst_forest_host(), the sequential restatement of a whole skl_self_mst call (csrc/mst.hip: the
min-edge kernel over the triangle, the two per-sample offers, the append, the hook, flatten and count, round after round),
against a plain Kruskal over the edges sorted by (w, i, j); the key map; and skl_clusters_from_edges' host form on prefixes of a
tree.  tests/native/mst_check.cpp is a program of its own, built with the host compiler under AddressSanitizer and UBSan and run
directly."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

from conftest import ROOT

_DIR = tempfile.TemporaryDirectory(prefix="mst_check_")
CSRC = os.path.join(ROOT, "sketchlib.rust_amd", "csrc")


@functools.lru_cache(maxsize=None)
def native():
    exe = os.path.join(_DIR.name, "mst_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "mst_check.cpp"), "-o", exe])
    return exe


def run(*args):
    res = subprocess.run([native(), *map(str, args)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stderr == "", res.stderr          # no sanitizer report
    return res.stdout


def test_constants_header_and_binding_agree():
    empty_is_all_ones, max_rounds, head, labels, best, comp_min, comp_hi, rec_i, rec_j, rec_w, total, fill_at, fill_bytes = map(int, run("consts").split())
    assert empty_is_all_ones == 1 and max_rounds == 32 and head == 16
    # n = 1000: every array on a 16-byte boundary, in the order the header comment gives, none overlapping the next
    assert (labels, best, comp_min, comp_hi, rec_i, rec_j, rec_w, total) == (16, 4016, 12016, 20016, 24016, 28016, 32016, 36016)
    assert all(x % 16 == 0 for x in (labels, best, comp_min, comp_hi, rec_i, rec_j, rec_w, total))
    assert (fill_at, fill_at + fill_bytes) == (best, rec_i)                # one fill empties best, comp_min and comp_hi
    from sketchlib.rust_amd import capi
    # the public header declares the two calls with the argument lists the binding passes
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sketchlib_dist.h")).read())
    assert ("int skl_self_mst(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, int column, double max_dist, "
            "uint32_t *out_i, uint32_t *out_j, float *out_w, uint32_t *labels, uint64_t *n_edges, uint32_t *rounds);") in header
    assert ("int skl_clusters_from_edges(skl_ctx *ctx, const uint32_t *edge_i, const uint32_t *edge_j, uint64_t n_edges_in, "
            "uint64_t n, uint32_t *labels, uint64_t *n_clusters);") in header
    sig = {name: (res, args) for name, res, args in capi._SIG}
    P = C.c_void_p
    assert sig["skl_self_mst"] == (C.c_int, [P, P, C.POINTER(capi.DistParams), C.c_int, C.c_double, P, P, P, P, C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_uint32)])
    assert sig["skl_clusters_from_edges"] == (C.c_int, [P, P, P, C.c_uint64, C.c_uint64, P, C.POINTER(C.c_uint64)])
    for fn in ("mst", "clusters_from_edges"):
        assert callable(getattr(capi, fn))


def test_the_plan_is_pure_and_the_union_header_is_shared():
    """mst_plan.hpp has no HIP header and does not read the environment; cluster.hip and mst.hip take the union-find's device
    functions from one header instead of two copies, and mst.hip reads a band through within_wave.hpp like the others."""
    plan = open(os.path.join(CSRC, "mst_plan.hpp")).read()
    assert "hip/" not in plan and "getenv" not in plan
    union = open(os.path.join(CSRC, "cluster_union.hpp")).read()
    for fn in ("uint32_t cluster_find(", "void cluster_union(", "void cluster_shorten("):
        assert union.count(fn) == 1, fn
    for f in ("cluster.hip", "mst.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "cluster_union.hpp"' in text and '#include "within_wave.hpp"' in text, f
        assert "void cluster_union(" not in text and "uint32_t cluster_find(" not in text and "struct WithinWave" not in text, f
        assert "cluster_union(" in text, f                                  # ... and both call it
    make = open(os.path.join(CSRC, "Makefile")).read()
    dev_hdr = re.search(r"^DEV_HDR := (.*)$", make, flags=re.M).group(1).split()
    assert {"mst_plan.hpp", "cluster_union.hpp", "within_wave.hpp", "cluster_plan.hpp"} <= set(dev_hdr)
    assert "$(OUT)/mst.o" in make and "$(OUT)/capi_mst.o" in make


def test_key_map():
    """mst_key orders like the float comparison on a table of edge values and 100 000 random bit patterns, -0.0f and +0.0f share
    a key, the way back returns the value (+0.0f for both zeros), no offer reaches the empty word; the cap rules; the predicate
    reads the chosen column alone."""
    out = run("keys").split()
    assert out[0] == "ok" and int(out[1]) >= 90000


def test_host_forest_equals_kruskal():
    """n in {0, 1, 2, 3, 65, 300, 2100} x (one column; two columns, column 0 and 1; the other column holds noise and NaNs):
    random weights without a cap, with a cap that leaves a forest and with a cap equal to a weight; a cap below every weight;
    three distinct values, also capped at the middle one; all equal (the star at 0, in one round); -0.0f among +0.0f, alone and
    among other values, also capped at 0; NaNs scattered, in whole rows and diagonals, everywhere; the path whose weights are
    the ruler sequence, which takes floor(log2 n) rounds.  Each: the edge list identical to Kruskal's and strictly ascending,
    labels identical, n_edges + components == n, rounds <= ceil(log2 n), nothing written beyond n_edges or n."""
    out = run("forest").split()
    assert out[0] == "ok" and int(out[1]) == 7 * 3 * 16


def test_host_clusters_from_edges():
    """The prefix w <= t of a tree gives the components of ALL pairs within t, for six thresholds at four sizes; an index equal
    to n on either side is refused with labels and the count untouched."""
    out = run("edges").split()
    assert out[0] == "ok" and int(out[1]) == 4 * 7
