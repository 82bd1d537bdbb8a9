"""csrc/cluster_plan.hpp on the CPU: cluster_labels_host(), the sequential restatement of the kernels behind
skl_self_clusters_within (csrc/cluster.hip: union of the passing pairs of a band, flatten, count), the label check and the merge
of skl_clusters_merge, against a brute-force component search.  tests/native/cluster_check.cpp is a program of its own, built
with the host compiler under AddressSanitizer and UBSan and run directly."""
import functools
import os
import re
import subprocess
import tempfile

from conftest import ROOT

_DIR = tempfile.TemporaryDirectory(prefix="cluster_check_")
CSRC = os.path.join(ROOT, "sketchlib.rust_amd", "csrc")


@functools.lru_cache(maxsize=None)
def native():
    exe = os.path.join(_DIR.name, "cluster_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "native", "cluster_check.cpp"), "-o", exe])
    return exe


def run(*args):
    res = subprocess.run([native(), *map(str, args)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stderr == "", res.stderr          # no sanitizer report
    return res.stdout


def test_constants_header_and_binding_agree():
    threads, head, limit = map(int, run("consts").split())
    assert threads % 64 == 0 and head == 16 and limit == (1 << 32) - 1
    from sketchlib.rust_amd import capi
    # the public header declares the two calls with the argument lists the binding passes
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sketchlib_dist.h")).read())
    assert ("int skl_self_clusters_within(skl_ctx *ctx, const skl_sketches *s, const skl_dist_params *p, size_t row_begin, size_t row_end, "
            "double max_first, double max_second, uint32_t *labels, int labels_on_device, int flags, uint64_t *n_clusters);") in header
    assert "int skl_clusters_merge(skl_ctx *ctx, uint32_t *labels, const uint32_t *other, uint64_t n, int on_device, uint64_t *n_clusters);" in header
    assert re.search(r"#define SKL_CLUSTERS_CONTINUE 1\b", header) and capi.CLUSTERS_CONTINUE == 1
    sig = {name: (res, args) for name, res, args in capi._SIG}
    import ctypes as C
    P = C.c_void_p
    assert sig["skl_self_clusters_within"] == (C.c_int, [P, P, C.POINTER(capi.DistParams), C.c_size_t, C.c_size_t, C.c_double, C.c_double, P, C.c_int,
                                                         C.c_int, C.POINTER(C.c_uint64)])
    assert sig["skl_clusters_merge"] == (C.c_int, [P, P, P, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)])
    for fn in ("clusters_within", "clusters_merge", "dereplicate"):
        assert callable(getattr(capi, fn))


def test_the_plan_is_pure_and_the_wave_header_is_shared():
    """cluster_plan.hpp has no HIP header and does not read the environment; within.hip and cluster.hip take a wave's loads and
    ballots from one header instead of two copies."""
    plan = open(os.path.join(CSRC, "cluster_plan.hpp")).read()
    assert "hip/" not in plan and "getenv" not in plan
    wave = open(os.path.join(CSRC, "within_wave.hpp")).read()
    assert "struct WithinWave" in wave and "within_lanes_below" in wave
    for f in ("within.hip", "cluster.hip"):
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "within_wave.hpp"' in text and "struct WithinWave" not in text, f
    make = open(os.path.join(CSRC, "Makefile")).read()
    dev_hdr = re.search(r"^DEV_HDR := (.*)$", make, flags=re.M).group(1).split()
    assert {"within_wave.hpp", "cluster_plan.hpp"} <= set(dev_hdr)
    assert "$(OUT)/cluster.o" in make and "$(OUT)/capi_clusters.o" in make


def test_host_labels_equal_a_brute_force_component_search():
    """Self bands of 1 and 2 columns (with and without the second cap) for n in {2, 3, 65, 300, 2100}: random graphs at three
    densities, all-pass and none-pass bands, a star whose hub is not the lowest index, a path in ascending, descending and
    permuted index order, two paths joined by their far ends; the whole triangle and three row ranges that start inside it;
    four chained ranges, and the same four from the identity folded with the merge, against the whole call; n = 1 and n = 0."""
    out = run("labels").split()
    assert out[0] == "ok" and int(out[1]) >= 5 * 9 * 3 * 5


def test_merge_and_label_check():
    """A links (0,1) and (2,3), B links (1,2): one cluster.  Identity on either side, a partition with itself, random unflattened
    partitions against the brute force.  The check accepts every output and refuses labels[0] = 1, labels[3] = 7, a value
    equal to n and one far beyond it; a refused merge leaves both arrays and the count untouched."""
    out = run("merge").split()
    assert out[0] == "ok" and int(out[1]) >= 30
