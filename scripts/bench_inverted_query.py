#!/usr/bin/env python3
"""`inverted query` on one MI355X (csrc/inv_query.hip).

Kernel shape: an index of N samples x S u16 bins (default 1 M x 1 000) against Q = 1 024 queries, through
skl_inverted_query in every mode.  Reports per mode the call time (query upload + relayout + kernel + the
results' copy to the host), queries/s, pairs/s and the fraction of the VALU peak the call reaches: 17 VALU
lane-ops per (pair, 32 bins) (1 v_xnor + 15 v_bitop3 + 1 v_bcnt) against 256 CUs x 4 SIMDs x 32 lanes x
2.4 GHz = 78.64 T lane-op/s.  The kernel's own time comes from a `rocprofv3 --kernel-trace --stats` run of
this script (--no-e2e --reps 2).

End to end: `sketchlib inverted query` on a synthetic .ski of --e2e-n samples (written with
`skl_dbtool make-ski` from a clustered .skq, k = 21, S = 1 000), queried with the four genomes of
tests/golden/reference_fixtures, in match-count and any-bins mode, with SKL_CLI_TIMING=1 phases.

Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from sketchlib.rust_amd import capi  # noqa: E402

VALU_PEAK = 256 * 4 * 32 * 2.4e9
BUILD = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build")
FIXTURES = os.path.join(ROOT, "tests", "golden", "reference_fixtures")


def clustered(rng, n, S, n_clusters=1000, keep=0.8):
    centres = rng.integers(0, 65536, size=(n_clusters, S), dtype=np.uint16)
    R = centres[rng.integers(0, n_clusters, n)]
    mutate = rng.random((n, S)) >= keep
    R[mutate] = rng.integers(0, 65536, size=int(mutate.sum()), dtype=np.uint16)
    return R


def kernel_bench(args):
    rng = np.random.default_rng(1)
    n, S, nq = args.n, args.sketch_size, args.queries
    R = clustered(rng, n, S)
    Q = R[rng.integers(0, n, nq)].copy()
    Q[nq // 2:] = rng.integers(0, 65536, size=(nq - nq // 2, S), dtype=np.uint16)
    ctx = capi.Context(0)
    t0 = time.perf_counter()
    ix = capi.Inverted(ctx, R)
    t_create = time.perf_counter() - t0
    words = (S + 31) // 32
    lane_ops = n * nq * (words * 17 + 1)   # + the tail mask's AND on the last word
    out = {"n": n, "sketch_size": S, "queries": nq, "create_s": round(t_create, 4),
           "band_queries": ix.band_queries(capi.INVQ_MATCH_COUNT)}
    for name, mode in (("all-bins", capi.INVQ_ALL_BINS), ("any-bins", capi.INVQ_ANY_BINS),
                       ("match-count", capi.INVQ_MATCH_COUNT)):
        ix.query(Q[:64], mode)   # warm-up (code objects, allocations)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res = ix.query(Q, mode)
            times.append(time.perf_counter() - t0)
        t = float(np.median(times))
        out[name] = {"call_s": round(t, 5), "queries_per_s": round(nq / t, 1), "pairs_per_s": float(f"{n * nq / t:.4g}"),
                     "valu_peak_fraction": round(lane_ops / t / VALU_PEAK, 4), "spread_s": [round(min(times), 5), round(max(times), 5)]}
        if name == "match-count":
            # spot check against numpy on a few queries
            for q in (0, nq - 1):
                assert np.array_equal(res[q], (R == Q[q]).sum(1, dtype=np.uint32)), q
        del res
    ix.close()
    ctx.close()
    return out


def e2e_bench(args):
    n, S = args.e2e_n, 1000
    rng = np.random.default_rng(2)
    R = clustered(rng, n, S)
    res = {"n": n, "sketch_size": S}
    with tempfile.TemporaryDirectory() as d:
        R.astype("<u2").tofile(os.path.join(d, "index.skq"))
        with open(os.path.join(d, "names.txt"), "w") as f:
            f.writelines(f"sample_{i}\n" for i in range(n))
        t0 = time.perf_counter()
        subprocess.run([os.path.join(BUILD, "skl_dbtool"), "make-ski", os.path.join(d, "index"), "21", str(S),
                        "@" + os.path.join(d, "names.txt")], check=True, capture_output=True)
        res["make_ski_s"] = round(time.perf_counter() - t0, 2)
        res["ski_bytes"] = os.path.getsize(os.path.join(d, "index.ski"))
        with open(os.path.join(FIXTURES, "rfile.txt")) as f:
            qlist = [line.rstrip("\n").split("\t") for line in f if line.strip()]
        with open(os.path.join(d, "queries.txt"), "w") as f:
            f.writelines(f"{name}\t{os.path.join(FIXTURES, path)}\n" for name, path in qlist)
        res["queries"] = len(qlist)
        for mode in ("match-count", "any-bins"):
            cmd = [os.path.join(BUILD, "sketchlib"), "inverted", "query", os.path.join(d, "index.ski"), "-f",
                   os.path.join(d, "queries.txt"), "--query-type", mode, "--threads", "4", "-o", os.path.join(d, "out.txt")]
            t0 = time.perf_counter()
            p = subprocess.run(cmd, check=True, capture_output=True, text=True, env={**os.environ, "SKL_CLI_TIMING": "1"})
            wall = time.perf_counter() - t0
            timing = [line for line in p.stderr.splitlines() if line.startswith("TIMING")]
            res[mode] = {"wall_s": round(wall, 3), "timing": timing[0] if timing else None,
                         "output_bytes": os.path.getsize(os.path.join(d, "out.txt"))}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--sketch-size", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--e2e-n", type=int, default=50_000)
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("bench_inverted_query.py: no gfx950 device visible")
    out = {"kernel": kernel_bench(args)}
    if not args.no_e2e:
        out["e2e"] = e2e_bench(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
