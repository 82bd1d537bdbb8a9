#!/usr/bin/env python3
"""`inverted query --top N` on one MI355X (csrc/inv_top.hip behind csrc/inv_query.hip).

An index of N samples x S u16 bins (default 1 M x 1 000) against Q = 1 024 queries, half of them copies of indexed samples,
half unrelated.  Per `top` in {1, 10, 1 024}: the call time of skl_inverted_query_top (query upload + relayout + counts
kernel + selection kernel + top x 8 bytes per query back), warm-up first, then the median of --reps calls with the spread;
and the selection kernel's own time, summed over the call's bands, from the context's event brackets in one more call
(ctx.kernel_ms; the brackets are off in the timed calls).  The baseline is skl_inverted_query in match-count mode in the
same process: every count to the host, which is what a caller had to fetch -- and then sort -- before.  The counts
kernel's own time comes from a `rocprofv3 --kernel-trace --stats` run of this script (--reps 1 --no-baseline), which
lists both kernels.

Every result is checked against numpy on a few queries.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from sketchlib.rust_amd import capi  # noqa: E402


def clustered(rng, n, S, n_clusters=1000, keep=0.8, rows=100_000):
    """bench_inverted_query.py's index (samples around 1 000 centres, a fifth of the bins redrawn), made in slices."""
    centres = rng.integers(0, 65536, size=(n_clusters, S), dtype=np.uint16)
    R = np.empty((n, S), dtype=np.uint16)
    for r0 in range(0, n, rows):
        part = centres[rng.integers(0, n_clusters, min(rows, n - r0))]
        mutate = rng.random(part.shape, dtype=np.float32) >= keep
        part[mutate] = rng.integers(0, 65536, size=int(mutate.sum()), dtype=np.uint16)
        R[r0:r0 + rows] = part
    return R


def timed(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        times.append(time.perf_counter() - t0)
    return res, {"call_s": round(float(np.median(times)), 5), "spread_s": [round(min(times), 5), round(max(times), 5)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--sketch-size", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--tops", type=int, nargs="+", default=[1, 10, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("bench_inverted_top.py: no gfx950 device visible")
    rng = np.random.default_rng(1)
    n, S, nq = args.n, args.sketch_size, args.queries
    R = clustered(rng, n, S)
    Q = R[rng.integers(0, n, nq)].copy()
    Q[nq // 2:] = rng.integers(0, 65536, size=(nq - nq // 2, S), dtype=np.uint16)
    ctx = capi.Context(0)
    ix = capi.Inverted(ctx, R)
    out = {"n": n, "sketch_size": S, "queries": nq, "reps": args.reps, "band_queries": ix.band_queries(capi.INVQ_MATCH_COUNT),
           "digit_passes": 1 if S <= 2047 else 2, "top": {}}
    spot = {q: (R == Q[q]).sum(1, dtype=np.uint32) for q in (0, nq // 2 - 1, nq - 1)}
    for top in args.tops:
        ix.top(Q[:64], top)   # warm-up (code objects, allocations)
        (ids, cnt), t = timed(lambda: ix.top(Q, top), args.reps)
        ctx.timing_enable(1)
        ctx.timing_reset()
        ix.top(Q, top)
        ms, launches = ctx.kernel_ms()
        ctx.timing_enable(0)
        t["select_kernel_ms"] = round(ms, 3)
        t["select_launches"] = launches
        t["queries_per_s"] = round(nq / t["call_s"], 1)
        t["bytes_back"] = int(ids.nbytes + cnt.nbytes)
        for q, counts in spot.items():
            keys = (counts.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
            best = np.sort(keys)[::-1][:top]
            assert np.array_equal(ids[q][:best.size], (best & np.uint64(0xFFFFFFFF)).astype(np.uint32)), (top, q)
            assert np.array_equal(cnt[q][:best.size], (best >> np.uint64(32)).astype(np.uint32)), (top, q)
        out["top"][str(top)] = t
    if not args.no_baseline:
        ix.query(Q[:64], capi.INVQ_MATCH_COUNT)
        res, t = timed(lambda: ix.query(Q, capi.INVQ_MATCH_COUNT), args.reps)
        t["bytes_back"] = int(res.nbytes)
        for q, counts in spot.items():
            assert np.array_equal(res[q], counts), q
        # what the caller still had to do for the ten best of ONE query: a partial sort of its row on the host
        t0 = time.perf_counter()
        keys = (res[0].astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        np.partition(keys, n - 10)[n - 10:]
        t["host_top10_of_one_row_s"] = round(time.perf_counter() - t0, 5)
        out["match_count_baseline"] = t
    ix.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
