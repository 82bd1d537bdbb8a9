#!/usr/bin/env python3
"""What picking the pairs within a distance cap on the GPU costs beside the dense call it follows (csrc/within.hip,
csrc/capi_within.cpp), on one MI355X.

Self core/accessory over n clustered synthetic genomes (4 096 bins, k = 15..31, relatives at random ids), for each n of --n
and each number of clusters of --clusters (50 clusters: 2 % of the pairs are related).  0.6 % of ALL pairs of this generator
come out at exactly (0, 0) whatever the number of clusters, so no cap keeps a share between 0 and 0.6 %; the caps below are
the ones the data allow.

  within        skl_self_dists_within with device outputs, at caps that keep nothing (core <= 0 and accessory <= -1), the
                pairs at distance 0 (core <= 0: 0.6 %), and 1 % of the pairs (the quantile of the core distances of the
                first 64 rows, if it lies below 0.5); and count-only at the last of these;
  dense_device  skl_self_dists_all with out_on_device = 1: what the same library spends on the distances alone (the dense
                path is untouched by the filter, so this is the parent commit's figure on the same chip and data);
  host_filter   (first number of clusters only) what a caller does without the call: skl_self_dists_all into host memory,
                then the same predicate in numpy and a take of the survivors, in slices of 64 Mi pairs, at the cap of 0.

Each is a whole call timed by a host clock between device synchronisations, the median of --reps after a warm-up, the
calls of a size taken in turn within every repetition.  The filter's cost is within - dense_device; its traffic is 16 B per
pair (the count and the scatter each read the 8 B record once; the dense epilogue's own 8 B store is in both figures) over
that cost, against the HBM peak of 8 TB/s.

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from sketchlib.rust_amd import capi, synth  # noqa: E402

HBM_PEAK = 8.0e12
KMERS = [15, 19, 23, 27, 31]
KEEP = [0.97, 0.955, 0.94, 0.925, 0.91]
SS64 = 64


def interleaved(ctx, fns, reps):
    """Every fn warmed up, then `reps` rounds of all of them in turn -> per fn (median seconds, [min, max])."""
    for fn in fns:   # warm-up: code objects, scratch, the early-break decision, first touch of host pages
        fn()
    ctx.synchronize()
    wall = [[] for _ in fns]
    for _ in range(reps):
        for w, fn in zip(wall, fns):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            w.append(time.perf_counter() - t0)
    return [(float(np.median(w)), [round(min(w), 5), round(max(w), 5)]) for w in wall]


def one_size(ctx, torch, n, n_clusters, reps, host_reps):
    bins = synth.set_clustered_device(n, len(KMERS), SS64, "cuda:0", keep=KEEP, n_clusters=n_clusters, scatter=True)
    torch.cuda.synchronize()
    s = ctx.sketches(bins, n, KMERS, SS64)
    p = s.set_k()
    pairs = capi.self_pairs(n)
    out = {"n": n, "clusters": n_clusters, "pairs": pairs, "sketchsize64": SS64, "kmers": KMERS}

    # the 1 % cap: a quantile of the core distance over the first 64 rows, if it lies among the related pairs
    rows = torch.zeros((capi.self_pairs(n, 0, 64), 2), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    capi.self_dists_rows(ctx, s, p, 0, 64, out=rows)
    ctx.synchronize()
    q01 = float(torch.sort(rows[:, 0]).values[int(rows.shape[0] * 0.01)])
    caps = {"nothing": (0.0, -1.0), "at distance 0": (0.0, float("inf"))}
    if q01 < 0.5:
        caps["1%"] = (q01, float("inf"))
    last = list(caps)[-1]
    del rows

    dense = torch.zeros((pairs, 2), dtype=torch.float32, device="cuda:0")
    outs = {}
    for label, cap in caps.items():
        found = capi.count_within(ctx, s, p, *cap)
        room = max(found, 1)
        outs[label] = (found, room, (torch.zeros(room, dtype=torch.int32, device="cuda:0"), torch.zeros(room, dtype=torch.int32, device="cuda:0"),
                                     torch.zeros((room, 2), dtype=torch.float32, device="cuda:0")))
    torch.cuda.synchronize()

    def within(label):
        found, room, o = outs[label]
        return lambda: capi.dists_within_into(ctx, s, p, *caps[label], out=o, capacity=room)

    fns = [lambda: capi.self_dists_all(ctx, s, p, out=dense)] + [within(label) for label in caps] + [lambda: capi.count_within(ctx, s, p, *caps[last])]
    times = interleaved(ctx, fns, reps)
    t_dense, spread = times[0]
    capi.self_dists_all(ctx, s, p, out=dense)
    ctx.synchronize()
    out["dense_device"] = {"call_s": round(t_dense, 5), "spread_s": spread, "kernel": ctx.last_kernel()}

    def costs(t):
        cost = t - t_dense
        return {"filter_cost_s": round(cost, 5), "filter_cost_of_dense": round(cost / t_dense, 3),
                "filter_hbm_peak_fraction": round(16.0 * pairs / cost / HBM_PEAK, 3) if cost > 0 else None}

    out["within"] = []
    for (label, cap), (t, spread) in zip(caps.items(), times[1:]):
        found, _room, (oi, oj, od) = outs[label]
        # the same answer as a filter of the library's own dense result (values and count; the tests hold it to the oracle)
        assert found == int(((dense[:, 0] <= cap[0]) & (dense[:, 1] <= cap[1])).sum()) and bool((od[:found, 0] <= cap[0]).all()), label
        out["within"].append({"keeps": label, "max_first": cap[0], "max_second": cap[1] if cap[1] != float("inf") else "inf",
                              "found": found, "share": found / pairs, "call_s": round(t, 5), "spread_s": spread, **costs(t)})
    capi.dists_within_into(ctx, s, p, *caps[last], out=outs[last][2], capacity=outs[last][1])
    out["kernel"] = ctx.last_kernel()
    t, spread = times[-1]
    out["count_only"] = {"keeps": last, "call_s": round(t, 5), "spread_s": spread, **costs(t)}
    del dense, outs
    torch.cuda.empty_cache()

    # what a caller does today: the dense matrix to the host, filtered there
    if host_reps:
        host = np.empty((pairs, 2), dtype=np.float32)
        step = 64 << 20

        def host_filter(cap):
            capi.self_dists_all(ctx, s, p, out=host)
            kept = []
            for a in range(0, pairs, step):
                blk = host[a:a + step]
                idx = np.flatnonzero((blk[:, 0] <= np.float32(cap[0])) & (blk[:, 1] <= np.float32(cap[1])))
                kept.append((idx + a, blk[idx]))
            return sum(k[0].size for k in kept)

        (t_copy, spread_copy), (t_host, spread) = interleaved(ctx, [lambda: capi.self_dists_all(ctx, s, p, out=host),
                                                                   lambda: host_filter(caps["at distance 0"])], host_reps)
        out["host_filter"] = {"keeps": "at distance 0", "call_s": round(t_host, 4), "spread_s": spread, "dense_to_host_s": round(t_copy, 4),
                              "dense_to_host_spread_s": spread_copy, "found": host_filter(caps["at distance 0"])}
        del host
    s.close()
    del bins
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", default="16000,100000")
    ap.add_argument("--clusters", default="50", help="comma-separated; the host-filter baseline runs at the first")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3, help="0: skip the host-filter baseline")
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("bench_dist_within.py: no gfx950 device visible")
    import torch

    ctx = capi.Context(0)
    clusters = [int(c) for c in args.clusters.split(",")]
    out = {"sizes": [one_size(ctx, torch, int(n), c, args.reps, args.host_reps if c == clusters[0] else 0)
                     for n in args.n.split(",") for c in clusters]}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
