#!/usr/bin/env python3
"""What single-linkage clustering under a distance cap costs on the GPU (csrc/cluster.hip, csrc/capi_clusters.cpp) beside the
calls it is built from, on one MI355X.  Modelled on scripts/bench_dist_within.py: the same generator (self core/accessory over
n clustered synthetic genomes, 4 096 bins, k = 15..31, relatives at random ids, 50 clusters), n of --n, plus one data set in
which half the samples form ONE cluster and the rest are unrelated (every passing pair hooks into the same tree: contention).

On the same data and in the same process, the calls of a data set taken in turn, medians of --reps after a warm-up:
  dense_device   skl_self_dists_all with out_on_device = 1 (the dense path is untouched: the parent commit's figure)
  count          skl_self_dists_within, count-only, at the cap
  within         skl_self_dists_within with device outputs sized to the answer, at the cap: THE YARDSTICK
  clusters       skl_self_clusters_within with device labels, at the cap
  host_clusters  (n <= --host-n only) what a caller does today: the within call into host arrays, then a union-find there
Caps: one that keeps nothing (core <= 0 and accessory <= -1), the pairs at distance 0 (core <= 0), and about 1 % of the pairs
(the quantile of the core distances of the first 64 rows, if it lies below 0.5); the half-cluster data set at core <= 0.5.

The clusters call reads each band once where the within call reads it twice, and writes no records, so it is expected to cost
no more than the within call plus the run-to-run spread of that baseline.  Filter-side traffic: 8 B per pair read once, over
clusters - dense_device, against the HBM peak of 8 TB/s.

Prints one JSON line and writes the table to --out (default profiles/clusters_within.md)."""
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
INF = float("inf")


def interleaved(ctx, fns, reps):
    """Every fn warmed up, then `reps` rounds of all of them in turn -> per fn (median seconds, [min, max])."""
    for fn in fns:
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


def host_union_find(n, i, j):
    """The caller's side today: scipy is not assumed; numpy rounds of hooking and pointer jumping, label = lowest index."""
    lab = np.arange(n, dtype=np.int64)
    i, j = i.astype(np.int64), j.astype(np.int64)
    while i.size:
        li, lj = lab[i], lab[j]
        live = li != lj
        if not live.any():
            break
        li, lj = li[live], lj[live]
        lo = np.minimum(li, lj)
        for at in (li, lj, i[live], j[live]):
            np.minimum.at(lab, at, lo)
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    return lab


def one_set(ctx, torch, name, bins, n, caps, reps, host):
    s = ctx.sketches(bins, n, KMERS, SS64)
    p = s.set_k()
    pairs = capi.self_pairs(n)
    out = {"data": name, "n": n, "pairs": pairs, "caps": []}
    if "1%" in caps:
        rows = torch.zeros((capi.self_pairs(n, 0, 64), 2), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        capi.self_dists_rows(ctx, s, p, 0, 64, out=rows)
        ctx.synchronize()
        q01 = float(torch.sort(rows[:, 0]).values[int(rows.shape[0] * 0.01)])
        del rows
        if q01 < 0.5:
            caps = dict(caps, **{"1%": (q01, INF)})
        else:
            caps = {k: v for k, v in caps.items() if k != "1%"}
    dense = torch.zeros((pairs, 2), dtype=torch.float32, device="cuda:0")
    labels = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    state = {}
    for label, cap in caps.items():
        found = capi.count_within(ctx, s, p, *cap)
        room = max(found, 1)
        state[label] = (found, room, (torch.zeros(room, dtype=torch.int32, device="cuda:0"), torch.zeros(room, dtype=torch.int32, device="cuda:0"),
                                      torch.zeros((room, 2), dtype=torch.float32, device="cuda:0")))
    torch.cuda.synchronize()

    def fresh_clusters(cap):
        # (device labels continue from what they hold: the identity is written first, inside the timed window -- 4 B per sample)
        torch.arange(n, dtype=torch.int32, out=labels)
        return capi.clusters_within(ctx, s, p, *cap, labels=labels)

    fns = [lambda: capi.self_dists_all(ctx, s, p, out=dense)]
    for label, cap in caps.items():
        found, room, o = state[label]
        fns += [lambda cap=cap: capi.count_within(ctx, s, p, *cap),
                lambda cap=cap, o=o, room=room: capi.dists_within_into(ctx, s, p, *cap, out=o, capacity=room),
                lambda cap=cap: fresh_clusters(cap)]
    times = interleaved(ctx, fns, reps)
    t_dense, spread = times[0]
    out["dense_device"] = {"call_s": round(t_dense, 5), "spread_s": spread}
    for k, (label, cap) in enumerate(caps.items()):
        (t_count, sp_count), (t_within, sp_within), (t_clu, sp_clu) = times[1 + 3 * k:4 + 3 * k]
        _lab, n_clusters = fresh_clusters(cap)
        kernel = ctx.last_kernel()
        lab = labels.cpu().numpy().view(np.uint32)
        sizes = np.bincount(lab)
        cost = t_clu - t_dense
        row = {"keeps": label, "max_first": cap[0], "max_second": cap[1] if cap[1] != INF else "inf", "found": state[label][0],
               "share": state[label][0] / pairs, "n_clusters": n_clusters, "largest": int(sizes.max()),
               "count_s": round(t_count, 5), "count_spread_s": sp_count, "within_s": round(t_within, 5), "within_spread_s": sp_within,
               "clusters_s": round(t_clu, 5), "clusters_spread_s": sp_clu, "clusters_over_within": round(t_clu / t_within, 4),
               "within_spread_rel": round((sp_within[1] - sp_within[0]) / t_within, 4),
               "union_cost_s": round(cost, 5), "union_hbm_peak_fraction": round(8.0 * pairs / cost / HBM_PEAK, 3) if cost > 0 else None,
               "kernel": kernel}
        if host:
            found, room, _o = state[label]

            def today():
                i, j, _d = capi.self_dists_within(ctx, s, p, *cap, capacity=room)
                return host_union_find(n, i, j)

            (t_host, sp_host), = interleaved(ctx, [today], reps)
            ref = today()
            assert np.array_equal(ref.astype(np.uint32), lab), "the device labels differ from the host union-find over the within call's pairs"
            row.update({"host_clusters_s": round(t_host, 4), "host_clusters_spread_s": sp_host})
        out["caps"].append(row)
    s.close()
    del dense, state, labels
    torch.cuda.empty_cache()
    return out


def half_cluster(torch, n):
    """n / 2 samples of ONE cluster, then n / 2 samples each of a cluster of its own."""
    a = synth.set_clustered_device(n // 2, len(KMERS), SS64, "cuda:0", keep=KEEP, n_clusters=1)
    b = synth.set_clustered_device(n - n // 2, len(KMERS), SS64, "cuda:0", keep=KEEP, n_clusters=n - n // 2, first_sample=n, seed=synth.SEED_R + 1)
    return torch.cat([a, b])


def ms(t):
    return f"{t * 1e3:.2f} ms" if t < 1 else f"{t:.3f} s"


def table(results):
    lines = ["| data set | cap | share kept | clusters (largest) | dense, device | count-only | within (yardstick; min–max) | clusters (min–max) | clusters / within | within's spread | union pass, of the HBM peak | today: within to host + union-find |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        for c in r["caps"]:
            lines.append(f"| {r['data']}, n = {r['n']} | {c['keeps']} | {100 * c['share']:.2f} % ({c['found']}) | {c['n_clusters']} ({c['largest']}) | "
                         f"{ms(r['dense_device']['call_s'])} | {ms(c['count_s'])} | {ms(c['within_s'])} ({ms(c['within_spread_s'][0])}–{ms(c['within_spread_s'][1])}) | "
                         f"{ms(c['clusters_s'])} ({ms(c['clusters_spread_s'][0])}–{ms(c['clusters_spread_s'][1])}) | {c['clusters_over_within']:.3f} | "
                         f"{100 * c['within_spread_rel']:.1f} % | {c['union_hbm_peak_fraction']} | {ms(c['host_clusters_s']) if 'host_clusters_s' in c else '–'} |")
    return "\n".join(lines) + "\n"


TABLE_BEGIN, TABLE_END = "<!-- table written by scripts/bench_clusters_within.py -->\n", "<!-- end of the table -->\n"


def write_table(path, text):
    """The table goes between the two markers of `path` when it has them (the profile's reading of the figures around it is
    written by hand and is NOT updated: re-read it after a new run); otherwise the file is the table."""
    doc = open(path).read() if os.path.exists(path) else ""
    if TABLE_BEGIN in doc and TABLE_END in doc:
        text = doc[:doc.index(TABLE_BEGIN) + len(TABLE_BEGIN)] + text + doc[doc.index(TABLE_END):]
    else:
        text = TABLE_BEGIN + text + TABLE_END
    with open(path, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", default="16000,100000")
    ap.add_argument("--clusters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=16000, help="sizes up to this one also time the caller's side of today (0: never)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clusters_within.md"))
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("bench_clusters_within.py: no gfx950 device visible")
    import torch

    ctx = capi.Context(0)
    results = []
    for n in (int(x) for x in args.n.split(",")):
        bins = synth.set_clustered_device(n, len(KMERS), SS64, "cuda:0", keep=KEEP, n_clusters=args.clusters, scatter=True)
        torch.cuda.synchronize()
        caps = {"nothing": (0.0, -1.0), "at distance 0": (0.0, INF), "1%": None}
        results.append(one_set(ctx, torch, f"{args.clusters} clusters", bins, n, caps, args.reps, n <= args.host_n))
        del bins
        bins = half_cluster(torch, n)
        torch.cuda.synchronize()
        results.append(one_set(ctx, torch, "one cluster of half the samples", bins, n, {"core <= 0.5": (0.5, INF)}, args.reps, False))
        del bins
        torch.cuda.empty_cache()
    ctx.close()
    write_table(args.out, table(results))
    print(json.dumps({"sets": results}))


if __name__ == "__main__":
    main()
