#!/usr/bin/env python3
"""What the minimum spanning tree of the distances costs on the GPU (csrc/mst.hip, csrc/capi_mst.cpp) beside the call it shares
its dense pass with, on one MI355X.  Modelled on scripts/bench_clusters_within.py: the same generator (self core/accessory over
n clustered synthetic genomes, 4 096 bins, k = 15..31, relatives at random ids, 50 clusters), n of --n.

On the same data and in the same process, taken in turn, medians of --reps after a warm-up:
  clusters   skl_self_clusters_within with an infinite cap: one dense pass over the triangle plus the union kernel, which joins
             every pair -- the same dense pass as a Boruvka round with a cheaper consumer: THE YARDSTICK
  mst        skl_self_mst, column 0, no cap, host outputs: `passes` dense passes, each followed by the min-edge kernel
A round's cost is mst / passes (a tree is finished by the round that adds its last edge, so passes == rounds; a forest needs one
more pass to find that nothing is left), and round / clusters is what the min-edge kernel costs over the union kernel.

--ablation-library PATH repeats the measurement with another build of the library (csrc/mst.hip compiled with
-DMST_ROW_REDUCE=0: every live position sends its own atomic to best[row]), which records what the row-side wave reduction buys.

Prints one JSON line and writes the table to --out (default profiles/mst.md)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from sketchlib.rust_amd import capi, synth  # noqa: E402

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


def one_set(build, n, clusters, reps):
    import torch

    ctx = capi.Context(0)
    bins = synth.set_clustered_device(n, len(KMERS), SS64, "cuda:0", keep=KEEP, n_clusters=clusters, scatter=True)
    torch.cuda.synchronize()
    s = ctx.sketches(bins, n, KMERS, SS64)
    del bins
    p = s.set_k()
    (t_clu, sp_clu), (t_mst, sp_mst) = interleaved(ctx, [lambda: capi.clusters_within(ctx, s, p, INF), lambda: capi.mst(ctx, s, p)], reps)
    _labels, n_clusters = capi.clusters_within(ctx, s, p, INF)
    i, j, w, rounds, labels = capi.mst(ctx, s, p, labels=True)
    kernel = ctx.last_kernel()
    passes = rounds if i.size == n - 1 else rounds + 1
    assert i.size == n - n_clusters and (np.diff(w) >= 0).all() and (i < j).all()
    row = {"build": build, "n": n, "pairs": capi.self_pairs(n), "clusters_data": clusters, "edges": int(i.size), "components": int(n - i.size),
           "rounds": rounds, "passes": passes, "clusters_s": round(t_clu, 5), "clusters_spread_s": sp_clu, "mst_s": round(t_mst, 5),
           "mst_spread_s": sp_mst, "round_s": round(t_mst / passes, 5), "round_over_clusters": round(t_mst / passes / t_clu, 4),
           "heaviest_edge": float(w[-1]) if w.size else None, "kernel": kernel}
    s.close()
    ctx.close()
    torch.cuda.empty_cache()
    return row


def ms(t):
    return f"{t * 1e3:.2f} ms" if t < 1 else f"{t:.3f} s"


def table(rows):
    lines = ["| build | n | pairs | edges (components) | rounds | dense passes | clusters, infinite cap (yardstick; min–max) | mst (min–max) | a round | round / clusters |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['build']} | {r['n']} | {r['pairs']} | {r['edges']} ({r['components']}) | {r['rounds']} | {r['passes']} | "
                     f"{ms(r['clusters_s'])} ({ms(r['clusters_spread_s'][0])}–{ms(r['clusters_spread_s'][1])}) | "
                     f"{ms(r['mst_s'])} ({ms(r['mst_spread_s'][0])}–{ms(r['mst_spread_s'][1])}) | {ms(r['round_s'])} | {r['round_over_clusters']:.3f} |")
    return "\n".join(lines) + "\n"


TABLE_BEGIN, TABLE_END = "<!-- table written by scripts/bench_mst.py -->\n", "<!-- end of the table -->\n"


def write_table(path, text):
    """The table goes between the two markers of `path` when it has them (the profile's reading of the figures around it is
    written by hand and is NOT updated: re-read it after a new run); otherwise the file is the table."""
    doc = open(path).read() if os.path.exists(path) else ""
    if TABLE_BEGIN in doc and TABLE_END in doc:
        text = doc[:doc.index(TABLE_BEGIN) + len(TABLE_BEGIN)] + text + doc[doc.index(TABLE_END):]
    else:
        text = TABLE_BEGIN + text + TABLE_END
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", default="16000,100000")
    ap.add_argument("--clusters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ablation-library", default=None, help="a build with -DMST_ROW_REDUCE=0 to measure beside the product library")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mst.md"))
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("bench_mst.py: no gfx950 device visible")
    rows = []
    for n in (int(x) for x in args.n.split(",")):
        rows.append(one_set("product", n, args.clusters, args.reps))
        print(json.dumps(rows[-1]), flush=True)
        if args.ablation_library:
            with capi.using_library(args.ablation_library):
                rows.append(one_set("row reduction compiled out", n, args.clusters, args.reps))
            print(json.dumps(rows[-1]), flush=True)
    write_table(args.out, table(rows))
    print(json.dumps({"rows": rows}))


if __name__ == "__main__":
    main()
