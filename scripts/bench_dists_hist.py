#!/usr/bin/env python3
"""What the histogram of a collection's distances costs on the GPU (csrc/hist.hip, csrc/capi_hist.cpp) beside the calls it is
built like, on one MI355X.  Modelled on scripts/bench_clusters_within.py: the same generator (self core/accessory over n
clustered synthetic genomes, 4 096 bins, k = 15..31, relatives at random ids, 50 clusters), n of --n, plus -- with --spike --
one collection in which nearly every pair is stored as (1, 1) or as 0: half the samples are copies of one genome, the rest are
unrelated, so whole waves hit one counter.

On the same data and in the same process, the calls of a data set taken in turn, medians of --reps after a warm-up:
  dense_device   skl_self_dists_all with out_on_device = 1 (the dense path is untouched: the parent commit's figure)
  count          skl_self_dists_within, count-only, at a cap that keeps about 1 % of the pairs: reads each band once, writes
                 almost nothing -- what a one-pass consumer of the band costs
  within         skl_self_dists_within with device outputs sized to the answer, at that cap (count + scan + scatter: two reads
                 of the band): THE YARDSTICK of the 64 x 64 call
  hist 64x64     skl_self_dists_hist on [0, 1] x [0, 1], device counts: hist_lds_kernel
  hist 256x256   the same grid range in 256 x 256 cells: hist_global_kernel
The library under test is the one SKL_LIBRARY names, else the product library: the peel's worth is measured by running this
script once more against a library built with -DSKL_HIST_PEEL_ROUNDS=0 (--label says which, for the table).

Prints the table and one JSON line; --out also writes the table to a file."""
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
GRIDS = {"64x64": (0, 1, 64, 0, 1, 64), "256x256": (0, 1, 256, 0, 1, 256)}


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


def one_set(ctx, torch, name, bins, n, reps, with_within):
    s = ctx.sketches(bins, n, KMERS, SS64)
    p = s.set_k()
    pairs = capi.self_pairs(n)
    out = {"data": name, "n": n, "pairs": pairs}
    dense = torch.zeros((pairs, 2), dtype=torch.float32, device="cuda:0")
    counts = {g: torch.zeros(grid[2] * grid[5], dtype=torch.int64, device="cuda:0") for g, grid in GRIDS.items()}
    fns = [lambda: capi.self_dists_all(ctx, s, p, out=dense)]
    names = ["dense_device"]
    if with_within:
        rows = torch.zeros((capi.self_pairs(n, 0, 64), 2), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        capi.self_dists_rows(ctx, s, p, 0, 64, out=rows)
        ctx.synchronize()
        cap = (float(torch.sort(rows[:, 0]).values[int(rows.shape[0] * 0.01)]), INF)
        del rows
        found = capi.count_within(ctx, s, p, *cap)
        room = max(found, 1)
        o = (torch.zeros(room, dtype=torch.int32, device="cuda:0"), torch.zeros(room, dtype=torch.int32, device="cuda:0"),
             torch.zeros((room, 2), dtype=torch.float32, device="cuda:0"))
        out.update({"cap": cap[0], "found": found, "share": found / pairs})
        fns += [lambda: capi.count_within(ctx, s, p, *cap), lambda: capi.dists_within_into(ctx, s, p, *cap, out=o, capacity=room)]
        names += ["count", "within"]
    torch.cuda.synchronize()
    for g, grid in GRIDS.items():
        fns.append(lambda g=g, grid=grid: capi.dists_hist(ctx, s, p, grid, counts=counts[g]))      # (accumulates: nothing is zeroed or copied)
        names.append("hist " + g)
    for name_, (t, spread) in zip(names, interleaved(ctx, fns, reps)):
        out[name_] = {"call_s": round(t, 5), "spread_s": spread}
    # what the histogram looks like, from one fresh call each; the device counts hold reps + 1 calls
    for g, grid in GRIDS.items():
        h, outside, nan = capi.dists_hist(ctx, s, p, grid)
        out["hist " + g].update({"kernel": ctx.last_kernel(), "occupied": int((h > 0).sum()), "largest_share": float(h.max()) / pairs,
                                 "second_share": float(np.sort(h.reshape(-1))[-2]) / pairs, "outside": outside, "nan": nan})
        assert int(h.sum()) + outside + nan == pairs
        assert np.array_equal(counts[g].cpu().numpy().view(np.uint64).reshape(h.shape), (reps + 1) * h), "accumulated device counts differ from reps + 1 fresh calls"
    s.close()
    del dense, counts
    torch.cuda.empty_cache()
    return out


def spike_set(torch, n):
    """n / 2 copies of ONE genome, then n / 2 unrelated genomes: pairs of copies are stored as 0, nearly all others as (1, 1)."""
    one = synth.set_clustered_device(1, len(KMERS), SS64, "cuda:0", keep=KEEP, n_clusters=1)
    rest = synth.set_clustered_device(n - n // 2, len(KMERS), SS64, "cuda:0", keep=KEEP, n_clusters=n - n // 2, first_sample=n, seed=synth.SEED_R + 1)
    return torch.cat([one.expand(n // 2, *one.shape[1:]).contiguous(), rest])


def ms(t):
    return f"{t * 1e3:.2f} ms" if t < 1 else f"{t:.3f} s"


def cell(r, key):
    if key not in r:
        return "–"
    return f"{ms(r[key]['call_s'])} ({ms(r[key]['spread_s'][0])}–{ms(r[key]['spread_s'][1])})"


def table(results, label):
    lines = ["| library | data set | largest cell, second (64 x 64) | dense, device | count-only | within (yardstick; min–max) | hist 64 x 64, LDS kernel (min–max) | hist 256 x 256, global kernel (min–max) | 64 x 64 / within | 64 x 64 / count | 256 x 256 / count |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        h64, h256 = r["hist 64x64"], r["hist 256x256"]
        ratio = lambda a, key: f"{a['call_s'] / r[key]['call_s']:.3f}" if key in r else "–"      # noqa: E731
        lines.append(f"| {label} | {r['data']}, n = {r['n']} | {100 * h64['largest_share']:.1f} %, {100 * h64['second_share']:.1f} % | {cell(r, 'dense_device')} | "
                     f"{cell(r, 'count')} | {cell(r, 'within')} | {cell(r, 'hist 64x64')} | {cell(r, 'hist 256x256')} | {ratio(h64, 'within')} | {ratio(h64, 'count')} | "
                     f"{ratio(h256, 'count')} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", default="16000,100000")
    ap.add_argument("--clusters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spike", default="", help="sizes of the all-(1, 1)-or-0 collection (comma-separated; default: none)")
    ap.add_argument("--label", default="product", help="what the table calls the library under test")
    ap.add_argument("--out", default="", help="also write the table to this file (profiles/dists_hist.md holds the tables of several runs, put there by hand)")
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("bench_dists_hist.py: no gfx950 device visible")
    import torch

    ctx = capi.Context(0)
    results = []
    for n in (int(x) for x in args.n.split(",") if x):
        bins = synth.set_clustered_device(n, len(KMERS), SS64, "cuda:0", keep=KEEP, n_clusters=args.clusters, scatter=True)
        torch.cuda.synchronize()
        results.append(one_set(ctx, torch, f"{args.clusters} clusters", bins, n, args.reps, True))
        del bins
        torch.cuda.empty_cache()
    for n in (int(x) for x in args.spike.split(",") if x):
        bins = spike_set(torch, n)
        torch.cuda.synchronize()
        results.append(one_set(ctx, torch, "half copies of one genome, half unrelated", bins, n, args.reps, False))
        del bins
        torch.cuda.empty_cache()
    ctx.close()
    print(table(results, args.label))
    if args.out:
        with open(args.out, "w") as f:
            f.write(table(results, args.label))
    print(json.dumps({"library": args.label, "sets": results}))


if __name__ == "__main__":
    main()
