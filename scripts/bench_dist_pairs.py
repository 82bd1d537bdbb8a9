#!/usr/bin/env python3
"""`dist --pairs` on one MI355X (csrc/pair_list.hip): the two-step recipe on a synthetic clustered database.

Step 1 builds the graph with ONE k-mer length (skl_self_dists_knn, single-k keys); step 2 asks for the core/accessory
distance of its edges only (skl_self_dists_pairs, the list grouped by row as the kNN call returns it), into a device
buffer.  Step 2 is timed between device synchronisations after a warm-up: the whole call (work items made on the host,
list upload, kernel) and, from the events skl_ctx_timing_enable puts around the launch, the kernel alone.

Reported: pairs/s; bytes/s from the COMPULSORY bytes -- nk x ss64 x 112 B per pair for the partner's record plus the same
once per run of up to 64 pairs for the row's -- and that figure over the HBM peak (8 TB/s).  The yardstick beside it is the
candidate-list kernel's 0.88 of the peak (pair_cand.hip, single-k keys).  The same list shuffled (runs of one: twice the
bytes per pair) is timed too.  For context only: the core/accessory `--knn` over the same database.

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
CAND_KERNEL_FRACTION = 0.88


def runs_of(a):
    """Work items of a list: runs of equal first sample, cut at 64."""
    starts = np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1]]))
    lengths = np.diff(np.concatenate([starts, [a.size]]))
    return int(((lengths + 63) // 64).sum())


def timed(ctx, fn, reps):
    fn()   # warm-up (code objects, allocations)
    ctx.synchronize()
    wall, kern = [], []
    for _ in range(reps):
        ctx.timing_reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        wall.append(time.perf_counter() - t0)
        kern.append(ctx.kernel_ms()[0] / 1e3)
    return float(np.median(wall)), float(np.median(kern)), [round(min(wall), 5), round(max(wall), 5)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--kmers", default="17,21,25,29")
    ap.add_argument("--sketchsize64", type=int, default=16)
    ap.add_argument("--knn", type=int, default=50)
    ap.add_argument("--graph-k", type=int, default=21)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-coreacc-knn", action="store_true", help="skip the core/accessory --knn timed for context")
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("bench_dist_pairs.py: no gfx950 device visible")
    import torch

    kmers = [int(k) for k in args.kmers.split(",")]
    n, nk, ss64 = args.n, len(kmers), args.sketchsize64
    ctx = capi.Context(0)
    ctx.set_knn_ties(capi.TIES_CANONICAL)
    bins = synth.set_clustered_device(n, nk, ss64, "cuda:0")
    torch.cuda.synchronize()
    s = ctx.sketches(bins, n, kmers, ss64)
    del bins
    out = {"n": n, "kmers": kmers, "sketchsize64": ss64, "knn": args.knn, "record_bytes": nk * ss64 * 112}

    t0 = time.perf_counter()
    idx, _, _ = capi.self_dists_knn(ctx, s, s.set_k(args.graph_k), args.knn)
    out["single_k_knn_s"] = round(time.perf_counter() - t0, 4)
    a = np.repeat(np.arange(n, dtype=np.uint32), args.knn)
    b = idx.reshape(-1).astype(np.uint32)
    n_pairs = a.size
    dev = torch.empty((n_pairs, 2), dtype=torch.float32, device="cuda:0")
    p = s.set_k()
    ctx.timing_enable(1)
    order = np.random.default_rng(1).permutation(n_pairs)
    for name, (la, lb) in (("knn_edges_grouped", (a, b)), ("knn_edges_shuffled", (a[order], b[order]))):
        wall, kern, spread = timed(ctx, lambda: capi.self_dists_pairs(ctx, s, p, la, lb, out=dev), args.reps)
        compulsory = (n_pairs + runs_of(la)) * nk * ss64 * 112
        res = {"pairs": n_pairs, "work_items": runs_of(la), "compulsory_bytes": compulsory, "kernel": ctx.last_kernel().split(" (")[0],
               "call_s": round(wall, 5), "call_spread_s": spread, "call_pairs_per_s": float(f"{n_pairs / wall:.4g}")}
        if kern > 0:
            res.update({"kernel_s": round(kern, 6), "kernel_pairs_per_s": float(f"{n_pairs / kern:.4g}"),
                        "kernel_bytes_per_s": float(f"{compulsory / kern:.4g}"),
                        "kernel_hbm_peak_fraction": round(compulsory / kern / HBM_PEAK, 4)})
        res["call_hbm_peak_fraction"] = round(compulsory / wall / HBM_PEAK, 4)
        out[name] = res
    ctx.timing_enable(0)
    out["yardstick_candidate_kernel_hbm_peak_fraction"] = CAND_KERNEL_FRACTION
    # spot check: the listed values are the dense call's
    rows = capi.self_dists_rows(ctx, s, p, 0, 1)
    got = dev.cpu().numpy()[order.argsort()][:args.knn]
    cols = b[:args.knn].astype(np.int64)
    keep = cols != 0
    assert np.array_equal(got[keep], rows[cols[keep] - 1]), "pair list disagrees with the dense row"
    if not args.no_coreacc_knn:
        capi.self_dists_knn(ctx, s, p, args.knn, 0, 64)   # warm-up of the forms involved
        ctx.synchronize()
        t0 = time.perf_counter()
        capi.self_dists_knn(ctx, s, p, args.knn)
        out["coreacc_knn_s_for_context"] = round(time.perf_counter() - t0, 4)
    s.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
