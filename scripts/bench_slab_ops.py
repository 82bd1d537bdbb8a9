#!/usr/bin/env python3
"""What a resident select / concat saves over re-uploading the slab (csrc/slab_ops.hip, csrc/capi_slab.cpp), on one MI355X.

At 1 000 000 samples x 1 024 bins, with one k-mer length and -- if device and host memory allow -- with five, it times

  select    skl_sketches_select of a random 90 % keep list (ascending, as remove_genomes keeps samples);
  concat    skl_sketches_concat of 990 000 + 10 000 samples;
  reupload  what a caller has to do without them: skl_sketches_create of the same result from (pageable) host memory.
            The host copy of the result is made outside the timed region, which flatters the re-upload: a caller that
            deletes samples also has to gather the rows on the host first.

Each is a whole call, timed by a host clock between device synchronisations (every one of these calls ends in one), the
median of --reps after a warm-up; the result slab is destroyed outside the timed region.  The gather kernel alone is timed
by the events skl_ctx_timing_enable puts around its launch; its bytes are the compulsory ones, every kept row read once and
written once (2 x n_ids x row bytes, the id list is 4 B per row on top), over the HBM peak of 8 TB/s (~6.3 TB/s is what
streaming kernels reach on this chip).

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
KMERS = {1: [21], 5: [15, 19, 23, 27, 31]}


def median_of(ctx, fn, reps, kernel=False):
    """fn() -> a slab; (median seconds of the call, median seconds of the bracketed kernel or None, [min, max])."""
    fn().close()   # warm-up: code objects, the allocator
    wall, kern = [], []
    for _ in range(reps):
        ctx.timing_reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        r = fn()
        ctx.synchronize()
        wall.append(time.perf_counter() - t0)
        if kernel:
            kern.append(ctx.kernel_ms()[0] / 1e3)
        r.close()
    return float(np.median(wall)), (float(np.median(kern)) if kernel else None), [round(min(wall), 5), round(max(wall), 5)]


def one_shape(ctx, torch, n, nk, ss64, reps, n_new):
    row_bytes = nk * ss64 * 112
    bins = synth.set_u_device(n, nk, ss64, "cuda:0")
    torch.cuda.synchronize()
    s = ctx.sketches(bins, n, KMERS[nk], ss64)
    keep = np.sort(np.random.default_rng(7).permutation(n)[: n * 9 // 10]).astype(np.uint32)
    out = {"n": n, "nk": nk, "sketchsize64": ss64, "row_bytes": row_bytes, "slab_bytes": n * row_bytes, "kept": int(keep.size)}

    ctx.timing_enable(1)
    wall, kern, spread = median_of(ctx, lambda: s.select(keep), reps, kernel=True)
    ctx.timing_enable(0)
    moved = 2 * keep.size * row_bytes
    out["select"] = {"call_s": round(wall, 5), "call_spread_s": spread, "kernel_s": round(kern, 6), "kernel": ctx.last_kernel(),
                     "kernel_bytes_per_s": float(f"{moved / kern:.4g}"), "kernel_hbm_peak_fraction": round(moved / kern / HBM_PEAK, 3),
                     "call_bytes_per_s": float(f"{moved / wall:.4g}")}
    # spot check: the result is the kept rows
    sel = s.select(keep)
    probe = np.array([0, 1, keep.size // 2, keep.size - 1], dtype=np.uint32)
    a, b = sel.select(probe), s.select(keep[probe])
    assert np.array_equal(capi.self_binmatch(ctx, a), capi.self_binmatch(ctx, b)) and capi.self_binmatch(ctx, a).max() < 64 * ss64
    for x in (a, b, sel):
        x.close()

    # the same result through host memory
    host = bins.cpu().numpy().view(np.uint64)[keep.astype(np.int64)]
    host = np.ascontiguousarray(host)
    wall_up, _, spread_up = median_of(ctx, lambda: ctx.sketches(host, keep.size, KMERS[nk], ss64), reps)
    out["reupload_of_select_result"] = {"call_s": round(wall_up, 5), "call_spread_s": spread_up,
                                        "host_bytes_per_s": float(f"{keep.size * row_bytes / wall_up:.4g}")}
    out["select"]["times_faster_than_reupload"] = round(wall_up / wall, 1)
    del host

    # concat: 990 000 resident + 10 000 new
    first = ctx.sketches(bins[: n - n_new], n - n_new, KMERS[nk], ss64)
    new = ctx.sketches(bins[n - n_new:].contiguous(), n_new, KMERS[nk], ss64)
    wall_c, _, spread_c = median_of(ctx, lambda: capi.concat(first, new), reps)
    out["concat"] = {"call_s": round(wall_c, 5), "call_spread_s": spread_c, "bytes_per_s": float(f"{2 * n * row_bytes / wall_c:.4g}"),
                     "hbm_peak_fraction": round(2 * n * row_bytes / wall_c / HBM_PEAK, 3)}
    host = bins.cpu().numpy().view(np.uint64)
    wall_cu, _, spread_cu = median_of(ctx, lambda: ctx.sketches(host, n, KMERS[nk], ss64), reps)
    out["reupload_of_concat_result"] = {"call_s": round(wall_cu, 5), "call_spread_s": spread_cu,
                                        "host_bytes_per_s": float(f"{n * row_bytes / wall_cu:.4g}")}
    out["concat"]["times_faster_than_reupload"] = round(wall_cu / wall_c, 1)
    for x in (first, new, s):
        x.close()
    del bins, host
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--sketchsize64", type=int, default=16, help="16 = 1 024 bins")
    ap.add_argument("--new", type=int, default=10_000, help="samples the concat adds")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nk", default="1,5")
    args = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("bench_slab_ops.py: no gfx950 device visible")
    import torch

    ctx = capi.Context(0)
    out = {"shapes": []}
    for nk in (int(x) for x in args.nk.split(",")):
        need = 4 * args.n * nk * args.sketchsize64 * 112   # generator output, source, result, and headroom
        free, _ = torch.cuda.mem_get_info()
        try:
            host_free = os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE")
        except (ValueError, OSError):
            host_free = need
        if free < need or host_free < need:
            out["shapes"].append({"nk": nk, "skipped": f"needs {need >> 30} GiB free on the device and the host, has {free >> 30} / {host_free >> 30}"})
            continue
        out["shapes"].append(one_shape(ctx, torch, args.n, nk, args.sketchsize64, args.reps, args.new))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
