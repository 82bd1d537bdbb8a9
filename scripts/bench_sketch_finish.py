#!/usr/bin/env python3
"""Device-side densify + transpose on one MI355X: what finishing the streams on the device is worth to the
sketching calls.  Three shapes at 1 024 bins and one k-mer length:

  (a) proteomes: 64 samples of 1.5 M residues in 4 000 records each, k = 7 (skl_sketch_*_aa);
  (b) single proteins: 1 M samples of log-normal length around 300, `--concat-fasta` semantics, k = 7 (skl_sketch_*_aa);
  (c) a DNA assembly batch: 64 samples of 1.5 M bases in 40 contigs each, both strands, k = 17 (skl_sketch_*_packed).

For each shape, in one process and alternating, `--repeats` times each after a warm-up call of each:

  signs        the call as it was before the finish kernel existed: skl_sketch_signs_* (raw u64 signs come back; densify and
               transpose were the caller's, on host threads, and are NOT in this figure);
  usigs        skl_sketch_usigs_* (finish kernel behind every batch's bin minima, finished words come back);
  usigs_host   the same entry point under SKL_SKETCH_FINISH=host (signs come back, the library's host threads finish them).

and the finish kernel alone: HIP events around the launches of skl_sketch_finish over the shape's signs.  The three variants'
words are compared byte for byte.  Then `sketchlib sketch` end to end on files of shapes (a) and (b): CPU path at --threads 16,
--gpu, and --gpu under SKL_SKETCH_FINISH=host.  One JSON line per figure.

    bench_sketch_finish.py [--proteomes 64] [--residues 1500000] [--proteins 1000000] [--repeats 5] [--no-cli]"""
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

CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")
BINS = 1024


def set_host_finish(ctx, on):
    if on:
        os.environ["SKL_SKETCH_FINISH"] = "host"
    else:
        os.environ.pop("SKL_SKETCH_FINISH", None)
    ctx.reload_env()


def shape_bench(ctx, shape, signs_call, usigs_call, streams, repeats, **more):
    """signs_call() -> signs; usigs_call() -> (usigs, first, flags)."""
    variants = [("signs", False, signs_call), ("usigs", False, usigs_call), ("usigs_host", True, usigs_call)]
    results = {}
    for name, host, call in variants:            # warm-up: the first call of a size grows the context's buffers
        set_host_finish(ctx, host)
        results[name] = call()
    walls = {name: [] for name, _h, _c in variants}
    for _ in range(repeats):
        for name, host, call in variants:
            set_host_finish(ctx, host)
            t0 = time.perf_counter()
            out = call()
            walls[name].append(time.perf_counter() - t0)
            del out
    set_host_finish(ctx, False)
    same = all(np.array_equal(a, b) for a, b in zip(results["usigs"], results["usigs_host"]))
    flags = results["usigs"][2]
    for name, w in walls.items():
        print(json.dumps({"shape": shape, "variant": name, "num_bins": BINS, "streams": streams, "call_wall_s": sorted(w),
                          "min_s": min(w), "median_s": float(np.median(w)), "max_s": max(w), "spread_s": max(w) - min(w), **more}), flush=True)
    # the finish kernel alone, over the signs of this shape
    signs = results["signs"].reshape(-1, BINS)
    capi.sketch_finish(ctx, signs)
    ctx.timing_enable()
    best = None
    for _ in range(3):
        ctx.timing_reset()
        capi.sketch_finish(ctx, signs)
        kms, launches = ctx.kernel_ms()
        if best is None or kms < best[0]:
            best = (kms, launches)
    ctx.timing_enable(0)
    print(json.dumps({"shape": shape, "variant": "finish kernel alone (skl_sketch_finish, HIP events)", "streams": streams, "kernel_ms": best[0],
                      "kernel_launches": best[1], "sign_bytes_read": int(signs.nbytes), "GB_per_s_read": signs.nbytes / best[0] / 1e6,
                      "kernel": ctx.last_kernel(), "usigs_identical_device_vs_host": bool(same),
                      "streams_densified": int((flags & capi.FINISH_DENSIFIED).astype(bool).sum()),
                      "streams_unfinished": int((flags & capi.FINISH_UNFINISHED).astype(bool).sum()),
                      "streams_empty": int((flags & capi.FINISH_EMPTY).astype(bool).sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteomes", type=int, default=64)
    ap.add_argument("--residues", type=int, default=1_500_000)
    ap.add_argument("--records", type=int, default=4000)
    ap.add_argument("--contigs", type=int, default=40)
    ap.add_argument("--proteins", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-cli", action="store_true", help="no child processes")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = capi.Context(0)
    n, length = a.proteomes, a.residues

    # (a) proteomes: codes 1..20, a separator after each of the records
    prot = rng.integers(1, 21, size=n * length, dtype=np.uint8)
    for s in range(n):
        ends = np.sort(rng.choice(length - 1, a.records - 1, replace=False))
        prot[s * length + ends] = 0
        prot[(s + 1) * length - 1] = 0
    begin_a = np.arange(n + 1, dtype=np.uint64) * length
    shape_bench(ctx, "(a) proteomes", lambda: capi.sketch_signs_aa(ctx, prot, begin_a, [7], BINS, 1, False),
                lambda: capi.sketch_usigs_aa(ctx, prot, begin_a, [7], BINS, 1, False), n, a.repeats, samples=n, residues_per_sample=length)

    # (c) a DNA assembly batch
    codes = rng.integers(0, 4, size=n * length, dtype=np.uint8)
    offs = np.concatenate([np.sort(rng.choice(length, a.contigs - 1, replace=False)).tolist() + [length] for _ in range(n)])
    offset_begin = np.arange(n + 1, dtype=np.uint64) * a.contigs
    packed = capi.pack_codes(codes, begin_a)
    del codes
    shape_bench(ctx, "(c) DNA assemblies", lambda: capi.sketch_signs_packed(ctx, packed, begin_a, offs, offset_begin, [17], BINS, True),
                lambda: capi.sketch_usigs_packed(ctx, packed, begin_a, offs, offset_begin, [17], BINS, True), n, a.repeats, samples=n,
                bases_per_sample=length)
    del packed

    # (b) single proteins
    m = a.proteins
    lengths = np.clip(rng.lognormal(np.log(300.0), 0.6, size=m), 50, 2000).astype(np.uint64)
    begin_b = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    singles = rng.integers(1, 21, size=int(begin_b[-1]), dtype=np.uint8)
    shape_bench(ctx, "(b) single proteins", lambda: capi.sketch_signs_aa(ctx, singles, begin_b, [7], BINS, 1, True),
                lambda: capi.sketch_usigs_aa(ctx, singles, begin_b, [7], BINS, 1, True), m, a.repeats, samples=m, residues=int(begin_b[-1]),
                sign_bytes=m * BINS * 8, usig_bytes=m * BINS // 64 * 14 * 8)
    ctx.close()
    if a.no_cli:
        return

    # end to end through the CLI
    letters = np.frombuffer(b"*ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for s in range(n):
            path = os.path.join(tmp, f"p{s}.fa")
            seq = letters[prot[s * length:(s + 1) * length]]
            with open(path, "wb") as f:
                start = 0
                for end in np.flatnonzero(seq == ord("*")):
                    f.write(b">r\n" + seq[start:end].tobytes() + b"\n")
                    start = end + 1
            files.append(path)
        single_path = os.path.join(tmp, "singles.fa")
        with open(single_path, "wb") as f:
            seq = letters[singles]
            for i in range(m):
                f.write(b">p\n" + seq[int(begin_b[i]):int(begin_b[i + 1])].tobytes() + b"\n")
        runs = (("cpu --threads 16", ["--threads", "16"], {}), ("gpu --threads 16", ["--gpu", "--threads", "16"], {}),
                ("gpu --threads 16, SKL_SKETCH_FINISH=host", ["--gpu", "--threads", "16"], {"SKL_SKETCH_FINISH": "host"}))
        for shape, inputs, extra_shape, residues in (("(a) proteomes", files, [], n * length),
                                                     ("(b) single proteins", [single_path], ["--concat-fasta"], int(begin_b[-1]))):
            out = {}
            for label, extra, env in runs:
                prefix = os.path.join(tmp, "db")
                t0 = time.perf_counter()
                res = subprocess.run([CLI, "sketch", "-o", prefix, "--seq-type", "aa", "-k", "7", "-s", str(BINS), *extra_shape, *extra, *inputs],
                                     env={**os.environ, "SKL_CLI_TIMING": "1", **env}, capture_output=True, text=True, check=True)
                wall = time.perf_counter() - t0
                out[label] = open(prefix + ".skd", "rb").read()
                print(json.dumps({"mode": f"{shape}: sketchlib sketch --seq-type aa end to end, {label}", "residues": residues, "wall_s": wall,
                                  "Mresidues_per_s": residues / wall / 1e6,
                                  "timing": [ln for ln in res.stderr.splitlines() if ln.startswith("TIMING")]}), flush=True)
            print(json.dumps({"shape": shape, "skd_identical": len(set(out.values())) == 1}), flush=True)


if __name__ == "__main__":
    main()
