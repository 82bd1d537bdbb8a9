#!/usr/bin/env python3
"""Amino-acid sketching on one MI355X, two workload shapes through skl_sketch_signs_aa:

  (a) proteomes: 64 samples of 1.5 M residues in 4 000 records each (the staged kernel);
  (b) single proteins: 1 M samples of log-normal length around 300, `--concat-fasta` semantics (the unstaged kernel, a
      thread per span of 16 window starts, samples packed into workgroups).

For both: the kernels alone (HIP events around the launches) and the whole call (upload, kernels, the signs' way back), at
k = 7 and 1 024 bins.  The yardstick is the DNA kernel on single-strand input of shape (a) at the same k and bins
(skl_sketch_signs_packed, rc = 0): it rolls one hash per window from 2-bit codes.  Then `sketchlib sketch --seq-type aa` end to
end on FASTA files of both shapes, CPU path at --threads 16 against --gpu.

    bench_sketch_aa.py [--proteomes 64] [--residues 1500000] [--proteins 1000000] [--kernel-only]"""
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
K, BINS = 7, 1024


def timed(ctx, call, windows, label, **more):
    call()                                   # (the first call of a size grows the context's buffers)
    ctx.timing_enable()
    best = None
    for _ in range(3):
        ctx.timing_reset()
        t0 = time.perf_counter()
        call()
        wall = time.perf_counter() - t0
        kms, launches = ctx.kernel_ms()
        if best is None or wall < best[0]:
            best = (wall, kms, launches)
    ctx.timing_enable(0)
    wall, kms, launches = best
    print(json.dumps({"mode": label, "k": K, "num_bins": BINS, "windows": windows, "kernel_ms": kms, "kernel_launches": launches,
                      "kernel_Gwindows_per_s": windows / kms / 1e6, "call_wall_s": wall,
                      "call_fraction_outside_kernels": 1.0 - kms / 1e3 / wall, "kernel": ctx.last_kernel(), **more}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteomes", type=int, default=64)
    ap.add_argument("--residues", type=int, default=1_500_000)
    ap.add_argument("--records", type=int, default=4000)
    ap.add_argument("--proteins", type=int, default=1_000_000)
    ap.add_argument("--kernel-only", action="store_true", help="no child processes (profiling runs)")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ctx = capi.Context(0)

    # (a) proteomes: codes 1..20, a separator after each of the records
    n, length = a.proteomes, a.residues
    prot = rng.integers(1, 21, size=n * length, dtype=np.uint8)
    for s in range(n):
        ends = np.sort(rng.choice(length - 1, a.records - 1, replace=False))
        prot[s * length + ends] = 0
        prot[(s + 1) * length - 1] = 0
    begin_a = np.arange(n + 1, dtype=np.uint64) * length
    timed(ctx, lambda: capi.sketch_signs_aa(ctx, prot, begin_a, [K], BINS, 1, False), n * length,
          "(a) proteomes, skl_sketch_signs_aa", samples=n, residues_per_sample=length, records_per_sample=a.records)

    # the yardstick: DNA, single strand, the same sample lengths
    codes = rng.integers(0, 4, size=n * length, dtype=np.uint8)
    offs = np.concatenate([np.sort(rng.choice(length, a.records - 1, replace=False)).tolist() + [length] for _ in range(n)])
    offset_begin = np.arange(n + 1, dtype=np.uint64) * a.records
    packed = capi.pack_codes(codes, begin_a)
    timed(ctx, lambda: capi.sketch_signs_packed(ctx, packed, begin_a, offs, offset_begin, [K], BINS, False), n * length,
          "yardstick: DNA single strand, skl_sketch_signs_packed", samples=n, bases_per_sample=length, records_per_sample=a.records)
    del codes, packed

    # (b) single proteins
    m = a.proteins
    lengths = np.clip(rng.lognormal(np.log(300.0), 0.6, size=m), 50, 2000).astype(np.uint64)
    begin_b = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    singles = rng.integers(1, 21, size=int(begin_b[-1]), dtype=np.uint8)
    timed(ctx, lambda: capi.sketch_signs_aa(ctx, singles, begin_b, [K], BINS, 1, True), int(begin_b[-1]),
          "(b) single proteins, skl_sketch_signs_aa", samples=m, residues=int(begin_b[-1]), sign_bytes=m * BINS * 8)
    if a.kernel_only:
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
        for shape, inputs, extra_shape, residues in (("(a) proteomes", files, [], n * length),
                                                     ("(b) single proteins", [single_path], ["--concat-fasta"], int(begin_b[-1]))):
            out = {}
            for label, extra in (("cpu --threads 16", ["--threads", "16"]), ("gpu --threads 16", ["--gpu", "--threads", "16"])):
                prefix = os.path.join(tmp, "db_" + label.split()[0])
                t0 = time.perf_counter()
                subprocess.check_call([CLI, "sketch", "-o", prefix, "--seq-type", "aa", "-k", str(K), "-s", str(BINS), *extra_shape,
                                       *extra, *inputs], env={**os.environ, "SKL_CLI_TIMING": "1"})
                wall = time.perf_counter() - t0
                out[label] = open(prefix + ".skd", "rb").read()
                print(json.dumps({"mode": f"{shape}: sketchlib sketch --seq-type aa end to end, {label}", "residues": residues,
                                  "wall_s": wall, "Mresidues_per_s": residues / wall / 1e6}), flush=True)
            print(json.dumps({"shape": shape, "skd_identical_cpu_vs_gpu": out["cpu --threads 16"] == out["gpu --threads 16"]}), flush=True)


if __name__ == "__main__":
    main()
