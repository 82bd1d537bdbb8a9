#!/usr/bin/env python3
"""`sketchlib inverted build` and `inverted query` end to end on synthetic assemblies, CPU sketching at --threads 16 against
--gpu of the same build (the u16 finish): N random genomes of about 2 Mb in a few contigs each, written as
plain FASTA, at -s 1000 -k 21.  Every figure comes from a run of its own (a fresh process per command and repetition); the
phases are the commands' own `TIMING inverted build:` / `TIMING inverted query:` lines (SKL_CLI_TIMING=1), the wall time is
the process's.  Writes a Markdown table (default profiles/inverted_sketch.md) and prints one JSON line per run.

    bench_inverted_sketch.py [--samples 256] [--bases 2000000] [--reps 3] [--out profiles/inverted_sketch.md]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")
K, S = 21, 1000


def write_assemblies(tmp, n, bases, rng):
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    names, total = [], 0
    for s in range(n):
        length = int(bases * rng.uniform(0.9, 1.1))
        seq = letters[rng.integers(0, 4, size=length, dtype=np.uint8)]
        cuts = [0] + sorted(rng.choice(length - 1, size=int(rng.integers(5, 40)), replace=False).tolist()) + [length]
        path = os.path.join(tmp, f"g{s:04d}.fa")
        with open(path, "wb") as f:
            for c in range(len(cuts) - 1):
                f.write(b">contig%d\n" % c + seq[cuts[c]:cuts[c + 1]].tobytes() + b"\n")
        names.append(path)
        total += length
    rfile = os.path.join(tmp, "rfile.txt")
    with open(rfile, "w") as f:
        f.writelines(f"g{s:04d}\t{p}\n" for s, p in enumerate(names))
    return rfile, total


def timed_run(args, tag):
    t0 = time.perf_counter()
    res = subprocess.run([CLI, *args], capture_output=True, text=True, env={**os.environ, "SKL_CLI_TIMING": "1"})
    wall = time.perf_counter() - t0
    if res.returncode != 0:
        raise SystemExit(f"{tag} failed:\n{res.stderr}")
    line = next(l for l in res.stderr.splitlines() if l.startswith("TIMING inverted"))
    phases = {m.group(1): float(m.group(2)) for m in re.finditer(r"(\w+)=([0-9.]+)s", line)}
    print(json.dumps({"run": tag, "wall_s": wall, **phases}), flush=True)
    return wall, phases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--bases", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inverted_sketch.md"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        rfile, total_bases = write_assemblies(tmp, a.samples, a.bases, rng)
        print(json.dumps({"samples": a.samples, "total_bases": total_bases}), flush=True)
        paths = {"cpu": ["--threads", "16"], "gpu": ["--gpu", "--threads", "16"]}
        for command in ("build", "query"):
            for tag, extra in paths.items():
                runs = []
                for rep in range(a.reps):
                    prefix = os.path.join(tmp, f"idx_{tag}")
                    if command == "build":
                        args = ["inverted", "build", "-o", prefix, "--write-skq", "-k", str(K), "-s", str(S), "-f", rfile, *extra]
                    else:
                        args = ["inverted", "query", prefix + ".ski", "-f", rfile, "-o", os.path.join(tmp, f"q_{tag}.txt"), *extra]
                    runs.append(timed_run(args, f"inverted {command} {tag} rep {rep}"))
                rows.append((command, tag, runs))
        same_skq = open(os.path.join(tmp, "idx_cpu.skq"), "rb").read() == open(os.path.join(tmp, "idx_gpu.skq"), "rb").read()
        same_ski = open(os.path.join(tmp, "idx_cpu.ski"), "rb").read() == open(os.path.join(tmp, "idx_gpu.ski"), "rb").read()
        same_query = open(os.path.join(tmp, "q_cpu.txt"), "rb").read() == open(os.path.join(tmp, "q_gpu.txt"), "rb").read()
    print(json.dumps({"skq_identical": same_skq, "ski_identical": same_ski, "query_output_identical": same_query}), flush=True)

    lines = ["# `inverted build` / `inverted query`: CPU sketching against `--gpu`", "",
             f"`scripts/bench_inverted_sketch.py --samples {a.samples} --bases {a.bases} --reps {a.reps}` on one MI355X host: {a.samples} synthetic",
             f"assemblies of about {a.bases / 1e6:.1f} Mb ({total_bases / 1e6:.0f} Mb in all; plain FASTA, 5-40 contigs), `-k {K} -s {S}`, the CPU path at `--threads 16` and the `--gpu`",
             "path of the same build (also `--threads 16` for parsing and packing).  Every row is a process of its own; the phases are",
             "the command's `TIMING` line, `wall` is the process from start to exit.  Seconds; median of the repetitions first, then each.", "",
             f"Outputs identical between the two paths: `.skq` {same_skq}, `.ski` {same_ski}, query listing {same_query}.", ""]
    for command, tag, runs in rows:
        keys = list(runs[0][1])
        lines.append(f"## inverted {command}, {'CPU --threads 16' if tag == 'cpu' else '--gpu --threads 16'}")
        lines.append("")
        lines.append("| | wall | " + " | ".join(keys) + " |")
        lines.append("|---|---|" + "---|" * len(keys))
        lines.append("| median | %.3f | " % statistics.median(w for w, _ in runs) + " | ".join("%.3f" % statistics.median(p[k] for _, p in runs) for k in keys) + " |")
        for rep, (wall, phases) in enumerate(runs):
            lines.append(f"| run {rep} | {wall:.3f} | " + " | ".join("%.3f" % phases[k] for k in keys) + " |")
        lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
