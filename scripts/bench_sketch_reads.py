#!/usr/bin/env python3
"""`sketchlib sketch` on paired read sets, CPU against --gpu.

Writes --samples synthetic read pairs to a temp dir: a random genome of --genome-mb Mb per sample, 100 bp reads
from both strands at --coverage x, 1 % substitutions, Phred+33 qualities 'I' with 2 % '#'.  Runs the CLI with
SKL_CLI_TIMING=1 at 1 and 5 k-mer lengths (--min-count 5, -s 1000), CPU (--threads T) and --gpu, checks the
two runs wrote the same bytes, and reports per run the wall time; for --gpu also the phases (parse, survivor
kernel calls, replay the kernel did not hide), the survivor fraction of every chunk, and windows/s (window
starts x k-mer lengths over the read path's time).  Prints one JSON line."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")


def write_pair(rng, d, name, genome_bp, coverage, read_len=100):
    genome = rng.integers(0, 4, size=genome_bp, dtype=np.uint8)
    n_reads = coverage * genome_bp // read_len // 2   # per file
    files = []
    for end in (1, 2):
        pos = rng.integers(0, genome_bp - read_len + 1, size=n_reads)
        codes = genome[pos[:, None] + np.arange(read_len)[None, :]]
        flip = rng.random(n_reads) < 0.5
        codes[flip] = (3 - codes[flip])[:, ::-1]
        sub = rng.random(codes.shape) < 0.01
        codes[sub] = rng.integers(0, 4, size=int(sub.sum()), dtype=np.uint8)
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
        qual = np.where(rng.random(codes.shape) < 0.02, ord("#"), ord("I")).astype(np.uint8)
        nl = np.full((n_reads, 1), ord("\n"), dtype=np.uint8)
        head = np.frombuffer(b"@r\n", dtype=np.uint8)[None, :].repeat(n_reads, 0)
        plus = np.frombuffer(b"+\n", dtype=np.uint8)[None, :].repeat(n_reads, 0)
        rec = np.concatenate([head, seq, nl, plus, qual, nl], axis=1)
        path = os.path.join(d, f"{name}_{end}.fastq")
        rec.tofile(path)
        files.append(path)
    return files


def run(args, env_extra, out):
    env = {**os.environ, "SKL_CLI_TIMING": "1", **env_extra}
    t0 = time.perf_counter()
    res = subprocess.run([CLI, "sketch", "-o", out, *args], capture_output=True, text=True, env=env)
    wall = time.perf_counter() - t0
    if res.returncode != 0:
        raise SystemExit(f"sketch failed ({res.returncode}): {res.stderr[-2000:]}")
    return wall, res.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--genome-mb", type=float, default=2.0)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    rng = np.random.default_rng(11)
    result = {"samples": a.samples, "genome_bp": int(a.genome_mb * 1e6), "coverage": a.coverage, "read_len": 100,
              "min_count": 5, "sketch_size": 1000, "threads": a.threads, "runs": []}
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        samples = [write_pair(rng, d, f"s{i}", result["genome_bp"], a.coverage) for i in range(a.samples)]
        result["generate_s"] = round(time.perf_counter() - t0, 2)
        rf = os.path.join(d, "rfile.txt")
        with open(rf, "w") as fh:
            fh.writelines(f"s{i}\t{f[0]}\t{f[1]}\n" for i, f in enumerate(samples))
        for kmers in ("21", "15,19,23,27,31"):
            base = ["-f", rf, "-k", kmers, "-s", "1000", "--min-count", "5", "--threads", str(a.threads)]
            cpu_wall, _ = run(base, {}, os.path.join(d, "cpu"))
            gpu_wall, log = run(base + ["--gpu"], {}, os.path.join(d, "gpu"))
            same = all(open(os.path.join(d, "cpu" + e), "rb").read() == open(os.path.join(d, "gpu" + e), "rb").read()
                       for e in (".skd", ".skm"))
            t = re.search(r"TIMING sketch --gpu: parse=([\d.]+)s", log)
            r = re.search(r"TIMING reads: total=([\d.]+)s survivors_gpu=([\d.]+)s replay_wait=([\d.]+)s chunks=(\d+) "
                          r"window_starts=(\d+) survivors=(\d+)", log)
            chunks = [float(x) for x in re.findall(r"READS chunk \d+: .*\(([\d.e+-]+)\)", log)]
            total, kern, replay, n_chunks, starts, surv = (float(r.group(i)) for i in range(1, 7))
            result["runs"].append({
                "kmers": kmers, "cpu_s": round(cpu_wall, 3), "gpu_s": round(gpu_wall, 3), "identical": same,
                "gpu_parse_s": float(t.group(1)), "gpu_reads_s": total, "gpu_survivor_calls_s": kern,
                "gpu_replay_wait_s": replay, "chunks": int(n_chunks), "window_starts": int(starts),
                "survivors": int(surv), "survivor_fraction": surv / starts if starts else 0.0,
                "survivor_fraction_per_chunk": [round(x, 6) for x in chunks],
                "windows_per_s_reads_path": starts / total if total else 0.0,
            })
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    if not all(r["identical"] for r in result["runs"]):
        sys.exit(1)


if __name__ == "__main__":
    main()
