#!/usr/bin/env python3
"""Records tests/golden/generated/cli_usage.json: what the CLI answers to argument vectors that end in its parser.

    python tests/golden/make_cli_usage_golden.py <path of a sketchlib CLI binary>

Every vector of CORPUS ends before a file is opened or a device is touched: exit code 2 (usage) or 0 (help).  The
record holds argv, exit code, stdout and stderr; tests/test_cli_usage_golden_cpu.py compares the built CLI with it byte
for byte.  A change of the accepted syntax is made on purpose: re-record with the new binary and review the diff.

(No vector combines a global -v with a command that ends by RETURNING 2, such as `inverted search`: main() then prints
"Complete in <seconds>s", which no record can hold.)"""
import json
import os
import subprocess
import sys
import tempfile

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "generated", "cli_usage.json")
BIG = "99999999999999999999999"   # 23 digits


def last_without_value(cmd, flags, before=()):
    return [[*cmd, *before, f] for f in flags]


def bad_values(cmd, flag, values, before=()):
    return [[*cmd, *before, flag, v] for v in values]


def corpus():
    c = [
        [], ["--help"], ["-h"], ["-v", "--quiet"], ["-v", "--quiet", "--help"], ["-v", "--quiet", "dist"],
        ["--verbose", "sketch"], ["--quiet", "info"], ["frobnicate"], ["-x", "dist"],
        ["inverted"], ["inverted", "search"], ["inverted", "--help"], ["--quiet", "inverted"],
    ]
    # ---- dist ----
    d = ["dist"]
    c += [d, d + ["--help"], d + ["-h"], d + ["a", "--help"], d + ["a", "b", "c"], d + ["--frob", "a"], d + ["-x", "a"],
          d + ["--frob=1", "a"], d + ["-v", "--quiet"]]
    c += last_without_value(d, ["-o", "--knn", "--knn-ties", "--subset", "--pairs", "-k", "--threads", "--ref-completeness-file",
                                "--query-completeness-file", "--completeness-cutoff", "--device", "--band-mb", "--gpus",
                                "--devices"], before=["a"])
    for flag in ("--knn", "-k", "--device", "--band-mb"):
        c += bad_values(d, flag, ["x", "-3", "", "3.5", BIG])
    c += bad_values(d, "--gpus", ["x", "-3", "", "3.5", "0", "1"])   # (not BIG: a device list of that length is built first)
    c += bad_values(d, "--devices", ["0,,1", "x", "0,1,", "-1", "0,1"])
    c += bad_values(d, "--threads", ["0", "x", "-1", "", "1x", BIG, "2"])
    c += bad_values(d, "--completeness-cutoff", ["x", "", "0.5x", "0.5"])
    c += bad_values(d, "--knn-ties", ["lowest", "", "canonical"])
    c += [d + ["--ani", "a"], d + ["--npy", "a"], d + ["--npy", "-o", "x", "--knn", "3", "a"]]
    for other in (["--knn", "3"], ["--subset", "s"], ["--npy"], ["--gpus", "2"], ["--devices", "0,1"]):
        c += [d + ["--pairs", "p", *other, "a"], d + [*other, "--pairs", "p", "a"]]
    c += [d + ["--knn=x"], d + ["--knn="], d + ["--knn=5"], d + ["-kx"], d + ["-k21"], d + ["-ofile"], d + ["--threads=0"],
          d + ["--knn-ties=x"], d + ["--ani=1", "a"], d + ["--devices=0,,1"], d + ["-k"], d + ["-k="]]
    # ---- sketch ----
    s = ["sketch"]
    c += [s, s + ["--help"], s + ["-h"], s + ["-o", "x"], s + ["-o", "x", "f.fa"], s + ["--k-vals", "21", "f.fa"],
          s + ["-o", "x", "-f", "l", "f.fa"], s + ["-o", "x", "-f", "l"],
          s + ["-o", "x", "f.fa", "--k-vals", "21", "--k-seq", "17,31,4"], s + ["--frob"], s + ["-o", "x", "f.fa", "-x"],
          s + ["--k-vals=21"], s + ["-ox"], s + ["-k21"], s + ["--threads", "0"], s + ["--gpu"], s + ["--single-strand"]]
    c += last_without_value(s, ["-f", "-o", "-k", "--k-vals", "--k-seq", "-s", "--sketch-size", "--threads", "--device",
                                "--seq-type", "--min-count", "--min-qual", "--level"])
    for flag in ("--k-vals", "-k", "--k-seq", "-s", "--sketch-size", "--threads", "--device"):
        c += bad_values(s, flag, ["x", "-1", "", BIG])
    c += bad_values(s, "--k-vals", ["21,,31", "21,", ",21", "21,x"])
    c += bad_values(s, "--min-count", ["x", "-1", "", "65535", "65536", BIG])
    c += bad_values(s, "--min-qual", ["x", "-1", "", "255", "256", BIG])
    c += bad_values(s, "--seq-type", ["rna", "pdb", "aa", ""])
    c += bad_values(s, "--level", ["level4", "2", "level2", ""])
    # ---- merge / delete / info ----
    m = ["merge"]
    c += [m, m + ["--help"], m + ["-h"], m + ["a"], m + ["-o", "x"], m + ["-o", "x", "a"], m + ["a", "b"],
          m + ["-o", "x", "a", "b", "c"], m + ["a", "b", "c"], m + ["--frob"], m + ["-o"], m + ["-ox"], m + ["-ox", "a"],
          m + ["-ox", "a", "b", "c"], m + ["-v", "--verbose", "--quiet"], m + ["--output=x", "a", "b"]]
    x = ["delete"]
    c += [x, x + ["--help"], x + ["-h"], x + ["a"], x + ["a", "b"], x + ["a", "b", "c", "d"], x + ["--frob"],
          x + ["a", "b", "-o", "c"], x + ["-v", "a"]]
    i = ["info"]
    c += [i, i + ["--help"], i + ["-h"], i + ["a", "b"], i + ["--frob"], i + ["--sample-info"], i + ["--quiet"],
          i + ["--sample-info=1", "a"]]
    # ---- append ----
    a = ["append"]
    c += [a, a + ["--help"], a + ["-h"], a + ["-o", "x"], a + ["db", "f.fa"], a + ["-o", "x", "db"],
          a + ["-o", "x", "db", "-f", "l", "f.fa"], a + ["--frob"], a + ["-ox"], a + ["--threads=2"], a + ["--k-vals", "21"],
          a + ["--threads", "0"]]
    c += last_without_value(a, ["-f", "-o", "--min-count", "--min-qual", "--threads", "--device", "--level"])
    c += bad_values(a, "--min-count", ["x", "-1", "65535", "65536", BIG])
    c += bad_values(a, "--min-qual", ["x", "-1", "255", "256", BIG])
    c += bad_values(a, "--threads", ["x", "-1", BIG])
    c += bad_values(a, "--device", ["x", "-1", BIG])
    c += bad_values(a, "--level", ["level0", "level3"])
    # ---- inverted build ----
    b = ["inverted", "build"]
    c += [b, b + ["--help"], b + ["-h"], b + ["f.fa"], b + ["-o", "x"], b + ["-o", "x", "-f", "l", "f.fa"], b + ["--frob"],
          b + ["-ox"], b + ["--kmer-length=21"], b + ["--threads", "0"], b + ["--write-skq"], b + ["--k-vals", "21"]]
    c += last_without_value(b, ["-f", "-o", "--species-names", "--metadata", "-s", "--sketch-size", "-k", "--kmer-length",
                                "--threads", "--min-count", "--min-qual", "--device"])
    for flag in ("-s", "--sketch-size", "-k", "--kmer-length", "--threads", "--device"):
        c += bad_values(b, flag, ["x", "-1", BIG])
    c += bad_values(b, "--min-count", ["x", "-1", "65535", "65536", BIG])
    c += bad_values(b, "--min-qual", ["x", "-1", "255", "256", BIG])
    # ---- inverted query ----
    q = ["inverted", "query"]
    c += [q, q + ["--help"], q + ["-h"], q + ["-f", "l"], q + ["i.ski"], q + ["i.ski", "-f", "l", "f.fa"], q + ["--frob"],
          q + ["-ox"], q + ["--top=3"], q + ["--single-strand"], q + ["--threads", "0"], q + ["--gpu"],
          q + ["--top", "3", "--query-type", "all-bins"], q + ["--query-type", "any-bins", "--top", "3", "i.ski", "f.fa"],
          q + ["--top", "3", "--query-type", "match-count"]]
    c += last_without_value(q, ["-f", "-o", "--top", "--query-type", "--threads", "--min-count", "--min-qual", "--device"])
    c += bad_values(q, "--top", ["x", "-3", "", "3.5", "0", "1", "1024", "1025", BIG])
    c += bad_values(q, "--query-type", ["some-bins", "", "all-bins"])
    c += bad_values(q, "--threads", ["x", "-1", BIG])
    c += bad_values(q, "--device", ["x", "-1", BIG])
    c += bad_values(q, "--min-count", ["x", "-1", "65535", "65536", BIG])
    c += bad_values(q, "--min-qual", ["x", "-1", "255", "256", BIG])
    # ---- inverted precluster ----
    p = ["inverted", "precluster"]
    c += [p, p + ["--help"], p + ["-h"], p + ["a.ski", "b.ski"], p + ["--frob"], p + ["-ox"], p + ["--knn=3"],
          p + ["a.ski", "--count", "--skd", "d"], p + ["--count", "--skd", "d"], p + ["--threads", "0"],
          p + ["--completeness-cutoff", "x"], p + ["--count"], p + ["--retain-unmatched", "all"]]
    c += last_without_value(p, ["--skd", "-o", "--knn", "--threads", "--ref-completeness-file", "--completeness-cutoff",
                                "--retain-unmatched", "--device", "--knn-ties"])
    for flag in ("--knn", "--threads", "--device"):
        c += bad_values(p, flag, ["x", "-1", BIG])
    c += bad_values(p, "--knn-ties", ["lowest", "reference"])
    c += bad_values(p, "--retain-unmatched", ["all", "", "singleton"], before=["a.ski", "--count", "--skd", "d"])
    c += bad_values(p, "--retain-unmatched", ["all", ""], before=["a.ski"])
    seen, out = set(), []
    for argv in c:
        if tuple(argv) not in seen:
            seen.add(tuple(argv))
            out.append(argv)
    return out


def answer(cli, argv, cwd):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SKL_")}
    res = subprocess.run([cli, *argv], cwd=cwd, env=env, stdin=subprocess.DEVNULL, capture_output=True, timeout=60)
    return {"argv": argv, "code": res.returncode, "stdout": res.stdout.decode(), "stderr": res.stderr.decode()}


def main():
    cli = os.path.abspath(sys.argv[1])
    with tempfile.TemporaryDirectory(prefix="cli_usage_") as cwd:   # an empty directory: no vector may find a file
        records = [answer(cli, argv, cwd) for argv in corpus()]
        assert os.listdir(cwd) == [], "a vector wrote a file: " + str(os.listdir(cwd))
    for r in records:
        assert r["code"] in (0, 2), r
    with open(OUT, "w") as f:
        json.dump(records, f, indent=0, ensure_ascii=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(records)} vectors, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
