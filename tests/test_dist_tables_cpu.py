"""csrc/dist_tables.hpp holds the arithmetic behind bit-parity -- bin matches -> Jaccard index, ln J with the early break's
`min_alive`, the single-k distance / ANI tables -- as pure functions; the library only uploads what they return.
tests/native/dist_tables_check.cpp includes the header alone (host compiler, no ROCm include path, -ffp-contract=off as the
library is built) and checks, at sketch sizes of 1, 2, 16, 64 and 1 024 chunks of 64 bins (one chunk ... the u16 limit; 256 is
the first size at which two unrelated sketches are expected to share a bin): the tables' sizes, -inf at or below the chance
level, `min_alive` as the first count not below the tolerance with none below it afterwards, distance = 1 - J, ANI clamped at
0 -- and every entry, bit for bit, against the oracle's C restatement of the reference (oracle/sketchlib_oracle.c, which
tests/test_oracle_golden.py holds to the fixtures recorded from the reference)."""
import os
import subprocess

from conftest import ROOT

SIZES = [1, 2, 16, 64, 256, 1024]


def test_tables_hold_their_properties_and_equal_the_oracle(tmp_path):
    oracle_o, exe = str(tmp_path / "oracle.o"), str(tmp_path / "dist_tables_check")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-c", os.path.join(ROOT, "oracle", "sketchlib_oracle.c"), "-o", oracle_o])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "native", "dist_tables_check.cpp"), oracle_o, "-lm", "-lpthread", "-o", exe])
    res = subprocess.run([exe] + [str(s) for s in SIZES], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout[-4000:] + res.stderr
    # per size 64 * ss64 + 1 counts, each checked in the ln J table (4 checks), the distance table and three ANI tables
    assert int(res.stdout.split()[1]) >= sum(64 * s + 1 for s in SIZES) * 8
