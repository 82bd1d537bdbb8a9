"""csrc/nthash.hpp and csrc/sketch_plan.hpp on the CPU.  The first holds the arithmetic the three sketch kernels share with the
host -- the split rotation, the ntHash seeds and top tables, `% SIGN_MOD`, the bin of a sign, the 2-bit packer -- the second
how the DNA sketching calls deal window starts to threads and samples to upload batches, the read-survivor span table, and the
one close-before cutter behind aa_batches and the five batch loops of host/sketch_gpu.cpp.  tests/native/sketch_plan_check.cpp
includes the two headers alone and checks each against the obvious slow form or against values worked out by hand; among them
both corrections of bin_of, of which no GPU input reaches `++bin`.  Built with the host compiler alone, a second time under
AddressSanitizer and UndefinedBehaviorSanitizer (a program with a main() of its own; any report ends it with a non-zero
status); nothing here is loaded into Python."""
import functools
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "sketch_plan_check.cpp")
SECTIONS = ["mod_sign", "bin_of", "hash", "pack", "plan", "upload", "cutter", "spans"]
_DIR = tempfile.TemporaryDirectory(prefix="sketch_plan_check_")


@functools.lru_cache(maxsize=None)
def build(sanitize):
    exe = os.path.join(_DIR.name, "sketch_plan_check_san" if sanitize else "sketch_plan_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
@pytest.mark.parametrize("section", SECTIONS)
def test_section(section, sanitize):
    res = subprocess.run([build(sanitize), section], capture_output=True, text=True)
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr
    assert res.returncode == 0 and res.stdout.splitlines()[-1].startswith("ok " + section), res.stdout + res.stderr


def test_both_bin_corrections_fire():
    """The `--bin` and the `++bin` branch of bin_of are both taken on the edge signs, and the estimate is off in both
    directions at 100 032 bins (the program itself requires what holds at the other bin counts, and says why)."""
    out = subprocess.run([build(False), "bin_of"], capture_output=True, text=True, check=True).stdout.splitlines()
    rows = {int(r.split()[1]): dict(zip(r.split()[2::2], map(int, r.split()[3::2]))) for r in out if r.startswith("bins ")}
    assert sorted(rows) == [1, 63, 64, 1000, 4096, 4097, 100032, 1 << 20]
    assert rows[100032]["over"] > 0 and rows[100032]["under"] > 0
    assert all(rows[nb]["over"] > 0 for nb in rows if nb > 1)
    _ok, _name, dec, inc = out[-1].split()
    assert int(dec) > 0 and int(inc) > 0
