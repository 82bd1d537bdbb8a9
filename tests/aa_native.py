"""Builds tests/native/aa_check.cpp -- the amino-acid sketcher's host code and the work plan of its GPU call behind a main()
of their own -- once per test session and flavour, with the host compiler alone (no ROCm include path, no library)."""
import functools
import glob
import os
import subprocess
import tempfile

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "aa_check.cpp")
HOST = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "host")
# the host layer (the CLI lies in host/cli/) without the two files that call the GPU library (the Makefile's HOST_LIB_SRC)
HOST_SRC = sorted(f for f in glob.glob(os.path.join(HOST, "*.cpp"))
                  if os.path.basename(f) not in ("distances.cpp", "sketch_gpu.cpp"))
_DIR = tempfile.TemporaryDirectory(prefix="aa_check_")


@functools.lru_cache(maxsize=None)
def build(sanitize=False):
    """Path of the program; sanitize=True: the same sources under AddressSanitizer and UndefinedBehaviorSanitizer."""
    exe = os.path.join(_DIR.name, "aa_check_san" if sanitize else "aa_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, *HOST_SRC, "-lz", "-lpthread", "-o", exe])
    return exe
