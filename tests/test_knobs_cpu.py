"""csrc/knobs.def is the one table of the environment switches; csrc/knobs.hpp expands it into `struct Knobs` and into the reader
knobs_from(lookup).  tests/native/knobs_check.cpp includes the header alone, is built with the host compiler (no ROCm include
path) once as the product library sees it and once with -DSKL_AB, and drives the reader through a map: defaults, the empty
string, values inside, below and above every clamp, text that is no number, the word-valued forms and wrong words -- against
expected values written out by hand.  In the product build an A/B-only switch changes nothing, and its name is not in the
product library's bytes."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "native", "knobs_check.cpp")


@pytest.fixture(scope="module")
def checks(tmp_path_factory):
    out = {}
    for build, flags in (("product", []), ("ab", ["-DSKL_AB"])):
        exe = str(tmp_path_factory.mktemp("knobs") / ("knobs_check_" + build))
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe] + flags)
        res = subprocess.run([exe], capture_output=True, text=True)
        out[build] = res
    return out


def _names(res, cls):
    return [l.split()[1] for l in res.stdout.splitlines() if l.startswith(cls + " ")]


@pytest.mark.parametrize("build", ["product", "ab"])
def test_every_switch_reads_as_it_did(checks, build):
    res = checks[build]
    assert res.returncode == 0 and res.stdout.splitlines()[-1].startswith("ok "), res.stdout[-2000:] + res.stderr[-4000:]
    # 53 switches, each with its default, the empty string and at least three texts, twice (the field, and no other field moved)
    assert int(res.stdout.splitlines()[-1].split()[1]) >= 53 * 5 * 2


def test_both_builds_list_the_same_classes(checks):
    for cls in ("product", "ab"):
        assert _names(checks["product"], cls) == _names(checks["ab"], cls)
    product, ab = _names(checks["product"], "product"), _names(checks["product"], "ab")
    assert len(product) == 18 and len(ab) == 35
    assert len(set(product + ab)) == 53 and all(n.startswith("SKL_") for n in product + ab)


def test_product_library_holds_the_product_names_only(checks):
    import sketchlib.rust_amd as pkg

    pkg.build_library()
    blob = open(pkg.library_path(), "rb").read()
    for name in _names(checks["product"], "product"):
        assert name.encode() + b"\0" in blob, name
    for name in _names(checks["product"], "ab"):
        assert name.encode() not in blob, name
