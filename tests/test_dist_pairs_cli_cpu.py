"""`sketchlib dist --pairs <FILE>` without a GPU: the pairs-file parser and name lookup (csrc/host/pairs_file.cpp), the
listing writer (write_pair_list) and the flag conflicts the CLI refuses before it touches a device.

The parser reads untrusted input, so tests/native/pairs_file_check.cpp -- a stand-alone host program -- is built with
-fsanitize=address,undefined and every case below runs through that build: a report from either sanitizer fails the test.
Decisions pinned here: a CR LF line end is TOLERATED (the CR is dropped, as --subset files have it); a line without a second
column, or with an empty name, is an error."""
import os
import subprocess

import pytest

from conftest import ROOT
from helpers import rust_f32

HOST = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "host")
NAMES = ["alpha", "beta gamma", "delta#3.fa.gz", "épsilon", "alpha2"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pairs_file") / "pairs_file_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-Wall",
                           "-Wextra", "-Werror", "-I" + HOST, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "pairs_file_check.cpp"), os.path.join(HOST, "pairs_file.cpp"),
                           os.path.join(HOST, "distance_matrix.cpp"), "-lpthread", "-o", exe])
    return exe


def run(exe, tmp_path, content, names=NAMES, second=None, mode="parse", extra=()):
    pairs = tmp_path / "pairs.txt"
    pairs.write_bytes(content if isinstance(content, bytes) else content.encode())
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))
    args = [exe, mode, str(pairs), str(tmp_path / "names.txt")]
    if second is not None:
        (tmp_path / "second.txt").write_text("".join(n + "\n" for n in second))
        args.append(str(tmp_path / "second.txt"))
    res = subprocess.run(args + list(extra), capture_output=True, timeout=120)
    err = res.stderr.decode("utf-8", "replace")
    assert "Sanitizer" not in err and "runtime error:" not in err, err[-3000:]
    assert res.returncode in (0, 1), (res.returncode, err[-2000:])
    return res.returncode, res.stdout.decode("utf-8", "replace"), err


def parsed(out):
    lines = out.splitlines()
    assert lines[0] == f"ok {len(lines) - 1}"
    return [tuple(int(v) for v in l.split("\t")) for l in lines[1:]]


def test_order_repeats_and_orientation_are_kept(check, tmp_path):
    rc, out, _ = run(check, tmp_path, "delta#3.fa.gz\talpha\nalpha\tdelta#3.fa.gz\nalpha\talpha\nbeta gamma\tépsilon\nalpha\tdelta#3.fa.gz\n")
    assert rc == 0 and parsed(out) == [(2, 0), (0, 2), (0, 0), (1, 3), (0, 2)]


def test_extra_columns_blank_lines_and_crlf(check, tmp_path):
    text = ("alpha\tbeta gamma\t0.125\t0.5\n"            # the listing of an earlier dist --knn run: distances follow
            "\n"
            "alpha2\talpha\t\t\n"                         # empty further columns
            "\r\n"                                        # blank line with a CR LF end
            "épsilon\tdelta#3.fa.gz\t1\r\n"               # CR LF after a further column
            "beta gamma\talpha2\r\n"                      # CR LF right after the second name: the CR is not part of it
            "\n\n"
            "alpha\talpha2")                              # no newline at the end of the file
    rc, out, _ = run(check, tmp_path, text)
    assert rc == 0 and parsed(out) == [(0, 1), (4, 0), (3, 2), (1, 4), (0, 4)]


def test_empty_file_and_blank_only_file(check, tmp_path):
    for text in ("", "\n\n\r\n"):
        rc, out, _ = run(check, tmp_path, text)
        assert rc == 0 and parsed(out) == []


def test_second_name_is_looked_up_in_the_query_names(check, tmp_path):
    rc, out, _ = run(check, tmp_path, "alpha\tq1\nbeta gamma\tq0\n", second=["q0", "q1", "alpha"])
    assert rc == 0 and parsed(out) == [(0, 1), (1, 0)]
    rc, _, err = run(check, tmp_path, "alpha\tq1\nq0\talpha\n", second=["q0", "q1", "alpha"])    # a query name in the first column
    assert rc == 1 and "line 2" in err and 'sample "q0" is not in the reference database' in err
    rc, _, err = run(check, tmp_path, "alpha\tbeta gamma\n", second=["q0", "q1"])
    assert rc == 1 and "line 1" in err and 'sample "beta gamma" is not in the query database' in err


def test_of_equal_names_the_first_sample_is_meant(check, tmp_path):
    rc, out, _ = run(check, tmp_path, "x\ty\n", names=["y", "x", "x", "y"])
    assert rc == 0 and parsed(out) == [(1, 0)]


def test_error_texts_name_file_line_and_sample(check, tmp_path):
    path = str(tmp_path / "pairs.txt")
    rc, _, err = run(check, tmp_path, "alpha\tbeta gamma\n\nalpha\tnobody\n")
    assert rc == 1 and err.strip() == f'error: {path}: line 3: sample "nobody" is not in the reference database'
    rc, _, err = run(check, tmp_path, "alpha\tbeta gamma\nAlpha\talpha\n")        # names are case-sensitive
    assert rc == 1 and err.strip() == f'error: {path}: line 2: sample "Alpha" is not in the reference database'
    rc, _, err = run(check, tmp_path, "alpha beta\n")                             # a space is not a separator
    assert rc == 1 and err.strip() == f"error: {path}: line 1: expected two tab-separated sample names"
    for bad in ("alpha\n", "alpha\t\n", "\talpha\n", "\t\n", "alpha\t\tbeta gamma\n"):
        rc, _, err = run(check, tmp_path, "alpha\talpha\n" + bad)
        assert rc == 1 and "line 2: expected two tab-separated sample names" in err, bad
    rc, _, err = run(check, tmp_path, "alpha \talpha\n")                          # nothing is trimmed
    assert rc == 1 and 'sample "alpha " is not' in err
    res = subprocess.run([check, "parse", str(tmp_path / "missing.txt"), str(tmp_path / "names.txt")], capture_output=True, text=True)
    assert res.returncode == 1 and "Unable to open" in res.stderr and "missing.txt" in res.stderr


def test_malformed_input_under_the_sanitizers(check, tmp_path):
    """Binary noise, NUL bytes, control characters, a 3 MB line, lone CRs: an error message or a clean parse, never a report."""
    import random

    rnd = random.Random(7)
    noise = bytes(rnd.randrange(256) for _ in range(20000))
    cases = [noise, b"\x00\x00\t\x00\n", b"alpha\x00\talpha\n", b"alpha\talpha\x00junk\n", b"\r\r\r\n", b"\r", b"\t" * 5000,
             b"a" * 3_000_000, b"alpha\t" + b"b" * 3_000_000 + b"\n", b"alpha\talpha\n" * 3 + b"\xff\xfe\t\x80\n",
             b"alpha\talpha\r\r\n", b"\x1b[31malpha\talpha\n"]
    for data in cases:
        rc, _, err = run(check, tmp_path, data)
        if rc == 1:
            assert err.startswith("error: ") and len(err) < 1000, err[:300]     # the message shows at most 200 bytes of a name
            assert "\x1b" not in err and "\x00" not in err                       # and no control characters from the file
    rc, out, _ = run(check, tmp_path, b"alpha\talpha\r\r\n")
    assert rc == 1          # only ONE CR belongs to the line end: "alpha\r" is not a sample
    rc, out, _ = run(check, tmp_path, b"alpha\talpha\x00junk\n")
    assert rc == 1          # a NUL does not end a name


def test_listing_is_in_input_order_for_any_thread_count(check, tmp_path):
    import random

    rnd = random.Random(3)
    pairs = [(rnd.randrange(len(NAMES)), rnd.randrange(len(NAMES))) for _ in range(70_000)]     # three blocks of 32 Ki lines
    text = "".join(f"{NAMES[a]}\t{NAMES[b]}\tignored\n" for a, b in pairs)
    expected = "".join(f"{NAMES[a]}\t{NAMES[b]}\t{rust_f32(x / 4)}\t{rust_f32(x / 8)}\n" for x, (a, b) in enumerate(pairs))
    for threads in ("1", "5"):
        rc, out, _ = run(check, tmp_path, text, mode="list", extra=(threads,))
        assert rc == 0 and out == expected


# ---- the CLI's own checks that need no device ----

CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")


@pytest.mark.parametrize("flags,named", [(("--knn", "3"), "--knn <KNN>"), (("--subset", "s.txt"), "--subset <SUBSET>"),
                                         (("--npy", "-o", "x.npy"), "--npy"), (("--gpus", "2"), "--gpus <N>"),
                                         (("--devices", "0,0"), "--devices <LIST>")])
def test_flags_that_do_not_go_with_pairs_are_usage_errors(skl, flags, named):
    res = subprocess.run([CLI, "dist", "db", "--pairs", "pairs.txt", *flags], capture_output=True, text=True)
    assert res.returncode == 2 and res.stdout == ""
    assert f"error: the argument '--pairs <FILE>' cannot be used with '{named}'" in res.stderr
    assert "Usage: sketchlib dist [OPTIONS] <REF_DB> [QUERY_DB]" in res.stderr


def test_help_lists_the_option(skl):
    res = subprocess.run([CLI, "dist", "--help"], capture_output=True, text=True)
    assert res.returncode == 0 and "--pairs <FILE>" in res.stdout and "name1<TAB>name2" in res.stdout
    res = subprocess.run([CLI, "dist", "db", "--pairs"], capture_output=True, text=True)
    assert res.returncode == 2 and "a value is required for '--pairs <FILE>' but none was supplied" in res.stderr


def test_binding_refuses_lists_it_cannot_pass_on():
    """capi.self_dists_pairs / cross_dists_pairs check their index lists before the C call reads them: unequal lengths, values
    that would wrap in the uint32 conversion and non-integers are ValueErrors (also under `python -O`)."""
    import numpy as np

    from sketchlib.rust_amd import capi

    for a, b in (([0, 1], [1]), ([-1], [0]), ([2 ** 32], [0]), ([0.5], [1]), (np.array([1, 2], dtype=np.int64), np.array([-3, 1]))):
        with pytest.raises(ValueError):
            capi._pair_lists(a, b)
    a, b = capi._pair_lists([], [])
    assert a.dtype == np.uint32 and a.size == 0 and b.size == 0
    a, b = capi._pair_lists(np.arange(3, dtype=np.int64), [2, 1, 2 ** 32 - 1])
    assert a.dtype == np.uint32 and list(b) == [2, 1, 2 ** 32 - 1]
