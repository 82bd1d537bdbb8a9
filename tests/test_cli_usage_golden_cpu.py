"""What the CLI answers to arguments that end in its parser -- exit code, stdout and stderr -- byte for byte as recorded in
tests/golden/generated/cli_usage.json (tests/golden/make_cli_usage_golden.py, recorded from the CLI before its commands
were split over one argument reader).  No vector opens a file or needs a device."""
import json
import os
import re

import pytest

from conftest import ROOT

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "_build", "sketchlib")
GOLDEN = os.path.join(GOLDEN_DIR, "generated", "cli_usage.json")
MAIN = os.path.join(ROOT, "sketchlib.rust_amd", "csrc", "host", "cli", "main.cpp")
GLOBAL_FLAGS = ("-v", "--verbose", "--quiet")


@pytest.fixture(scope="module", autouse=True)
def _built(skl):
    assert os.path.exists(CLI)


def records():
    with open(GOLDEN) as f:
        return json.load(f)


def recorder():
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_cli_usage_golden", os.path.join(GOLDEN_DIR, "make_cli_usage_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_record_is_the_recorders_corpus():
    assert [r["argv"] for r in records()] == recorder().corpus()
    assert all(r["code"] in (0, 2) for r in records())


def test_every_vector_answers_as_recorded(tmp_path):
    from concurrent.futures import ThreadPoolExecutor

    answer = recorder().answer
    with ThreadPoolExecutor(4) as pool:      # (processes that end in their parser: a few at a time)
        answers = list(pool.map(lambda want: answer(CLI, want["argv"], tmp_path), records()))
    wrong = [(want, got) for want, got in zip(records(), answers) if got != want]
    assert os.listdir(tmp_path) == []          # nothing was written
    assert not wrong, f"{len(wrong)} of {len(records())} differ; the first: want {wrong[0][0]} got {wrong[0][1]}"


def test_every_command_of_the_table_has_vectors():
    """A command added to main.cpp's table without vectors in the corpus fails here."""
    table = re.search(r"const CommandEntry COMMANDS\[\] = \{\n(.*?)\n\};", open(MAIN).read(), re.S).group(1)
    commands = re.findall(r'^\s*\{"([a-z]+)", (?:"([a-z]+)"|nullptr),', table, re.M)
    assert len(commands) == len(table.splitlines()) >= 10, table
    assert ("dist", "") in commands and ("inverted", "query") in commands
    vectors = []
    for r in records():
        argv = list(r["argv"])
        while argv and argv[0] in GLOBAL_FLAGS:
            argv.pop(0)
        vectors.append(argv)
    for name, sub in commands:
        prefix = [name, sub] if sub else [name]
        mine = [v for v in vectors if v[:len(prefix)] == prefix]
        assert len(mine) >= 1, prefix
        if sub or name != "inverted":       # (`inverted` without a subcommand of its own has its few vectors)
            assert len(mine) >= 5 and any(len(v) == len(prefix) for v in mine), prefix   # the bare command among them
