"""`sketchlib inverted query --top N` without a GPU: its argument errors exit 2 with the clap-style message and the usage
line before any device is needed, and a missing .ski is `Error:` and exit 1 as without --top."""
import pytest

from test_inverted_query_cli_cpu import CLI, run, usage_error, wd  # noqa: F401  (wd: the fixture index, built once per module)


@pytest.fixture(scope="module", autouse=True)
def _built(skl):
    import os

    assert os.path.exists(CLI)


def test_top_needs_a_value(wd):  # noqa: F811
    usage_error(run(wd, "-f", "rfile.txt", "inverted.ski", "--top"),
                "a value is required for '--top <N>' but none was supplied")


@pytest.mark.parametrize("value", ["three", "-3", "3.5", ""])
def test_top_is_a_number(wd, value):  # noqa: F811
    usage_error(run(wd, "-f", "rfile.txt", "inverted.ski", "--top", value),
                f"invalid value '{value}' for '--top <N>': invalid digit found in string")


def test_top_zero(wd):  # noqa: F811
    usage_error(run(wd, "-f", "rfile.txt", "inverted.ski", "--top", "0"),
                "invalid value '0' for '--top <N>': 0 is not in 1..=1024")


@pytest.mark.parametrize("value", ["1025", "1000000", "99999999999999999999999"])
def test_top_above_the_limit_names_it(wd, value):  # noqa: F811
    usage_error(run(wd, "-f", "rfile.txt", "inverted.ski", "--top", value),
                f"invalid value '{value}' for '--top <N>': {value} is not in 1..=1024")


@pytest.mark.parametrize("mode", ["all-bins", "any-bins"])
@pytest.mark.parametrize("top_first", [True, False])
def test_top_is_an_option_of_match_count(wd, mode, top_first):  # noqa: F811
    args = ["--top", "3", "--query-type", mode] if top_first else ["--query-type", mode, "--top", "3"]
    usage_error(run(wd, "-f", "rfile.txt", "inverted.ski", *args),
                "the argument '--top <N>' cannot be used with '--query-type <QUERY_TYPE>'")


def test_missing_ski_is_an_error(wd):  # noqa: F811
    res = run(wd, "-f", "rfile.txt", "missing.ski", "--top", "3")
    assert res.returncode == 1 and res.stdout == ""
    assert res.stderr == "Error: Could not open missing.ski\n"
    # naming the default type beside --top is not a conflict: the same error, not a usage error
    res = run(wd, "-f", "rfile.txt", "missing.ski", "--query-type", "match-count", "--top", "3")
    assert res.returncode == 1 and res.stderr == "Error: Could not open missing.ski\n"
