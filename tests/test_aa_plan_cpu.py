"""csrc/aa_plan.hpp decides which thread of which kernel form hashes which window starts of which sample in
skl_sketch_signs_aa, and how the samples fall into batches -- as pure functions, two of which (aa_short_item, aa_long_item) the
kernels themselves call on the device.  Here they run on the CPU: tests/native/aa_check.cpp walks every item of both forms and
requires that every window start of every sample is covered exactly once, that no item leaves its sample, that no thread of the
unstaged form is idle (short samples cost no padding), that a sample takes one form only, and that batches are whole samples
within their caps.  Built with the host compiler alone; the GPU suite checks the same kernels against the restatement."""
import subprocess

import numpy as np
import pytest

import aa_native

K = 7
LONG_MIN = 8192
SHORT = [int(x) for x in np.random.default_rng(3).integers(5, 71, size=3000)]


def covered(k, long_min, lengths):
    res = subprocess.run([aa_native.build(), "plan", str(k), str(long_min), *map(str, lengths)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.startswith("ok "), res.stdout + res.stderr
    return int(res.stdout.split()[1])


@pytest.mark.parametrize("lengths", [[0], [1], [K - 1, K, K + 1], SHORT, [10 ** 6], SHORT[:1500] + [10 ** 6] + SHORT[1500:]],
                         ids=["empty", "one", "around_k", "short3000", "long", "mix"])
@pytest.mark.parametrize("k,long_min", [(K, LONG_MIN), (K, 1), (300, LONG_MIN)], ids=["default", "all_staged", "k_past_staged"])
def test_every_window_start_once(lengths, k, long_min):
    assert covered(k, long_min, lengths) == sum(lengths)


def test_chunk_and_span_edges():
    """Lengths at the edges of a thread span and a workgroup chunk of either form."""
    lengths = [63, 64, 65, 16383, 16384, 16385, 8191, 8192, 8193, 15, 16, 17, 0, 2 * 16384]
    for k, long_min in ((3, LONG_MIN), (3, 1), (40, LONG_MIN), (257, 1)):
        assert covered(k, long_min, lengths) == sum(lengths)
