"""The operator-level API computes, bit for bit, what the commit recorded in tests/golden/ops_parent.json computed: every
output's SHA-256, shape and dtype, and every scalar result (frac_bits, clamp count, layer statistics, "returned None").
The digests hold for the ROCm version and GPU named in the file; after a toolchain change, rerun
tests/golden/gen_golden_ops_parent.py at that commit first to tell an environment change from a regression."""
import json
import os

import pytest

from ops_parent_cases import CASES, summarise

with open(os.path.join(os.path.dirname(__file__), "golden", "ops_parent.json")) as _f:
    GOLD = json.load(_f)


def test_every_case_is_recorded():
    assert sorted(GOLD["cases"]) == sorted(cid for cid, _ in CASES)
    assert len(GOLD["commit"]) == 40 and GOLD["rocm"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_operator_outputs_equal_the_recorded_parent(case):
    cid, fn = case
    got, want = summarise(fn()), GOLD["cases"][cid]
    assert sorted(got) == sorted(want)
    differ = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not differ, "%s differs from commit %s (ROCm %s): %r" % (cid, GOLD["commit"][:12], GOLD["rocm"], differ)
