"""The chain trims (csrc/mppi_rollout.h: the kernel-argument scalars held in SGPRs from the prologue,
the combine's store bases formed ahead of its barrier; csrc/mppi_finalize.hip: the full-chunk path and
the row factors without their selects) must leave every result bit for bit what the commit before them
computed.  tests/golden/chain_trims/parent.npz is that commit's build on an MI355X, recorded by
tools/record_chain_trims.py, which also holds the shapes -- the smallest that reach each changed path --
and the run this test repeats: a native batch, then one control call, device Philox, a fixed seed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import record_chain_trims as R  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = [f"{when}.{f}" for when in ("batch", "call") for f in R.FIELDS]


@pytest.fixture(scope="module")
def parent():
    return dict(np.load(R.FIXTURE, allow_pickle=False))


def _blob(rec, name):
    return b"".join(np.ascontiguousarray(rec[f"{name}/{k}"]).tobytes() for k in KEYS)


def test_fixture_holds_every_case(parent):
    assert sorted(parent) == sorted(f"{n}/{k}" for n in R.NAMES for k in KEYS)
    assert os.path.getsize(R.FIXTURE) < 200 * 1024


@pytest.mark.parametrize("case", R.CASES, ids=R.NAMES)
def test_outputs_are_the_parents_bit_for_bit(monkeypatch, parent, case):
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    name = case[0]
    # the recording tells the cases apart and is a real run: no two alike, finite, a moved warm start
    mine = _blob(parent, name)
    assert all(_blob(parent, o) != mine for o in R.NAMES if o != name)
    for when in ("batch", "call"):
        assert np.isfinite(parent[f"{name}/{when}.u_prev"]).all() and np.abs(parent[f"{name}/{when}.u_prev"]).max() > 1e-3
        assert np.isfinite(parent[f"{name}/{when}.costs"]).all() and parent[f"{name}/{when}.costs"].std() > 0
    got = R.run_case(case)
    for k in KEYS:
        a, b = got[k], parent[f"{name}/{k}"]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        # (bit patterns: -0.0 and NaN payloads count)
        assert a.tobytes() == b.tobytes(), f"{name} {k}: {int(np.sum(a != b))} of {a.size} differ, max |d| {np.abs(a - b).max()}"
