"""The launches the step paths hand to the launchers, without a GPU, against a recording: the sweep of
tools/record_step_launches.py (the five model rows at H = 32 and 64, V = 1 and 3; plain, stored and
injected noise, a shard, a peer exchange, the generic kernels, timing, an engine-owned communicator,
MPPI_DEBUG_OUT; a batch of one step and of three and a control call, through HIP and natively)
replayed through mppi_debug_step_launches must describe, row by row, the launches
tests/golden/step_launches.json holds: the kernel, the geometry, the argument size and the digest of
the argument bytes of every rollout, PACK and finalize of a step before the last and of the last
step -- recorded from the library as it was while every path assembled its DevParams and FinParams
by hand.  A path an engine would not take is recorded, and replayed, as a refusal."""
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_step_launches as R  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "step_launches.json")) as f:
        return R.decode(json.load(f))


@pytest.fixture(scope="module")
def replayed():
    return R.sweep()


def test_replayed_sweep_equals_the_recording(recorded, replayed):
    assert len(recorded) == len(replayed) == len(list(R.sweep_rows()))
    for want, (what, got) in zip(recorded, replayed):
        assert got == want, what


def test_recording_is_not_vacuous(recorded):
    rows = dict(zip((what for what, _, _ in R.sweep_rows()), recorded))
    assert len(rows) == len(R.MODELS) * 2 * 2 * (len(R.VARIANTS) * len(R.PATHS) - 3)   # (injected: not natively)
    took = [a for a in recorded if a != R.REFUSED]
    assert len(took) > len(recorded) // 2 and R.REFUSED in recorded
    assert all(sym.startswith("_Z") and "?" not in sym for a in took for _, _, sym, *_ in a)
    assert {kind for a in took for _, kind, *_ in a} == {"rollout", "pack", "finalize"}
    # several steps: a step before the last, then the last; one step or a call: the last alone
    for what, a in rows.items():
        if a != R.REFUSED:
            assert [lch[0] for lch in a] == sorted(lch[0] for lch in a), what
            assert ({lch[0] for lch in a} == {"early", "last"}) == what.endswith("n=3"), what
    # the quiet kernels run in a plain batch's early steps, natively and through HIP alike, and
    # nowhere in a peer engine's, a generic one's or one with timing
    for path in (R.HIP_BATCH, R.NATIVE_BATCH):
        plain = rows[f"arm f64 H=32 V=1 plain path {path} n=3"]
        assert [lch[2] for lch in plain[:2]] != [lch[2] for lch in plain[2:]]
        assert plain[0][2].startswith("_Z11k_rollout_q")
    for name in ("peer 1/2", "generic", "timing"):
        a = rows[f"arm f64 H=32 V=1 {name} path {R.HIP_BATCH} n=3"]
        assert [lch[2] for lch in a[:2]] == [lch[2] for lch in a[2:]], name
    # the paths differ where they should: the native rollout counts its step from the dispatch id,
    # the native call's finalize takes its sequence number from the vehicle constants
    hip, batch, call = (rows[f"arm f64 H=32 V=1 plain path {p} n=1"] for p in (R.HIP_CALL, R.NATIVE_BATCH, R.NATIVE_CALL))
    assert hip[0][:7] == batch[0][:7] and hip[0][7] != batch[0][7]
    assert batch[0] == call[0] and batch[1][7] != call[1][7]
    # a shard packs between its rollout and its finalize; natively it is refused
    shard = rows[f"arm f64 H=32 V=1 shard 1/2 path {R.HIP_CALL} n=1"]
    assert [lch[1] for lch in shard] == ["rollout", "pack", "finalize"]
    assert rows[f"arm f64 H=32 V=1 shard 1/2 path {R.NATIVE_CALL} n=1"] == R.REFUSED
    assert rows[f"arm f64 H=32 V=3 plain path {R.NATIVE_CALL} n=1"] == R.REFUSED
    assert rows[f"arm f64 H=32 V=1 timing path {R.NATIVE_BATCH} n=3"] == R.REFUSED
    assert rows[f"arm f64 H=32 V=1 injected path {R.HIP_BATCH} n=3"] == R.REFUSED
    assert rows[f"arm f64 H=32 V=1 injected path {R.HIP_CALL} n=1"] != R.REFUSED


def test_refusals_say_why():
    from quadrotor_manipulator_mppi_amd import _capi as capi
    from quadrotor_manipulator_mppi_amd.engine import make_config
    assert R.launches(make_config("arm", n_samples=256, n_vehicles=3), dict(path=R.NATIVE_CALL, n=1)) == R.REFUSED
    assert b"one vehicle" in capi.lib().mppi_last_error()
    assert R.launches(make_config("arm", n_samples=256), dict(path=R.NATIVE_BATCH, n=3, timing=1)) == R.REFUSED
    assert b"timing" in capi.lib().mppi_last_error()
