"""bench.py end to end on the GPU: a plain run (no --full) with --dump-outputs.

The line carries the headline fields and none of the --full figures, --steps is the number of
timed steps of a batch, and the dumped arrays are what a caller of the timed path receives after
the last timed step: a fresh engine with the benchmark's inputs, run for the same
max(1, warmup) + steps control steps, reads back the same bits (the steps are deterministic: the
same warm start, state, target and Philox (seed, step) give the same launches)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 3, 2


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    from quadrotor_manipulator_mppi_amd.distributed import ShardedEngine
    d = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--dump-outputs", str(d)], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["full"] is False and line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["timing"]["steps_per_batch"] == STEPS and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(4096 * 32 / (line["ms_per_step"] * 1e-3))
    assert line["unit"] == "rollout-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    for k in ("secondary", "cpu_baseline", "roofline", "kernels", "latency_p50_ms", "latency_100hz"):
        assert line[k] is None, k
    assert "dropin_latency" not in line
    assert sorted(os.listdir(d)) == ["costs.npy", "out.npy", "stats.npy", "u0.npy", "u_prev.npy"]
    got = {k[:-4]: np.load(d / k) for k in os.listdir(d)}
    assert {k: str(v.dtype) for k, v in got.items()} == {
        "out": "float64", "stats": "float64", "u0": "float32", "u_prev": "float32", "costs": "float32"}
    assert {k: v["shape"] for k, v in line["outputs"]["arrays"].items()} == {k: list(v.shape) for k, v in got.items()}
    assert sum(v.nbytes for v in got.values()) <= bench.DUMP_MAX_BYTES

    w = dict(bench.WORKLOADS["arm_c3"])
    w.pop("desc")
    se = ShardedEngine(seed=1234, native=None, mode=None, **w)
    try:
        eng = se.engine
        bench.set_targets(eng, "arm", se.vehicles)
        eng.set_state(bench.make_state("arm", 1))
        se.run_steps(max(1, WARMUP) + STEPS)
        eng.synchronize()
        out, u0, st = eng.read_outputs()
        ref = {"out": out, "u0": u0, "u_prev": eng.get_u_prev(), "costs": eng.get_costs(),
               "stats": np.array([[s.rho, s.eta, s.ess] for s in st], np.float64)}
    finally:
        eng.close()
    assert np.isfinite(ref["out"]).all() and ref["costs"].shape == (1, 4096)
    assert np.abs(ref["u_prev"]).max() > 0, "the steps moved the warm start"
    for k, v in ref.items():
        assert np.array_equal(got[k], v), f"{k}: max|d|={np.abs(got[k] - v).max()}"
