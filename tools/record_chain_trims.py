"""Record tests/golden/chain_trims/parent.npz: the outputs of the shapes that reach every path the
chain trims touch (csrc/mppi_rollout.h: kernel-argument scalars pinned in the prologue, the combine's
store bases ahead of its barrier; csrc/mppi_finalize.hip: the full-chunk path, the row factors'
selects), taken from the build of the commit BEFORE those edits on an MI355X.

    python tools/record_chain_trims.py [--out tests/golden/chain_trims/parent.npz]

tests/test_gpu_chain_trims.py imports CASES and run_case from here and compares the tree's outputs
with the recording bit for bit.  Per case: a native batch (3 steps; 4 at C3), then one control call;
device Philox, a seed of the case's own (so no two cases record the same numbers).  (A directory of its
own: the .npz files directly under tests/golden are the reference's, tests/test_golden_regen.py.)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HOME = [1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0]
ARM64 = dict(n_horizon=32, state_f64=True)
# (name, model, make_config keywords, environment at engine creation, batch steps)
CASES = [
    # 3 blocks: a ragged finalize chunk, waves that hold only k >= K rollouts (rho_w = +inf), a half-valid wave
    ("arm64-K40", "arm", dict(n_samples=40, **ARM64), {}, 3),
    ("arm64-K2048", "arm", dict(n_samples=2048, **ARM64), {}, 3),     # 128 records: a full chunk of the 128 class
    ("arm64-K4096", "arm", dict(n_samples=4096, **ARM64), {}, 4),     # 256 records: the C3 kernels themselves
    ("arm32-K48", "arm", dict(n_samples=48, n_horizon=32, state_f64=False), {}, 3),
    ("drone-K100-H20", "drone", dict(n_samples=100, n_horizon=20), {}, 3),
    ("wholebody-K96", "wholebody", dict(n_samples=96, n_horizon=64), {}, 3),
    ("wholebody-K64-V2", "wholebody", dict(n_samples=64, n_horizon=64, n_vehicles=2), {}, 3),   # the v products stay live
    ("arm64-K32-center", "arm", dict(n_samples=32, cost_terms=("center",), **ARM64), {}, 3),   # an extended (XC) body
    ("arm64-K32-track", "arm", dict(n_samples=32, cost_terms=("target_track",), **ARM64), {}, 3),
    ("arm64-K40-generic", "arm", dict(n_samples=40, **ARM64), {"MPPI_GENERIC_KERNELS": "1"}, 3),   # run-time geometry
]
NAMES = [c[0] for c in CASES]
FIELDS = ("u_prev", "costs", "out", "u0", "stats")
FIXTURE = os.path.join(ROOT, "tests", "golden", "chain_trims", "parent.npz")


def _state(model, V, shift=0.0):
    if model == "arm":
        s = [0, 0, 1, 0, 0, 0, 1] + HOME + [0.0] * 7
    elif model == "drone":
        s = [0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    else:
        s = [0, 0, 1, 0, 0, 0, 1] + HOME + [0.0] * 10
    s = np.tile(np.array(s, np.float64), (V, 1))
    s[:, 0] += shift
    return s


def _stats(st):
    return np.array([(s.rho, s.eta, s.ess, s.nonfinite) for s in st], np.float64)


def _snapshot(e, outs):
    out, u0, st = outs
    return dict(u_prev=e.get_u_prev(), costs=e.get_costs(), out=out, u0=u0, stats=_stats(st))


def run_case(case):
    """{"batch.<field>", "call.<field>"}: the engine's outputs after the batch and after the call."""
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    name, model, kw, env, steps = case
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)   # read at mppi_create
    try:
        e = Engine(make_config(model, device=0, seed=1000 + NAMES.index(name), **kw))
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        for v in range(e.V):
            if model == "drone":
                e.set_target([1.0, 2.0, 3.4], vehicle=v)
            else:
                e.set_target([0.1029 + 0.05 * v, 0.4055, 1.6498], [-0.5, -0.5, 0.5, -0.5], vehicle=v)
            if "target_track" in kw.get("cost_terms", ()):
                t = np.linspace(0.0, 1.0, e.H)[:, None]
                e.set_target_trajectory(np.array([0.1029, 0.4055, 1.6498]) + t * np.array([0.1, -0.05, 0.02]),
                                        vehicle=v)
        e.set_state(_state(model, e.V))
        res = {}
        e.run_steps(steps)
        e.synchronize()
        for f, x in _snapshot(e, e.read_outputs()).items():
            res["batch." + f] = x
        for f, x in _snapshot(e, e.step(_state(model, e.V, shift=0.01))).items():
            res["call." + f] = x
        return res
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    rec = {}
    for case in CASES:
        for k, x in run_case(case).items():
            rec[f"{case[0]}/{k}"] = x
        print(case[0], "recorded", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **rec)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
