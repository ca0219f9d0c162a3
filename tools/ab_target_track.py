"""The price of target tracking: a tracking engine against the extended-kernel (XC) and the common-kernel
engines of another build, same process, both engine orders (tools/, not shipped).

    python tools/ab_target_track.py <reps> <lib_new.so> <lib_parent.so>

Per shape (arm C3: fp64 state K=4096 H=32; whole-body K=8192 H=64; drone C2: K=4096 H=32; quadrotor
K=4096 H=32) three engines: `track` = lib_new with cost_terms = target_track and a table set; `xc` =
lib_parent with cost_terms = center at w_center = 0, the nearest extended launch it has (ARM and
WHOLEBODY only: the vehicles take no CostManager terms); `common` = lib_parent's default engine.
Per rep the wall time of a 500-step mppi_run_steps batch (MPPI_AB_STEPS) of each engine, in the
order track, xc, common on even reps and reversed on odd ones; the medians per order and overall.
Then the wall time of one set_target_trajectory call at C3: 200 calls after 20.
Both libraries are loaded RTLD_LOCAL with their code objects next to them, as tools/ab_native.py does.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
from tools.ab_native import STATE, load

SHAPES = [("arm", 4096, 32), ("wholebody", 8192, 64), ("drone", 4096, 32), ("quadrotor", 4096, 32)]


def engine(lib, model, K, H, **kw):
    capi._lib = lib
    e = Engine(make_config(model, n_samples=K, n_horizon=H, state_f64=(model == "arm"), **kw))
    if model in ("drone", "quadrotor"):
        e.set_target([1.0, 2.0, 3.4])
    else:
        e.set_target([0.1, 0.4, 1.6], [-0.5, -0.5, 0.5, -0.5])
    e.set_state(np.array(STATE[model], np.float64)[None])
    return e


def table(H):
    t = (np.arange(H, dtype=np.float32) + 1.0)[:, None] * 0.01
    pos = np.array([0.1, 0.4, 1.6], np.float32) + 0.5 * t * np.array([0.8, 0.5, -0.3], np.float32)
    quat = np.tile(np.array([-0.5, -0.5, 0.5, -0.5], np.float32), (H, 1))
    return pos, quat


def main():
    reps = int(sys.argv[1])
    new, parent = load(sys.argv[2]), load(sys.argv[3])
    steps = int(os.environ.get("MPPI_AB_STEPS", "500"))
    for model, K, H in SHAPES:
        eng = {"track": engine(new, model, K, H, cost_terms=("target_track",))}
        eng["track"].set_target_trajectory(*table(H))
        if model in ("arm", "wholebody"):
            eng["xc"] = engine(parent, model, K, H, cost_terms=("center",), cost_weights={"w_center": 0.0})
        eng["common"] = engine(parent, model, K, H)
        for e in eng.values():
            e.run_steps(50)
            e.synchronize()
        names = list(eng)
        res = {(n, o): [] for n in names for o in (0, 1)}
        for rep in range(reps):
            order = names if rep % 2 == 0 else names[::-1]
            for n in order:
                e = eng[n]
                e.run_steps(50)
                e.synchronize()
                t0 = time.perf_counter()
                e.run_steps(steps)
                e.synchronize()
                res[n, rep % 2].append((time.perf_counter() - t0) / steps * 1e6)
        print(f"{model} K={K} H={H}: us per step over {steps}-step batches, {reps} reps, dispatch {eng['track'].dispatch_info()!r}")
        for n in names:
            a, b = np.array(res[n, 0]), np.array(res[n, 1])
            both = np.concatenate([a, b])
            q1, q3 = np.percentile(both, [25, 75])
            print(f"  {n:7s} median {np.median(both):7.3f}  (order forward {np.median(a):7.3f}, reversed {np.median(b):7.3f}; "
                  f"IQR {q3 - q1:.3f}, min {both.min():.3f})")
        if model == "arm":
            e = eng["track"]
            pos, quat = table(H)
            ts = []
            for i in range(220):
                pos[:, 0] += 1e-4
                t0 = time.perf_counter()
                e.set_target_trajectory(pos, quat)
                if i >= 20:
                    ts.append((time.perf_counter() - t0) * 1e6)
            print(f"  set_target_trajectory at C3: median {np.median(ts):.1f} us per call (200 calls after 20; "
                  f"IQR {np.subtract(*np.percentile(ts, [75, 25])):.1f})")
        for e in eng.values():
            e.close()


if __name__ == "__main__":
    main()
