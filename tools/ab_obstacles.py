"""The price of the obstacle term: scene engines with 0, 4 and 16 obstacles against the tracking engine
of another build, same process, both engine orders (tools/, not shipped).

    python tools/ab_obstacles.py <reps> <lib_new.so> <lib_parent.so>

Per shape (C3: arm fp64 state K=4096 H=32; the C4 rank shape: whole-body K=8192 H=64) four engines:
`track` = lib_parent with cost_terms = target_track and a table set; `scene0`, `scene4`, `scene16` =
lib_new scene engines (9 body spheres, the tracking bit and the same table) with that many obstacles,
a quarter of them inside the margin of the arm's sweep, the rest metres away (the loops run over all
of them either way).  Per rep the wall time of a 500-step mppi_run_steps batch (MPPI_AB_STEPS) of each
engine, in the listed order on even reps and reversed on odd ones; the medians per order and overall.
Then the wall time of one set_obstacles call (16 obstacles) at C3: 200 calls after 20.
Both libraries are loaded RTLD_LOCAL with their code objects next to them, as tools/ab_native.py does.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd.engine import Engine, Scene, make_config
from tools.ab_native import STATE, load
from tools.ab_target_track import table

SHAPES = [("arm", 4096, 32), ("wholebody", 8192, 64)]
BODY = ((-1, (0.0, 0.0, -0.05), 0.09), (0, (0.0, 0.02, 0.08), 0.07), (1, (0.0, 0.0, 0.0), 0.05),
        (2, (0.0, -0.1, 0.0), 0.05), (3, (0.0, 0.03, -0.04), 0.05), (4, (0.0, 0.1, 0.0), 0.05),
        (5, (0.0, 0.0, 0.0), 0.05), (6, (0.0, 0.0, 0.0), 0.05), (7, (0.0, 0.0, -0.1), 0.04))


def engine(lib, model, K, H, scene=None):
    capi._lib = lib
    e = Engine(make_config(model, n_samples=K, n_horizon=H, state_f64=(model == "arm"), cost_terms=("target_track",)),
               **({} if scene is None else {"scene": scene}))
    e.set_target([0.1, 0.4, 1.6], [-0.5, -0.5, 0.5, -0.5])
    e.set_target_trajectory(*table(H))
    e.set_state(np.array(STATE[model], np.float64)[None])
    return e


def obstacles(n, near):
    """n obstacles: every fourth within reach of `near` (a point by the arm), the others metres away."""
    c = np.zeros((n, 3), np.float32)
    for i in range(n):
        c[i] = (np.asarray(near) + [0.12 + 0.02 * i, 0.05, -0.03 * (i % 3)]) if i % 4 == 0 else (3.0 + i, -2.0, 1.0 + 0.1 * i)
    return c, np.full(n, 0.06, np.float32), np.tile(np.array([0.1, -0.05, 0.0], np.float32), (n, 1))


def main():
    reps = int(sys.argv[1])
    new, parent = load(sys.argv[2]), load(sys.argv[3])
    steps = int(os.environ.get("MPPI_AB_STEPS", "500"))
    for model, K, H in SHAPES:
        near = np.asarray(STATE[model][:3], np.float32) + [-0.3, 0.4, -0.1]
        eng = {"track": engine(parent, model, K, H)}
        for n in (0, 4, 16):
            e = eng[f"scene{n}"] = engine(new, model, K, H, Scene(BODY))
            e.set_obstacles(*obstacles(n, near))
        for e in eng.values():
            e.run_steps(50)
            e.synchronize()
        clr = eng["scene16"].get_clearances()[0]
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
        print(f"{model} K={K} H={H}: us per step over {steps}-step batches, {reps} reps, dispatch {eng['scene16'].dispatch_info()!r}; "
              f"scene16 clearances {clr.min():.3f} .. {clr.max():.3f} m; kernels {eng['scene16'].kernel_info()!r}")
        base = None
        for n in names:
            a, b = np.array(res[n, 0]), np.array(res[n, 1])
            both = np.concatenate([a, b])
            q1, q3 = np.percentile(both, [25, 75])
            base = np.median(both) if base is None else base
            print(f"  {n:8s} median {np.median(both):7.3f}  ({np.median(both) - base:+.3f} vs track; order forward {np.median(a):7.3f}, "
                  f"reversed {np.median(b):7.3f}; IQR {q3 - q1:.3f}, min {both.min():.3f})")
        if model == "arm":
            e = eng["scene16"]
            c, r, v = obstacles(16, near)
            ts = []
            for i in range(220):
                c[:, 0] += 1e-4
                t0 = time.perf_counter()
                e.set_obstacles(c, r, v)
                if i >= 20:
                    ts.append((time.perf_counter() - t0) * 1e6)
            print(f"  set_obstacles (16) at C3: median {np.median(ts):.1f} us per call (200 calls after 20; "
                  f"IQR {np.subtract(*np.percentile(ts, [75, 25])):.1f})")
        for e in eng.values():
            e.close()


if __name__ == "__main__":
    main()
