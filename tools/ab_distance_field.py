"""The price of the distance-field term: field engines against the scene engine of another build with no
obstacles, same process, both engine orders (tools/, not shipped).

    python tools/ab_distance_field.py <reps> <lib_new.so> <lib_parent.so>

Per shape (C3: arm fp64 state K=4096 H=32; the C4 rank shape: whole-body K=8192 H=64) five engines, all
with 9 body spheres and no sphere obstacles: `scene` = lib_parent's scene engine (k_rollout_ob);
`scene_new` = lib_new's scene engine (the same kernel, by the identity listing); `cleared` = a lib_new
field engine with a 64^3 grid and the field cleared (k_rollout_df: the price of the flag alone);
`field64`, `field128` = lib_new field engines with a 64^3 (2 MiB of x-pair cells) and a 128^3 (16 MiB)
field set: a floor 0.6 m under the grid's centre and a box beside it.  The body stands partly inside that
world from the first row (min clearance -0.16 m for the arm, -0.49 m for the whole-body model, the same at
both grid sizes), so hinge and penalty are active throughout; the loads are issued for every body sphere
on every row either way, and the timing does not depend on the values read.  Per rep the wall time of a
500-step mppi_run_steps batch (MPPI_AB_STEPS) of each engine, in the listed order on even reps and
reversed on odd ones; the medians per order and overall.  Then the wall time of one
set_distance_field call at both grid sizes: 200 calls after 20.
Both libraries are loaded RTLD_LOCAL with their code objects next to them, as tools/ab_native.py does.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd.engine import DistanceField, Engine, Scene, make_config
from tools.ab_native import STATE, load
from tools.ab_obstacles import BODY, SHAPES


def engine(lib, model, K, H, field=None):
    capi._lib = lib
    e = Engine(make_config(model, n_samples=K, n_horizon=H, state_f64=(model == "arm")), scene=Scene(BODY), field=field)
    e.set_target([0.1, 0.4, 1.6], [-0.5, -0.5, 0.5, -0.5])
    e.set_state(np.array(STATE[model], np.float64)[None])
    return e


def world(n, centre):
    """An n^3 grid, 2 m on a side, around `centre`: a floor 0.6 m below it and a box 0.3 m beside it
    (the robot at `centre` - 0.4 m in z reaches into both)."""
    voxel = 2.0 / (n - 1)
    c = np.asarray(centre, np.float64)
    origin = c - 1.0
    boxes = [((-9.0, -9.0, -9.0), (9.0, 9.0, c[2] - 0.6)), (tuple(c + [0.3, -0.2, -0.3]), tuple(c + [0.6, 0.2, 0.4]))]
    return DistanceField.from_boxes(boxes, (n, n, n), voxel, origin)


def main():
    reps = int(sys.argv[1])
    new, parent = load(sys.argv[2]), load(sys.argv[3])
    steps = int(os.environ.get("MPPI_AB_STEPS", "500"))
    for model, K, H in SHAPES:
        centre = np.asarray(STATE[model][:3], np.float64) + [0.0, 0.0, 0.4]
        f64, f128 = world(64, centre), world(128, centre)
        eng = {"scene": engine(parent, model, K, H), "scene_new": engine(new, model, K, H),
               "cleared": engine(new, model, K, H, DistanceField(f64.dims, f64.voxel, f64.origin)),
               "field64": engine(new, model, K, H, f64), "field128": engine(new, model, K, H, f128)}
        for e in eng.values():
            e.run_steps(50)
            e.synchronize()
        clr = {n: eng[n].get_clearances()[0] for n in ("cleared", "field64", "field128")}
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
        print(f"{model} K={K} H={H}: us per step over {steps}-step batches, {reps} reps, dispatch {eng['field64'].dispatch_info()!r}; "
              f"clearances cleared {clr['cleared'].min():.3f}, field64 {clr['field64'].min():.3f} .. {clr['field64'].max():.3f} m, "
              f"field128 {clr['field128'].min():.3f} .. {clr['field128'].max():.3f} m; kernels {eng['field64'].kernel_info()!r}")
        base = None
        for n in names:
            a, b = np.array(res[n, 0]), np.array(res[n, 1])
            both = np.concatenate([a, b])
            q1, q3 = np.percentile(both, [25, 75])
            base = np.median(both) if base is None else base
            print(f"  {n:9s} median {np.median(both):7.3f}  ({np.median(both) - base:+.3f} vs scene; order forward {np.median(a):7.3f}, "
                  f"reversed {np.median(b):7.3f}; IQR {q3 - q1:.3f}, min {both.min():.3f})")
        if model == "arm":
            for name, f in (("field64", f64), ("field128", f128)):
                e, d = eng[name], f.d.copy()
                ts = []
                for i in range(220):
                    d[0, 0, 0] += 1e-4
                    t0 = time.perf_counter()
                    e.set_distance_field(d)
                    if i >= 20:
                        ts.append((time.perf_counter() - t0) * 1e6)
                e.synchronize()
                print(f"  set_distance_field ({f.dims[0]}^3) at C3: median {np.median(ts):.1f} us per call (200 calls after 20; "
                      f"IQR {np.subtract(*np.percentile(ts, [75, 25])):.1f})")
        for e in eng.values():
            e.close()


if __name__ == "__main__":
    main()
