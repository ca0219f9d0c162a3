"""The price of the self-collision term: self engines with the default pairs and with 32 pairs against the
scene engine without pairs of another build, same process, both engine orders (tools/, not shipped).

    python tools/ab_self_collision.py <reps> <lib_new.so> <lib_parent.so>

Per shape (C3: arm fp64 state K=4096 H=32; the C4 rank shape: whole-body K=8192 H=64) four engines:
`scene` = lib_parent's scene engine (9 body spheres, the tracking bit and a table set, no obstacles: its
k_rollout_ob at the automatic 512-thread block); `scene256` = the same at block_threads = 256, the block a
self engine gets; `self_d` = lib_new's self engine with the default pairs of those spheres
(SelfCollision.default), `self32` = with 32 pairs.  Per rep the wall time of a 500-step mppi_run_steps
batch (MPPI_AB_STEPS) of each engine, in the listed order on even reps and reversed on odd ones; the
medians per order and overall, and the added us per step and per pair against `scene`.
Both libraries are loaded RTLD_LOCAL with their code objects next to them, as tools/ab_native.py does.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd.engine import Engine, Scene, SelfCollision, make_config
from tools.ab_native import STATE, load
from tools.ab_obstacles import BODY
from tools.ab_target_track import table

SHAPES = [("arm", 4096, 32), ("wholebody", 8192, 64)]


def engine(lib, model, K, H, pairs=None, **kw):
    capi._lib = lib
    cfg = make_config(model, n_samples=K, n_horizon=H, state_f64=(model == "arm"), cost_terms=("target_track",), **kw)
    scene = Scene(BODY)
    sc = None
    if pairs == "default":
        sc = SelfCollision.default(cfg, scene)
    elif pairs is not None:
        every = [(a, b) for a in range(len(BODY)) for b in range(a + 1, len(BODY)) if (a, b) != (0, 1)]   # (0, 1): rigid
        sc = SelfCollision(every[:pairs])
    e = Engine(cfg, scene=scene) if sc is None else Engine(cfg, scene=scene, self_collision=sc)
    e.set_target([0.1, 0.4, 1.6], [-0.5, -0.5, 0.5, -0.5])
    e.set_target_trajectory(*table(H))
    e.set_state(np.array(STATE[model], np.float64)[None])
    return e, (0 if sc is None else len(sc.pairs))


def main():
    reps = int(sys.argv[1])
    new, parent = load(sys.argv[2]), load(sys.argv[3])
    steps = int(os.environ.get("MPPI_AB_STEPS", "500"))
    for model, K, H in SHAPES:
        eng = {"scene": engine(parent, model, K, H), "scene256": engine(parent, model, K, H, block_threads=256),
               "self_d": engine(new, model, K, H, "default"), "self32": engine(new, model, K, H, 32)}
        for e, _ in eng.values():
            e.run_steps(50)
            e.synchronize()
        sclr = eng["self32"][0].get_self_clearances()[0]
        names = list(eng)
        res = {(n, o): [] for n in names for o in (0, 1)}
        for rep in range(reps):
            order = names if rep % 2 == 0 else names[::-1]
            for n in order:
                e = eng[n][0]
                e.run_steps(50)
                e.synchronize()
                t0 = time.perf_counter()
                e.run_steps(steps)
                e.synchronize()
                res[n, rep % 2].append((time.perf_counter() - t0) / steps * 1e6)
        print(f"{model} K={K} H={H}: us per step over {steps}-step batches, {reps} reps, dispatch {eng['self32'][0].dispatch_info()!r}; "
              f"self32 clearances {sclr.min():.3f} .. {sclr.max():.3f} m; kernels {eng['self32'][0].kernel_info()!r}")
        base = None
        for n in names:
            a, b = np.array(res[n, 0]), np.array(res[n, 1])
            both = np.concatenate([a, b])
            q1, q3 = np.percentile(both, [25, 75])
            base = np.median(both) if base is None else base
            pairs = eng[n][1]
            per = f", {(np.median(both) - base) / pairs:+.3f} per pair ({pairs})" if pairs else ""
            print(f"  {n:8s} median {np.median(both):7.3f}  ({np.median(both) - base:+.3f} vs scene{per}; order forward {np.median(a):7.3f}, "
                  f"reversed {np.median(b):7.3f}; IQR {q3 - q1:.3f}, min {both.min():.3f})")
        for e, _ in eng.values():
            e.close()


if __name__ == "__main__":
    main()
