"""Host time of one drop-in tick with a stub engine, several trees alternated in ONE process (tools/, not shipped).

    python tools/time_dropin_host.py [--calls 100000] [--times 3] [--slice 2000] <tree> [<tree> ...]

No GPU: every tree's package is imported under a name of its own (its imports are relative), and
``Engine`` in every ``mppi_solver`` module of it is a stub whose ``step`` returns fixed arrays, so what
is timed is the Python of the classes alone: the arm class's ``update_joint`` +
``compute_control_input`` (fp64 tensors, as bench.py's dropin_latency) and the drone class's
``set_state`` + ``compute_control_input``.  A time is ``--calls`` calls of ``timeit``, taken in slices
of ``--slice`` calls with the trees alternated slice by slice (separate processes, and whole times one
after the other, differ by more than the trees do on a shared machine: 11 to 18 us for the same code);
the last lines give each tree's ``--times`` figures in microseconds per tick, their median and the
slowest.
"""
import argparse
import importlib
import os
import pkgutil
import statistics
import sys
import timeit
import types


def load(tree, alias):
    """(arm tick, drone tick) of the tree's classes over a stub engine."""
    import numpy as np
    import torch
    pkg = types.ModuleType(alias)
    pkg.__path__ = [os.path.join(os.path.abspath(tree), "quadrotor_manipulator_mppi_amd")]
    sys.modules[alias] = pkg
    solver = importlib.import_module(f"{alias}.mppi_solver")
    StepStats = importlib.import_module(f"{alias}.engine").StepStats

    class Stub:
        def __init__(self, cfg):
            self.cfg, self.K, self.H = cfg, cfg.n_samples, cfg.n_horizon
            self._ret = (np.zeros((1, 14 if cfg.n_action == 7 else 6)), np.zeros((1, cfg.n_action), np.float32), [StepStats(0.0, 1.0, 2.0, False, False)])

        def close(self): pass
        def set_u_prev(self, u): pass
        def set_prewarm(self, us): pass
        def set_target(self, pos, quat=None): pass
        def step(self, state=None, noise=None): return self._ret

    mods = [importlib.import_module(f"{solver.__name__}.{m.name}") for m in pkgutil.iter_modules(solver.__path__)]
    for mod in mods:
        if hasattr(mod, "Engine"):
            mod.Engine = Stub
    arm = sys.modules[f"{solver.__name__}.mppi"].MPPI(n_samples=32, n_horizon=32, verbose=False)
    drone = sys.modules[f"{solver.__name__}.drone_mppi"].MPPI(n_samples=32, n_timestep=16)
    drone._out_ring.device = torch.device("cpu")   # (no device copy in a host timing)
    q = torch.tensor([0, 0, 1, 0, 0, 0, 1] + [1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0], dtype=torch.float64)
    v = torch.zeros(13, dtype=torch.float64)
    x, xd = [0.1, 0.2, 0.3], [0.0, 0.0, 0.0]

    def arm_tick():
        arm.update_joint(q, v)
        arm.compute_control_input()

    def drone_tick():
        drone.set_state(x, xd)
        drone.compute_control_input()

    return arm_tick, drone_tick


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100000)
    ap.add_argument("--times", type=int, default=3)
    ap.add_argument("--slice", type=int, default=2000)
    ap.add_argument("trees", nargs="+")
    a = ap.parse_args()
    ticks = [load(t, f"tree{i}") for i, t in enumerate(a.trees)]
    n = max(1, a.calls // a.slice)
    for i, what in enumerate(("arm", "drone")):
        for fs in ticks:
            timeit.timeit(fs[i], number=a.slice)
        got = [[] for _ in ticks]
        for _ in range(a.times):
            tot = [0.0] * len(ticks)
            for s in range(n):
                order = range(len(ticks)) if s % 2 == 0 else reversed(range(len(ticks)))
                for k in order:
                    tot[k] += timeit.timeit(ticks[k][i], number=a.slice)
            for k, t in enumerate(tot):
                got[k].append(t / (n * a.slice) * 1e6)
        for t, xs in zip(a.trees, got):
            print(f"{t} {what}: {' '.join(f'{x:.3f}' for x in xs)} | median {statistics.median(xs):.3f} slowest {max(xs):.3f}", flush=True)


if __name__ == "__main__":
    main()
