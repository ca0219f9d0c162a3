"""Record what the drop-in solver classes ask of their engine, over one scenario each (tools/, not shipped).

    python tools/record_dropin_calls.py [--out tests/golden/dropin_calls.json]

No GPU: the name ``Engine`` in every ``mppi_solver`` module that has it is replaced by a stub that logs
its creation (a digest of the config's bytes; ``make_config`` is the real one) and every ``close``,
``get_u_prev``, ``set_u_prev``, ``set_prewarm``, ``set_target`` and ``step`` with its arguments (arrays
as dtype, shape and a digest), and answers ``step`` with outputs that depend only on the call's number
(``reach`` on an engine's second step; the warm start moves by one per step, so a rebuild's carry-over
shows in the log).  After every control call the log also takes what the call returned and printed,
``m.u`` and the class's public surface (instance attributes and properties).  The fixture pins the
engine lifecycle (what rebuilds an engine, in which order the warm start and the prewarm reach the new
one), the target writes (only when the bytes changed, once per engine) and the values handed back, so
the three classes can share code and be shown to make the same calls
(tests/test_dropin_calls_cpu.py replays the scenarios).  It was recorded while ``mppi.py``,
``drone_mppi.py`` and ``quadrotor_mppi.py`` each carried their own copy of all of it.

The fixture's layout: {class: [event, ...]}, an event a list headed by its name.
"""
import argparse
import contextlib
import ctypes as C
import hashlib
import importlib
import io
import json
import os
import pkgutil
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from quadrotor_manipulator_mppi_amd import _capi as capi  # noqa: E402
from quadrotor_manipulator_mppi_amd import mppi_solver  # noqa: E402
from quadrotor_manipulator_mppi_amd.engine import StepStats  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "dropin_calls.json")


def digest(b: bytes) -> str:
    return hashlib.sha1(b).hexdigest()[:16]


def arr(x):
    """[dtype, shape, digest] of an array or a tensor (on any device); None stays None."""
    if x is None:
        return None
    a = np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x)
    return [str(a.dtype), list(a.shape), digest(a.tobytes())]


def shares(a, b) -> bool:
    """Whether the two returned values are views of one allocation."""
    if isinstance(a, torch.Tensor):
        return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
    return bool(np.shares_memory(a, b))


class StubEngine:
    """What the solver classes use of engine.Engine; every call goes to ``log``."""
    log = None

    def __init__(self, cfg):
        self.cfg = cfg
        self.V, self.K, self.H, self.A = cfg.n_vehicles, cfg.n_samples, cfg.n_horizon, cfg.n_action
        self.out_dim = capi.lib().mppi_output_dim(C.byref(cfg))
        self._u = np.zeros((self.V, self.H, self.A), np.float32)
        self._n = 0
        self.log.append(["create", digest(bytes(cfg))])

    def close(self):
        self.log.append(["close"])

    def get_u_prev(self):
        self.log.append(["get_u_prev"])
        return self._u.copy()

    def set_u_prev(self, u):
        self.log.append(["set_u_prev", arr(u)])
        self._u = np.array(u, np.float32).reshape(self.V, self.H, self.A)

    def set_prewarm(self, window_us):
        self.log.append(["set_prewarm", window_us])

    def set_target(self, pos, quat=None):
        self.log.append(["set_target", arr(pos), arr(quat)])

    def step(self, state=None, noise=None):
        self.log.append(["step", arr(state), arr(noise)])
        self._n += 1
        n = self._n
        self._u = self._u + 1.0
        out = (n + np.arange(self.out_dim) / 16.0).reshape(1, -1)
        u0 = (0.5 * n + np.arange(self.A, dtype=np.float32)).reshape(1, -1)
        return out, u0, [StepStats(float(n), 1.0, 2.0, False, n == 2)]


@contextlib.contextmanager
def stubbed(log):
    """``Engine`` -> StubEngine in every mppi_solver module that has the name."""
    mods = [importlib.import_module(f"{mppi_solver.__name__}.{m.name}") for m in pkgutil.iter_modules(mppi_solver.__path__)]
    saved = [(m, m.Engine) for m in mods if hasattr(m, "Engine")]
    assert saved
    StubEngine.log = log
    for m, _ in saved:
        m.Engine = StubEngine
    try:
        yield
    finally:
        for m, e in saved:
            m.Engine = e
        StubEngine.log = None


def surface(m):
    """The sorted public names of the instance's attributes and of its class's properties."""
    props = {n for c in type(m).__mro__ for n, v in vars(c).items() if isinstance(v, property)}
    return sorted(n for n in set(vars(m)) | props if not n.startswith("_"))


def call(m, log, noise=None):
    """One control call and what is to be seen after it."""
    said = io.StringIO()
    with contextlib.redirect_stdout(said):
        a, b = m.compute_control_input() if noise is None else m.compute_control_input(noise)
    log.append(["returned", arr(a), arr(b), shares(a, b), said.getvalue()])
    log.append(["u", arr(m.u)])
    log.append(["surface", surface(m)])


def arm_scenario(log):
    from quadrotor_manipulator_mppi_amd.mppi_solver.mppi import MPPI
    m = MPPI(n_samples=32, n_horizon=32, prewarm_us=200, verbose=False)
    log.append(["surface", surface(m)])
    m.u_prev = torch.arange(32 * 7, dtype=torch.float64).reshape(32, 7) / 64.0
    q = [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0]
    m.update_joint(q, [0.0] * 13)                       # Python lists: an fp32 state
    call(m, log)
    call(m, log)
    m.target_pose.pose = torch.tensor([0.2, 0.3, 1.5])
    m.update_joint(torch.tensor(q, dtype=torch.float64), torch.full((13,), 0.25, dtype=torch.float64))
    call(m, log)                                        # fp64 state: a new engine
    call(m, log, np.zeros((32, 32, 7), np.float32))     # injected noise: a new engine
    log.append(["u_prev", arr(m.u_prev)])
    log.append(["cnt", m.cnt])


def vehicle_scenario(cls, width):
    def run(log):
        m = cls(n_samples=32, n_timestep=16, prewarm_us=100)
        log.append(["surface", surface(m)])
        m.set_state(np.arange(width) / 8.0, -np.arange(width) / 4.0)
        call(m, log)
        m.target = [0.5, 1.5, 2.5]
        call(m, log)
        call(m, log)                                               # the same target: no write
        m.n_samples = 64
        call(m, log, np.zeros((64, 16, m.n_action), np.float32))   # more samples, injected: a new engine
        log.append(["u_prev", arr(m.u_prev)])
    return run


def scenarios():
    from quadrotor_manipulator_mppi_amd.mppi_solver.drone_mppi import MPPI as Drone
    from quadrotor_manipulator_mppi_amd.mppi_solver.quadrotor_mppi import MPPI as Quadrotor
    return {"arm": arm_scenario, "drone": vehicle_scenario(Drone, 3), "quadrotor": vehicle_scenario(Quadrotor, 6)}


def record():
    """{class: its scenario's events}."""
    out = {}
    for name, run in scenarios().items():
        log = []
        with stubbed(log):
            run(log)
        out[name] = log
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    doc = record()
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": [\n' + ",\n".join("  " + json.dumps(e) for e in v) + "\n ]"
                                   for k, v in doc.items()) + "\n}\n")
    print(f"{a.out}: " + ", ".join(f"{k} {len(v)} events" for k, v in doc.items())
          + f"; digest {digest(json.dumps(doc, sort_keys=True).encode())}")


if __name__ == "__main__":
    main()
