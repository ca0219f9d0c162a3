"""What the drop-in solver classes share: the engine's lifecycle, the warm start, the target
write, the lazy ``u``, the readbacks (``SolverBase``); the drone-shaped class body
(``VehicleSolver``: ``set_state`` and a control call returning device tensors); and the device
copy of those return values (``OutputRing``).

The reference drone solver returns its (x, v) as torch tensors on its device
(``drone_mppi.py:169-176``; the node calls ``xdes.to('cpu').tolist()``, ``drone.py:240``).
The engine's outputs land in host memory, so each call needs one host-to-device copy.
``OutputRing`` makes it ONE non-blocking copy of all the outputs into a fresh device
tensor per call, from a ring of pinned staging rows: a row is reused only after its copy
has run (its event; by then a whole control step has passed, so the wait is a no-op).
Two synchronous ``torch.tensor(..., device=cuda)`` copies per call used to sit on the
control step's latency path.
"""
from __future__ import annotations

import threading
from typing import Optional

import numpy as np
import torch

from .. import _capi as capi
from ..engine import Engine, Limits, Scene, SelfCollision, check_shift, cost_term_bits, make_config


class OutputRing:
    def __init__(self, device: torch.device, width: int, depth: int = 8):
        self.device, self.width = device, width
        self._host = None
        self._events = None
        self._used = [False] * depth
        self._depth = depth
        self._i = 0

    def to_device(self, row: np.ndarray) -> torch.Tensor:
        """A fresh float32 tensor on ``device`` holding ``row`` (stream-ordered on the
        current stream; CPU devices get a host tensor)."""
        if self.device.type != "cuda":
            return torch.tensor(np.asarray(row, np.float32))
        if self._host is None:
            self._host = torch.zeros((self._depth, self.width), dtype=torch.float32).pin_memory()
            self._events = [torch.cuda.Event() for _ in range(self._depth)]
        i = self._i
        self._i = (i + 1) % self._depth
        if self._used[i]:
            self._events[i].synchronize()
        self._host[i].numpy()[:] = row
        t = torch.empty(self.width, dtype=torch.float32, device=self.device)
        t.copy_(self._host[i], non_blocking=True)
        self._events[i].record()
        self._used[i] = True
        return t


class _Cleared:
    """SolverBase._field_data after clear_distance_field: cleared, and distinct from the clear before it."""


class SolverBase:
    """A class gives: ``_horizon_attr`` (the name of its horizon attribute), ``_config(key)`` (the
    engine's config for a reuse key) and, in its control call, the reuse key itself: the engine is
    rebuilt when the key differs from the one it was made for."""

    _horizon_attr = "n_horizon"

    def __init__(self, n_action: int, horizon: int, device: Optional[int], noise: str, seed: int,
                 verbose: bool, prewarm_us: int):
        self.device = torch.device(f"cuda:{device or 0}" if torch.cuda.is_available() else "cpu")
        self._dev_index = device or 0
        self.n_action = n_action
        self.dt = 0.01
        self.u = torch.zeros(n_action)
        self.verbose = verbose
        self._noise, self._seed = noise, seed
        self._prewarm_us = int(prewarm_us)
        self._lock = threading.Lock()
        self._engine: Optional[Engine] = None
        self._engine_key = None                # the reuse key _engine was made for
        self._u_prev_host = np.zeros((horizon, n_action), np.float32)
        self._last_target = None               # (engine, target bytes) last written (_sync_target)

    # ------------------------------------------------------------------ u
    # The reference's ``u`` attribute (``self.u = u[0].clone()``, mppi.py:155 /
    # drone_mppi.py:163): a torch tensor, built on its first read after each call from the
    # call's own u0 row, so a controller that never reads it does not pay a
    # ``torch.from_numpy`` (~1 us) per control call.  Assigning ``u`` stores the tensor.
    _u_t = None
    _u_np = None

    @property
    def u(self):
        t = self._u_t
        if t is None:
            t = self._u_t = torch.from_numpy(self._u_np)
        return t

    @u.setter
    def u(self, value):
        self._u_t = value
        self._u_np = None

    def _set_u0(self, row: np.ndarray) -> None:
        """row: this call's u0 (a fresh array the engine returned, owned from here on)."""
        self._u_np = row
        self._u_t = None

    def _after_step(self, u0, stats):
        """What a control call keeps of eng.step's answer: u0 (as _set_u0) and the stats."""
        self._u_np = u0[0]
        self._u_t = None
        st = self.last_stats = stats[0]
        return st

    # -------------------------------------------------------------- engine
    def _ensure_engine(self, key) -> Engine:
        """The engine made for ``key``: the one at hand, or a new one that takes over the warm
        start (and the prewarm window, mppi_set_prewarm: for a loop ticking with idle gaps)."""
        e = self._engine
        full_key = (key, self._scene, self._field)   # (the scene and the field's grid are fixed per engine)
        if self._self_collision is not None:
            full_key += (self._self_collision,)       # (and the pair list)
        if self._limits is not None:
            full_key += ("limits",)                   # (that an engine is bounded; the values are replaceable)
        if e is not None and full_key == self._engine_key:
            return e
        u = self._u_prev_host if e is None else e.get_u_prev()[0]
        if e is not None:
            sent = self._field_sent
            if self._field is not None and self._map_live and sent is not None and sent[0] is e and sent[1] is self._field_data:
                # the map built on the device moves to the new engine (nothing newer from the user waits)
                fd = e.get_distance_field()
                self._field_data = (e.get_occupancy(), None if fd is None else fd[1], self._map_max_dist)
            e.close()
        cfg = self._config(key)
        scene = Scene.default(cfg) if self._scene is True else self._scene
        if self._self_collision is not None:   # True: the placeholder pairs of the scene (engine.SelfCollision.default)
            if scene is None:
                scene = Scene.default(cfg)
            pairs = SelfCollision.default(cfg, scene) if self._self_collision is True else self._self_collision
            e = self._engine = Engine(cfg, scene=scene, field=self._field, self_collision=pairs)
        elif self._limits is not None:   # True: the default bounds of the config (engine.Limits.default)
            if self._limits is True:
                self._limits = Limits.default(cfg)
            e = self._engine = Engine(cfg, limits=self._limits)
            self._limits_sent = (e, self._limits)
        else:
            e = self._engine = Engine(cfg) if scene is None and self._field is None else Engine(cfg, scene=scene, field=self._field)
        self._engine_key = full_key
        e.set_u_prev(u)
        if self._prewarm_us:
            e.set_prewarm(self._prewarm_us)
        return e

    @property
    def u_prev(self) -> torch.Tensor:
        if self._engine is None:
            return torch.from_numpy(self._u_prev_host.copy())
        return torch.from_numpy(self._engine.get_u_prev()[0])

    @u_prev.setter
    def u_prev(self, value):
        u = np.ascontiguousarray(torch.as_tensor(value).detach().cpu().numpy(), np.float32)
        self._u_prev_host = u.reshape(getattr(self, self._horizon_attr), self.n_action).copy()
        if self._engine is not None:
            self._engine.set_u_prev(self._u_prev_host)

    def _sync_target(self, eng: Engine, pos: np.ndarray, quat: Optional[np.ndarray] = None) -> None:
        """The target into the engine when its bytes changed since the last call (the control
        call's host time: a target write rebuilds the vehicle constants through one more C call)."""
        key = pos.tobytes() if quat is None else pos.tobytes() + quat.tobytes()
        last = self._last_target
        if last is None or last[0] is not eng or last[1] != key:
            eng.set_target(pos, quat)
            self._last_target = (eng, key)

    # ------------------------------------------------- target trajectory
    # ``track_target=True`` (a constructor switch of the three classes) makes the engine a
    # ``target_track`` one: the pose target may move along the horizon.  While no table is set the
    # control call keeps pushing the class's fixed target, which a clear table follows.
    _track_target = False
    _target_rows = None    # (pos (H,3), quat (H,4) or None) of set_target_trajectory; None: clear
    _rows_sent = None      # (engine, rows) last written (_sync_target_rows)

    def _track_bits(self, cost_terms=0) -> int:
        return cost_term_bits(cost_terms) | (capi.COST_TARGET_TRACK if self._track_target else 0)

    def set_target_trajectory(self, poses) -> None:
        """One pose per horizon step: (H, 7) rows xyz + quaternion xyzw, or (H, 3) positions (the
        drone classes; the arm then keeps ``target_pose``'s orientation on every row).  Row t is the
        pose wanted at horizon index t, (t + 1) dt from now.  Used from the next control call on."""
        if not self._track_target:
            raise RuntimeError("set_target_trajectory needs track_target=True at construction")
        a = np.ascontiguousarray(poses, np.float32)
        H = getattr(self, self._horizon_attr)
        if a.shape == (H, 7):
            self._target_rows = (a[:, :3].copy(), a[:, 3:].copy())
        elif a.shape == (H, 3):
            self._target_rows = (a.copy(), None)
        else:
            raise ValueError(f"target trajectory of shape {a.shape}: ({H}, 7) or ({H}, 3)")

    def clear_target_trajectory(self) -> None:
        """Back to the fixed target (``target_pose`` / ``target``) on every horizon step."""
        if not self._track_target:
            raise RuntimeError("clear_target_trajectory needs track_target=True at construction")
        self._target_rows = None

    def _sync_target_rows(self, eng: Engine) -> None:
        """The table into the engine when it changed since the last call (after _sync_target: a
        clear table follows the fixed target)."""
        if not self._track_target:
            return
        rows, sent = self._target_rows, self._rows_sent
        if sent is None or sent[0] is not eng or sent[1] is not rows:
            if rows is None:
                eng.set_target_trajectory(None)
            else:
                eng.set_target_trajectory(rows[0], rows[1])
            self._rows_sent = (eng, rows)

    # ------------------------------------------------------------ obstacles
    # ``scene=`` (a constructor keyword of the arm and drone classes): an ``engine.Scene``, or True for
    # the project's placeholder spheres (``Scene.default``), makes the engine an obstacle-avoiding one.
    _scene = None
    _obstacles = None      # (centers, radii, velocities) of set_obstacles; None: none
    _obs_sent = None       # (engine, obstacles) last written (_sync_obstacles)

    def set_obstacles(self, centers, radii, velocities=None) -> None:
        """Sphere obstacles (``Engine.set_obstacles``): (n, 3) centres now, (n,) radii, (n, 3)
        velocities or None.  Used from the next control call on, until set or cleared again."""
        if self._scene is None:
            raise RuntimeError("set_obstacles needs scene=... at construction")
        c = np.ascontiguousarray(centers, np.float32).reshape(-1, 3).copy()
        r = np.ascontiguousarray(radii, np.float32).reshape(-1).copy()
        w = None if velocities is None else np.ascontiguousarray(velocities, np.float32).reshape(-1, 3).copy()
        self._obstacles = (c, r, w)

    def clear_obstacles(self) -> None:
        if self._scene is None:
            raise RuntimeError("clear_obstacles needs scene=... at construction")
        self._obstacles = None

    # ``limits=`` (a constructor keyword of the quadrotor and aerial classes): an ``engine.Limits``, or True for the
    # default bounds (thrust within [0, 2 m g]), makes the engine a bounded one.  That is fixed at construction;
    # the values are not.
    _limits = None
    _limits_sent = None    # (engine, limits) last written (_sync_limits)

    def set_limits(self, limits) -> None:
        """The rotor limits (``Engine.set_limits``): an ``engine.Limits``.  Used from the next control call on."""
        if self._limits is None:
            raise RuntimeError("set_limits needs limits=... at construction")
        if not isinstance(limits, Limits):
            raise TypeError("set_limits takes an engine.Limits")
        self._limits = limits

    def get_limits(self):
        """The rotor limits in use (True until the first control call has made the engine, when they were left to
        the default), or None without ``limits=``."""
        return self._limits

    def _sync_limits(self, eng: Engine) -> None:
        lim, sent = self._limits, self._limits_sent
        if lim is not None and (sent is None or sent[0] is not eng or sent[1] is not lim):
            eng.set_limits(lim)
            self._limits_sent = (eng, lim)

    # ``self_collision=`` (a constructor keyword of the arm class): an ``engine.SelfCollision``, or True for
    # the placeholder pairs, makes the engine a self engine (with ``scene``, or the placeholder spheres).
    _self_collision = None

    def get_self_clearances(self) -> np.ndarray:
        """(K,): the last control call's samples' min clearances over the self-collision pairs
        (``Engine.get_self_clearances``)."""
        if self._self_collision is None:
            raise RuntimeError("get_self_clearances needs self_collision=... at construction")
        if self._engine is None:
            raise RuntimeError("get_self_clearances: no control call yet")
        return self._engine.get_self_clearances()[0]

    # ``field=`` (a constructor keyword of the arm and drone classes): an ``engine.DistanceField`` makes
    # the engine a field engine (with ``scene``, or the placeholder spheres); its data, when it has some,
    # is the field until set_distance_field / clear_distance_field.
    _field = None
    _field_data = None     # (d, origin or None) of set_distance_field, (occ, origin or None, max_dist) of set_occupancy; None: cleared
    _field_sent = None     # (engine, data) last written (_sync_field)

    def set_distance_field(self, d, origin=None) -> None:
        """The distance field (``Engine.set_distance_field``): (nz, ny, nx) metres, negative inside;
        ``origin`` moves node (0, 0, 0).  Used from the next control call on."""
        if self._field is None:
            raise RuntimeError("set_distance_field needs field=... at construction")
        o = None if origin is None else np.ascontiguousarray(origin, np.float32).reshape(3).copy()
        self._field_data = (self._field.check(d).copy(), o)

    def set_occupancy(self, occ, origin=None, max_dist=None) -> None:
        """The distance field of an occupancy grid, built on the device (``Engine.set_occupancy``):
        (nz, ny, nx) bool or uint8, nonzero = occupied.  Used from the next control call on."""
        if self._field is None:
            raise RuntimeError("set_occupancy needs field=... at construction")
        o = None if origin is None else np.ascontiguousarray(origin, np.float32).reshape(3).copy()
        self._field_data = (self._field.check_occupancy(occ).copy(), o, max_dist)

    # The engine's occupancy map (Engine.integrate_depth, shift_map, get_occupancy) lives on the device.  Map
    # calls made before the first control call has made the engine wait in _map_ops and run, in order, right
    # after the field data is written.  A call is checked before it is queued (the view and max_dist by
    # mppi_integrate_depth's own argument check, the shift's range here), and an op leaves the queue before
    # it runs: one the engine still refuses raises once, to whoever synchronises next, and is gone -- the ops
    # behind it run at the next synchronise, none runs twice.  When a new engine replaces the old one, the
    # old one's map goes with it as an occupancy grid (_ensure_engine) as long as the map is what the field
    # was last built from: a set_distance_field, set_occupancy or clear_distance_field made since wins.
    _map_ops = ()          # pending (name, args) map calls
    _map_live = False      # the engine's map holds more than _field_data says
    _map_max_dist = None

    def _map_call(self, name, *args) -> None:
        with self._lock:
            self._map_ops = tuple(self._map_ops) + ((name, args),)
            if self._engine is not None:
                self._sync_field(self._engine)

    @staticmethod
    def _check_max_dist(max_dist) -> None:
        if max_dist is not None and (np.isnan(max_dist) or max_dist == np.inf):
            raise ValueError(f"max_dist {max_dist}: a finite cap, or None / <= 0 for none")

    def integrate_depth(self, depth, view, max_dist=None) -> None:
        """One depth image into the occupancy map, on the device (``Engine.integrate_depth``): ``depth``
        (height, width) float32 metres, ``view`` an ``engine.DepthView``.  Used from the next control call on.
        A view or ``max_dist`` the engine would refuse raises here and nothing is queued."""
        if self._field is None:
            raise RuntimeError("integrate_depth needs field=... at construction")
        view.validate(self._field, max_dist)
        self._map_call("integrate_depth", view.check_image(depth).copy(), view, max_dist)

    def shift_map(self, shift, max_dist=None) -> None:
        """Moves the map's window by ``shift`` nodes (``Engine.shift_map``)."""
        if self._field is None:
            raise RuntimeError("shift_map needs field=... at construction")
        self._check_max_dist(max_dist)
        self._map_call("shift_map", tuple(check_shift(shift)), max_dist)

    def get_occupancy(self):
        """The occupancy map the engine holds (``Engine.get_occupancy``), or None before the first control
        call has made the engine."""
        if self._field is None:
            raise RuntimeError("get_occupancy needs field=... at construction")
        with self._lock:
            if self._engine is None:
                return None
            self._sync_field(self._engine)
            return self._engine.get_occupancy()

    def get_distance_field(self):
        """``(d, origin)`` of the field the engine holds (``Engine.get_distance_field``), or None while it
        is cleared or before the first control call has made the engine."""
        if self._field is None:
            raise RuntimeError("get_distance_field needs field=... at construction")
        if self._engine is None:
            return None
        self._sync_field(self._engine)
        return self._engine.get_distance_field()

    def clear_distance_field(self) -> None:
        if self._field is None:
            raise RuntimeError("clear_distance_field needs field=... at construction")
        self._field_data = _Cleared()   # (a fresh object: a clear after map calls built a field is a change too)

    def _init_field(self, field) -> None:
        self._field = field
        self._field_data = None if field is None or field.d is None else (field.d, None)

    def _sync_field(self, eng: Engine) -> None:
        if self._field is None:
            return
        data, sent = self._field_data, self._field_sent
        if sent is None or sent[0] is not eng or sent[1] is not data:
            if data is None or isinstance(data, _Cleared):
                eng.clear_distance_field()
            elif len(data) == 3:   # (occ, origin, max_dist) of set_occupancy
                eng.set_occupancy(*data)
            else:
                eng.set_distance_field(*data)
            self._field_sent = (eng, data)
            self._map_live = False
        while self._map_ops:
            (name, args), self._map_ops = self._map_ops[0], tuple(self._map_ops[1:])   # (gone before it can raise)
            getattr(eng, name)(*args)
            self._map_live, self._map_max_dist = True, args[-1]

    def _sync_obstacles(self, eng: Engine) -> None:
        self._sync_field(eng)
        if self._scene is None:
            return
        obs, sent = self._obstacles, self._obs_sent
        if sent is None or sent[0] is not eng or sent[1] is not obs:
            if obs is None:
                eng.set_obstacles(None)
            else:
                eng.set_obstacles(*obs)
            self._obs_sent = (eng, obs)

    def compute_weights(self, S: torch.Tensor, _lambda) -> torch.Tensor:
        """mppi.py:173-193 / drone_mppi.py:111-130 (host helper; the engine computes the same
        weights on device)."""
        rho = S.min()
        scaled_S = (-1.0 / _lambda) * (S - rho)
        return torch.exp(scaled_S) / torch.exp(scaled_S).sum()

    # ------------------------------------------------------- build extras
    def get_trajectory(self) -> np.ndarray:
        """(K,H,C) of the last step: the arm's q_samples (7) and EE 4x4 (16); the drone's xyz; the
        quadrotor's xyz, rpy (the commented loop's trajectory)."""
        return self._engine.get_trajectory()[0]

    def get_plan(self):
        """The nominal plan: the zero-noise rollout of u_prev from the last state (engine.Plan of
        vehicle 0: traj (H,C), cost_t (H), pos_err (H), S, ee_path (H,3), first_reach(tol))."""
        return self._engine.get_plan().vehicle(0)

    def get_elites(self, n=16):
        """The n lowest-cost sampled rollouts of the last step, best first (engine.Elites of vehicle 0:
        idx (n), S (n), w (n), traj (n,H,C) in get_trajectory()'s layout, ee_path (n,H,3))."""
        return self._engine.get_elites(n).vehicle(0)

    def get_costs(self) -> np.ndarray:
        return self._engine.get_costs()[0]


class VehicleSolver(SolverBase):
    """The drone solver's body for a state (x, v) of ``width`` numbers each; the class's
    ``_config(key)`` names its model (``_vehicle_config``)."""

    _horizon_attr = "n_timestep"

    def __init__(self, width: int, sigma: torch.Tensor, n_samples: int, n_timestep: int, *base_args,
                 track_target: bool = False, scene=None, field=None, limits=None):
        super().__init__(sigma.shape[0], n_timestep, *base_args)
        self._track_target = bool(track_target)
        self._scene = scene
        self._limits = limits
        self._init_field(field)
        self.n_samples = n_samples
        self.n_timestep = n_timestep
        self.x_prev = torch.zeros(width)
        self.v_prev = torch.zeros(width)
        self.sigma = sigma
        self.param_lambda = 0.1
        self.target = [1.0, 2.0, 3.4]          # drone_mppi.py:141
        self._width = width
        self._row = np.zeros(2 * width, np.float64)        # x + v of the control call
        self._out_ring = OutputRing(self.device, 2 * width)   # (x, v): one async H2D copy per call

    def _vehicle_config(self, model: str, key, **extra):
        return make_config(model, n_samples=self.n_samples, n_horizon=self.n_timestep, dt=self.dt,
                           lam=self.param_lambda, sigma=self.sigma.numpy(), seed=self._seed,
                           noise="injected" if key[0] else self._noise, device=self._dev_index,
                           cost_terms=self._track_bits(), **extra)

    def set_state(self, x, v):
        """drone_mppi.py:179-183 (stored as float32 like the reference)."""
        with self._lock:
            self.x_prev = torch.tensor(np.asarray(x, np.float64), dtype=torch.float32)
            self.v_prev = torch.tensor(np.asarray(v, np.float64), dtype=torch.float32)

    def compute_control_input(self, noise: Optional[np.ndarray] = None):
        row, w = self._row, self._width   # x, v into one preallocated fp64 row (the engine copies it)
        with self._lock:
            row[:w] = self.x_prev.numpy()
            row[w:] = self.v_prev.numpy()
        # the reuse key: unlike the arm's, it holds the sizes, so assigning n_samples or n_timestep
        # after construction rebuilds the engine at the next call
        eng = self._ensure_engine((noise is not None or self._noise == "injected", self.n_samples, self.n_timestep))
        self._sync_target(eng, np.asarray(self.target, np.float32))
        self._sync_target_rows(eng)
        self._sync_obstacles(eng)
        self._sync_limits(eng)
        out, u0, stats = eng.step(row, noise)
        st = self._after_step(u0, stats)   # (u: the tensor is made on first read)
        if self.verbose:
            print("Rho :", torch.tensor(st.rho))
        t = self._out_ring.to_device(out[0])   # (the engine's row is x, v: mppi_output_dim)
        return t[:w], t[w:]

    def compute_weights(self, S: torch.Tensor) -> torch.Tensor:
        return super().compute_weights(S, self.param_lambda)
