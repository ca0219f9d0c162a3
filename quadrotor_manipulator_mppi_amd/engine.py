"""Python handle on one libmppi_hip.so engine.

Thin host-side plumbing over the C-ABI (``include/mppi_hip.h``): it fills the
config struct, keeps numpy staging arrays, and turns status codes into
exceptions.  All arithmetic of the control step runs in the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _capi as capi
from .robot.urdf_chain import load_chain

MODELS = {"drone": capi.MODEL_DRONE, "arm": capi.MODEL_ARM, "wholebody": capi.MODEL_WHOLEBODY,
          "quadrotor": capi.MODEL_QUADROTOR, "aerial": capi.MODEL_AERIAL}
QUAD_FIELDS = ("quad_mass", "quad_kd", "quad_gravity")
JOINT_TYPES = {"fixed": capi.JOINT_FIXED, "revolute": capi.JOINT_REVOLUTE,
               "continuous": capi.JOINT_REVOLUTE, "prismatic": capi.JOINT_PRISMATIC}


@dataclass(slots=True)
class StepStats:
    rho: float
    eta: float
    ess: float
    nonfinite: bool
    reach: bool
    exchange_timeout: bool = False   # a peer-exchange step gave up waiting for a rank (u_prev kept)


@dataclass(slots=True)
class Plan:
    """The nominal plan (``Engine.get_plan``): the zero-noise rollout of the warm start ``u_prev``
    from the current state.  Arrays are per vehicle, ``(V, ...)``; ``vehicle(v)`` drops that axis."""
    traj: np.ndarray      # (V, H, C): the per-(t) layout of get_trajectory
    cost_t: np.ndarray    # (V, H): each step's share of S
    pos_err: np.ndarray   # (V, H): L1 distance of the EE / vehicle position to the target
    S: np.ndarray         # (V,)
    ee_path: np.ndarray   # (V, H, 3): the EE (arm, whole-body) or vehicle (drone, quadrotor) positions
    clearance: Optional[np.ndarray] = None   # (V, H): min clearance to the obstacles at each step (scene engines)
    self_clearance: Optional[np.ndarray] = None   # (V, H): min clearance over the self-collision pairs (self engines)

    def first_reach(self, tol: float = 0.005):
        """The first t with pos_err < tol (check_reach's measure), -1 if none: per vehicle."""
        hit = self.pos_err < tol
        t = np.where(hit.any(axis=-1), hit.argmax(axis=-1), -1)
        return int(t) if t.ndim == 0 else t

    def vehicle(self, v: int = 0) -> "Plan":
        return Plan(self.traj[v], self.cost_t[v], self.pos_err[v], self.S[v], self.ee_path[v],
                    None if self.clearance is None else self.clearance[v],
                    None if self.self_clearance is None else self.self_clearance[v])


@dataclass(slots=True)
class Elites:
    """The n lowest-cost sampled rollouts of the last step (``Engine.get_elites``), best first:
    ascending in (cost, index) -- ``np.argsort(S[v], kind="stable")[:n]``.  Arrays are per vehicle,
    ``(V, n, ...)``; ``vehicle(v)`` drops that axis."""
    idx: np.ndarray                 # (V, n) int32: sample index within the engine's K
    S: np.ndarray                   # (V, n): get_costs()[v, idx]
    w: np.ndarray                   # (V, n): get_weights()[v, idx]
    traj: Optional[np.ndarray]      # (V, n, H, C): get_trajectory()[v, idx]; None when not asked for
    ee_path: Optional[np.ndarray]   # (V, n, H, 3): the EE (arm, whole-body) or vehicle positions

    def vehicle(self, v: int = 0) -> "Elites":
        return Elites(self.idx[v], self.S[v], self.w[v], None if self.traj is None else self.traj[v],
                      None if self.ee_path is None else self.ee_path[v])


@dataclass
class Scene:
    """The sphere scene of an obstacle-avoiding engine (``Engine(cfg, scene=...)``, mppi_create_scene):
    the robot's body spheres -- ``(frame, (ox, oy, oz), radius)``, frame an index into the config's
    chain joints (-1: the base transform; the only frame of a drone) -- and the term's weights
    (project constants: w_obs = 100, margin = 0.05 m, penalty = 1e4).  Hashable by value, so it can be
    part of an engine key."""
    body: tuple = ()
    w_obs: float = 100.0
    margin: float = 0.05
    penalty: float = 1e4

    def __post_init__(self):
        self.body = tuple((int(f), tuple(float(x) for x in o), float(r)) for f, o, r in self.body)

    def __hash__(self):
        return hash((self.body, self.w_obs, self.margin, self.penalty))

    @staticmethod
    def default(cfg: capi.Config) -> "Scene":
        """The project's placeholder spheres for the config's model and chain (mppi_scene_default)."""
        c = capi.Scene()
        capi.lib().mppi_scene_default(C.byref(c), C.byref(cfg))
        return Scene.from_c(c)

    @staticmethod
    def from_c(c: capi.Scene) -> "Scene":
        return Scene(tuple((c.body[i].frame, tuple(c.body[i].offset), c.body[i].radius) for i in range(c.n_body)),
                     c.w_obs, c.margin, c.penalty)

    def to_c(self) -> capi.Scene:
        if len(self.body) > capi.MAX_BODY_SPHERES:
            raise ValueError(f"{len(self.body)} body spheres (max {capi.MAX_BODY_SPHERES})")
        c = capi.Scene()
        c.n_body = len(self.body)
        for i, (f, o, r) in enumerate(self.body):
            c.body[i].frame, c.body[i].radius = f, r
            c.body[i].offset[:] = o
        c.w_obs, c.margin, c.penalty = self.w_obs, self.margin, self.penalty
        return c


class Limits:
    """The rotor limits of a bounded engine (``Engine(cfg, limits=...)``, mppi_create_limits; quadrotor and
    aerial): ``thrust=(lo, hi)`` [N] and ``torque=((lo, hi),) * 3`` [N m] about x, y, z -- action dims 0..3.
    ``-inf`` / ``+inf`` leave a side open.  Whether an engine has limits is fixed at creation; the values can
    be replaced with ``Engine.set_limits``.  Hashable by value."""

    def __init__(self, thrust=(-np.inf, np.inf), torque=((-np.inf, np.inf),) * 3):
        t = tuple(torque)
        if len(t) != 3 or len(tuple(thrust)) != 2 or any(len(tuple(x)) != 2 for x in t):
            raise ValueError("limits: thrust=(lo, hi) and torque=((lo, hi),) * 3")
        self.thrust = tuple(float(x) for x in thrust)
        self.torque = tuple(tuple(float(x) for x in pair) for pair in t)

    @property
    def lo(self) -> np.ndarray:
        return np.float32([self.thrust[0]] + [p[0] for p in self.torque])

    @property
    def hi(self) -> np.ndarray:
        return np.float32([self.thrust[1]] + [p[1] for p in self.torque])

    def _key(self):
        return (self.thrust, self.torque)

    def __eq__(self, other):
        return isinstance(other, Limits) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"Limits(thrust={self.thrust}, torque={self.torque})"

    @staticmethod
    def default(cfg: capi.Config) -> "Limits":
        """Thrust within [0, 2 m g] of the config's quad_mass and quad_gravity, the torques unbounded
        (mppi_limits_default)."""
        c = capi.Limits()
        capi.lib().mppi_limits_default(C.byref(c), C.byref(cfg))
        return Limits.from_c(c)

    @staticmethod
    def from_c(c: capi.Limits) -> "Limits":
        return Limits((c.lo[0], c.hi[0]), tuple((c.lo[a], c.hi[a]) for a in (1, 2, 3)))

    def to_c(self) -> capi.Limits:
        c = capi.Limits()
        c.lo[:] = [float(x) for x in self.lo]
        c.hi[:] = [float(x) for x in self.hi]
        return c


def limits_apply(limits: "Limits", u, eps):
    """The limits' arithmetic on the host (mppi_limits_apply: the kernels' own inline, no GPU): ``u`` (H, 4)
    and ``eps`` (K, H, 4) float32 into ``(eps_eff, ctl)``, each (K, H, 4)."""
    u = np.ascontiguousarray(u, np.float32)
    eps = np.ascontiguousarray(eps, np.float32)
    K, H = eps.shape[0], eps.shape[1]
    if u.shape != (H, 4) or eps.shape != (K, H, 4):
        raise ValueError(f"limits_apply: u {u.shape} and eps {eps.shape}, expected (H, 4) and (K, H, 4)")
    e, c = np.empty_like(eps), np.empty_like(eps)
    lc = limits.to_c()
    capi.check(capi.lib().mppi_limits_apply(C.byref(lc), capi.fptr(u), capi.fptr(eps), K, H, capi.fptr(e), capi.fptr(c)),
               "mppi_limits_apply")
    return e, c


class SelfCollision:
    """The self-collision pairs of a self engine (``Engine(cfg, scene=..., self_collision=...)``,
    mppi_create_scene_self): up to 32 unordered pairs ``(a, b)`` of the scene's body spheres, indexed as in
    ``Scene.body``, and the term's own weights (project constants: w_self = 100, margin = 0.02 m,
    penalty = 1e4).  Fixed at creation; hashable by value, so it can be part of an engine key."""

    def __init__(self, pairs=(), w_self: float = 100.0, margin: float = 0.02, penalty: float = 1e4):
        self.pairs = tuple((int(a), int(b)) for a, b in pairs)
        self.w_self, self.margin, self.penalty = float(w_self), float(margin), float(penalty)

    def _key(self):
        return (self.pairs, self.w_self, self.margin, self.penalty)

    def __eq__(self, other):
        return isinstance(other, SelfCollision) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"SelfCollision(pairs={self.pairs}, w_self={self.w_self}, margin={self.margin}, penalty={self.penalty})"

    @staticmethod
    def default(cfg: capi.Config, scene: Optional["Scene"] = None) -> "SelfCollision":
        """The project's placeholder pairs for a config and a scene (None: ``Scene.default(cfg)``): every
        pair with at least three moving joints between its frames (mppi_self_collision_default)."""
        c = capi.SelfCollision()
        sc = None if scene is None else scene.to_c()
        capi.lib().mppi_self_collision_default(C.byref(c), C.byref(cfg), None if sc is None else C.byref(sc))
        return SelfCollision(tuple((c.pair[i][0], c.pair[i][1]) for i in range(c.n_pairs)), c.w_self, c.margin, c.penalty)

    def to_c(self) -> capi.SelfCollision:
        if len(self.pairs) > capi.MAX_SELF_PAIRS:
            raise ValueError(f"{len(self.pairs)} self-collision pairs (max {capi.MAX_SELF_PAIRS})")
        c = capi.SelfCollision()
        c.n_pairs = len(self.pairs)
        for i, (a, b) in enumerate(self.pairs):
            c.pair[i][0], c.pair[i][1] = a, b
        c.w_self, c.margin, c.penalty = self.w_self, self.margin, self.penalty
        return c


class DistanceField:
    """The voxel signed distance field of a field engine (``Engine(cfg, field=...)``,
    mppi_create_scene_field): ``dims`` = (nx, ny, nz) nodes, ``voxel`` in metres, ``origin`` the world
    position of node (0, 0, 0).  ``d`` (nz, ny, nx) float32, metres, negative inside -- None: the
    engine starts with the field cleared.  Points outside the grid read the clamped position's
    value, so pad the grid."""

    def __init__(self, dims, voxel: float, origin=(0.0, 0.0, 0.0), d=None):
        self.dims = tuple(int(n) for n in dims)
        self.voxel = float(voxel)
        self.origin = tuple(float(x) for x in origin)
        if len(self.dims) != 3 or len(self.origin) != 3:
            raise ValueError("dims and origin have three entries (x, y, z)")
        self.d = None if d is None else self.check(d)

    @property
    def shape(self):
        return self.dims[::-1]   # (nz, ny, nx)

    def check(self, d) -> np.ndarray:
        d = np.ascontiguousarray(d, np.float32)
        if d.shape != self.shape:
            raise ValueError(f"field data {d.shape}, expected (nz, ny, nx) = {self.shape}")
        return d

    def nodes(self):
        """The nodes' world coordinates X, Y, Z, each (nz, ny, nx), float64."""
        ax = [self.origin[a] + self.voxel * np.arange(self.dims[a], dtype=np.float64) for a in range(3)]
        Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        return X, Y, Z

    def to_c(self) -> capi.FieldDesc:
        c = capi.FieldDesc()
        c.dims[:] = self.dims
        c.voxel = self.voxel
        c.origin[:] = self.origin
        return c

    @staticmethod
    def from_function(fn, dims, voxel, origin=(0.0, 0.0, 0.0)) -> "DistanceField":
        """``fn(X, Y, Z) -> d``, vectorised over the nodes' world coordinates."""
        f = DistanceField(dims, voxel, origin)
        f.d = f.check(np.asarray(fn(*f.nodes()), np.float64))
        return f

    @staticmethod
    def from_boxes(boxes, dims, voxel, origin=(0.0, 0.0, 0.0)) -> "DistanceField":
        """The exact SDF of a union of axis-aligned boxes ``(lo3, hi3)``: the min over the boxes."""
        def sdf(X, Y, Z):
            P = np.stack([X, Y, Z], -1)
            out = np.full(X.shape, np.inf)
            for lo, hi in boxes:
                lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
                q = np.abs(P - 0.5 * (lo + hi)) - 0.5 * (hi - lo)
                out = np.minimum(out, np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0))
            return out
        return DistanceField.from_function(sdf, dims, voxel, origin)

    def check_occupancy(self, occ) -> np.ndarray:
        """An occupancy grid of this field's shape as the uint8 bytes the library takes (nonzero = occupied)."""
        occ = np.asarray(occ)
        if occ.dtype != np.bool_ and occ.dtype != np.uint8:
            raise TypeError(f"occupancy of dtype {occ.dtype}: bool or uint8")
        if occ.shape != self.shape:
            raise ValueError(f"occupancy {occ.shape}, expected (nz, ny, nx) = {self.shape}")
        return np.ascontiguousarray(occ).view(np.uint8)

    @staticmethod
    def from_occupancy(occ, dims, voxel, origin=(0.0, 0.0, 0.0), max_dist=None) -> "DistanceField":
        """The field of an occupancy grid (nz, ny, nx), bool or uint8, by the host helper
        (mppi_occupancy_field): what ``Engine.set_occupancy`` builds on the device, bit for bit, without one."""
        f = DistanceField(dims, voxel, origin)
        occ = f.check_occupancy(occ)
        d = np.empty(f.shape, np.float32)
        desc = f.to_c()
        capi.check(capi.lib().mppi_occupancy_field(C.byref(desc), occ.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                   0.0 if max_dist is None else float(max_dist), capi.fptr(d)),
                   "mppi_occupancy_field")
        f.d = d
        return f


@dataclass
class DepthView:
    """One depth image's camera (mppi_depth_view): the pinhole intrinsics in pixels, the range gate, the
    pose of the optical frame (z forward, x right, y down) in the world, and which pixels are used (rows
    and columns 0, stride, 2 stride, ...).  ``carve=False`` marks end points only."""
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    pos: Sequence[float] = (0.0, 0.0, 0.0)
    quat_xyzw: Sequence[float] = (0.0, 0.0, 0.0, 1.0)
    z_min: float = 0.1
    z_max: float = 5.0
    stride: int = 1
    carve: bool = True

    def to_c(self) -> capi.DepthViewC:
        c = capi.DepthViewC()
        c.width, c.height, c.stride, c.carve = int(self.width), int(self.height), int(self.stride), int(bool(self.carve))
        c.fx, c.fy, c.cx, c.cy = float(self.fx), float(self.fy), float(self.cx), float(self.cy)
        c.z_min, c.z_max = float(self.z_min), float(self.z_max)
        pos, quat = np.asarray(self.pos, np.float64).reshape(3), np.asarray(self.quat_xyzw, np.float64).reshape(4)
        c.pos[:] = [float(x) for x in pos]
        c.quat_xyzw[:] = [float(x) for x in quat]
        return c

    def validate(self, field: "DistanceField", max_dist=None) -> None:
        """Raises what ``Engine.integrate_depth`` would raise for this view on an engine with ``field``
        (mppi_integrate_depth's argument check, without a device or an image)."""
        f = capi.lib().mppi_debug_depth_validate
        f.restype, f.argtypes = capi.DEBUG_PROTOTYPES["mppi_debug_depth_validate"]
        desc, v = field.to_c(), self.to_c()
        capi.check(f(C.byref(desc), C.byref(v), 0.0 if max_dist is None else float(max_dist)), "integrate_depth")

    def check_image(self, depth) -> np.ndarray:
        """``depth`` as the (height, width) float32 metres the library takes."""
        d = np.ascontiguousarray(depth, np.float32)
        if d.shape != (int(self.height), int(self.width)):
            raise ValueError(f"depth image {d.shape}, expected (height, width) = {(int(self.height), int(self.width))}")
        return d

    @staticmethod
    def from_camera_info(K, width, height, pos=(0.0, 0.0, 0.0), quat_xyzw=(0.0, 0.0, 0.0, 1.0), z_min=0.1, z_max=5.0,
                         stride=1, carve=True) -> "DepthView":
        """From a ``sensor_msgs/CameraInfo``'s K (9 values, row major): fx = K[0], fy = K[4], cx = K[2], cy = K[5]."""
        K = np.asarray(K, np.float64).reshape(9)
        return DepthView(int(width), int(height), float(K[0]), float(K[4]), float(K[2]), float(K[5]), tuple(pos),
                         tuple(quat_xyzw), float(z_min), float(z_max), int(stride), bool(carve))


def check_shift(shift):
    """``shift`` as three ints that fit mppi_shift_map's int32 (a value outside would wrap to another shift)."""
    s = [int(x) for x in shift]
    if len(s) != 3 or any(x < -2 ** 31 or x > 2 ** 31 - 1 for x in s):
        raise ValueError(f"shift {tuple(s)}: three node counts (sx, sy, sz) within int32")
    return s


def depth_integrate_host(field: "DistanceField", occ, depth, view: DepthView) -> np.ndarray:
    """One depth image into an occupancy map on the host (mppi_depth_integrate_host): what
    ``Engine.integrate_depth`` does to the device map, bit for bit, without a device.  ``occ`` (nz, ny, nx)
    bool or uint8 is not modified; the new map is returned as uint8 0 / 1."""
    out = field.check_occupancy(occ).copy()
    d = view.check_image(depth)
    desc, v = field.to_c(), view.to_c()
    capi.check(capi.lib().mppi_depth_integrate_host(C.byref(desc), C.byref(v), capi.fptr(d),
                                                    out.ctypes.data_as(C.POINTER(C.c_uint8))), "mppi_depth_integrate_host")
    return out


def fill_joints(cfg: capi.Config, chain: Sequence[Dict]) -> None:
    if len(chain) > capi.MAX_JOINTS:
        raise ValueError(f"chain has {len(chain)} joints (max {capi.MAX_JOINTS})")
    cfg.n_joints = len(chain)
    for i, j in enumerate(chain):
        J = cfg.joints[i]
        J.type = JOINT_TYPES.get(j["type"], capi.JOINT_FIXED)
        J.q_index = int(j.get("q_index", -1))
        for d in range(3):
            J.xyz[d] = float(j["xyz"][d])
            J.rpy[d] = float(j["rpy"][d])
        ax = j.get("axis")
        J.has_axis = 0 if ax is None else 1
        if ax is not None:
            for d in range(3):
                J.axis[d] = float(ax[d])


def make_config(model: str = "arm", n_samples: Optional[int] = None, n_horizon: Optional[int] = None,
                n_vehicles: int = 1, n_action: Optional[int] = None, dt: float = 0.01, lam: float = 0.1,
                sigma=None, weights: Optional[Sequence[float]] = None, chain=None,
                savgol_window: Optional[int] = None, savgol_order: int = 2, noise: str = "philox",
                seed: int = 0x5EED, device: int = 0, shard_rank: int = 0, shard_count: int = 1,
                state_f64: Optional[bool] = None, store_trajectory: bool = True, store_noise: bool = False,
                check_reach: Optional[bool] = None, reach_tol: float = 0.005, blocks_per_vehicle: int = 0,
                block_threads: int = 0, cost_terms=0, cost_weights: Optional[Dict[str, float]] = None,
                quad: Optional[Dict] = None, vehicle_offset: int = 0) -> capi.Config:
    """``cost_terms``: bitmask of ``capi.COST_*`` or an iterable of names among
    ``covar, center, joint_track, action, joint_limit`` -- the CostManager terms the
    reference ships disabled (cost_manager.py:83-87; ARM and WHOLEBODY) -- and ``target_track`` (every
    model): one pose target per horizon step, ``Engine.set_target_trajectory``.  ``cost_weights`` overrides
    ``w_covar, cost_alpha, cost_gamma, w_center, w_joint_track, w_action,
    joint_limit_penalty``.  ``quad`` overrides the QUADROTOR rigid body: ``quad_mass``,
    ``quad_inertia`` (3,), ``quad_kd``, ``quad_gravity``, ``quad_literal_jinv`` (also the base of the
    ``"aerial"`` model: the quadrotor carrying the Kinova arm, 4 + 7 action dims).  ``vehicle_offset``:
    the fleet-wide index of vehicle 0 (vehicle sharding: the device noise is keyed by it)."""
    L = capi.lib()
    cfg = capi.Config()
    L.mppi_config_default(C.byref(cfg), MODELS[model])
    cfg.n_vehicles = n_vehicles
    if n_samples is not None:
        cfg.n_samples = n_samples
    if n_horizon is not None:
        cfg.n_horizon = n_horizon
    if n_action is not None:
        cfg.n_action = n_action
    cfg.dt, cfg.lambda_ = dt, lam
    A = cfg.n_action
    if sigma is not None:
        s = np.asarray(sigma, np.float32)
        if s.ndim == 1:
            s = np.diag(s)
        if s.shape != (A, A):
            raise ValueError(f"sigma must be ({A},{A})")
        for i in range(A * A):
            cfg.sigma[i] = float(s.reshape(-1)[i])
    if weights is not None:
        cfg.w_stage_pos, cfg.w_stage_ori, cfg.w_term_pos, cfg.w_term_ori = map(float, weights)
    if model in ("arm", "wholebody", "aerial"):
        fill_joints(cfg, chain if chain is not None else load_chain())
    for k, val in (quad or {}).items():
        if k == "quad_inertia":
            for d in range(3):
                cfg.quad_inertia[d] = float(val[d])
        elif k in QUAD_FIELDS:
            setattr(cfg, k, float(val))
        elif k == "quad_literal_jinv":   # drone_mppi.py:73-76 taken literally (inv(J) for t >= 1)
            cfg.quad_literal_jinv = 1 if val else 0
        else:
            raise ValueError(f"unknown quadrotor parameter {k!r}")
    if savgol_window is not None:
        cfg.savgol_window = savgol_window
    cfg.savgol_order = savgol_order
    cfg.noise_mode = capi.NOISE_INJECTED if noise == "injected" else capi.NOISE_PHILOX
    cfg.seed = seed
    cfg.device = device
    cfg.shard_rank, cfg.shard_count = shard_rank, shard_count
    cfg.vehicle_offset = vehicle_offset
    if state_f64 is not None:
        cfg.state_f64 = int(state_f64)
    cfg.store_trajectory = int(store_trajectory)
    cfg.store_noise = int(store_noise)
    if check_reach is not None:
        cfg.check_reach = int(check_reach)
    cfg.reach_tol = reach_tol
    cfg.blocks_per_vehicle = blocks_per_vehicle
    cfg.block_threads = block_threads
    cfg.cost_terms = cost_term_bits(cost_terms)
    for k, val in (cost_weights or {}).items():
        if k not in COST_WEIGHT_FIELDS:
            raise ValueError(f"unknown cost weight {k!r}")
        setattr(cfg, k, float(val))
    return cfg


COST_TERMS = {"covar": capi.COST_COVAR, "center": capi.COST_CENTER, "joint_track": capi.COST_JOINT_TRACK,
              "action": capi.COST_ACTION, "joint_limit": capi.COST_JOINT_LIMIT,
              "target_track": capi.COST_TARGET_TRACK}
COST_WEIGHT_FIELDS = ("w_covar", "cost_alpha", "cost_gamma", "w_center", "w_joint_track", "w_action",
                      "joint_limit_penalty")


def cost_term_bits(terms) -> int:
    if isinstance(terms, int):
        return terms
    bits = 0
    for t in terms:
        if t not in COST_TERMS:
            raise ValueError(f"unknown cost term {t!r} (known: {sorted(COST_TERMS)})")
        bits |= COST_TERMS[t]
    return bits


class Engine:
    """One MPPI engine on one GPU (V vehicles x K samples x H steps)."""

    def __init__(self, cfg: Optional[capi.Config] = None, scene: Optional[Scene] = None,
                 field: Optional[DistanceField] = None, self_collision: Optional[SelfCollision] = None,
                 limits: Optional[Limits] = None, **kw):
        """``scene``: a ``Scene`` makes this an obstacle-avoiding engine (``set_obstacles``,
        ``get_clearances``, ``Plan.clearance``); None: the engine as before.  ``field``: a
        ``DistanceField`` adds a voxel distance field as one more obstacle (``set_distance_field``,
        ``clear_distance_field``); without ``scene`` it uses ``Scene.default(cfg)``.
        ``self_collision``: a ``SelfCollision`` adds the self-collision pairs of the scene's spheres
        (``get_self_clearances``, ``Plan.self_clearance``; arm and whole-body), likewise with the default scene.
        ``limits``: a ``Limits`` makes this a bounded engine (quadrotor and aerial; ``set_limits``,
        ``get_limits``): thrust and body torques are clamped in the rollouts, the plan and the returned u0."""
        self._L = capi.lib()
        self.cfg = cfg if cfg is not None else make_config(**kw)
        if (field is not None or self_collision is not None) and scene is None:
            scene = Scene.default(self.cfg)
        if limits is not None and scene is not None:
            raise ValueError("limits are for the quadrotor and aerial models, which have no scene engines")
        self.scene = scene
        self.field = field
        self.self_collision = self_collision
        self.has_limits = limits is not None
        h = C.c_void_p()
        if limits is not None:
            lc = limits.to_c()
            capi.check(self._L.mppi_create_limits(C.byref(self.cfg), C.byref(lc), C.byref(h)), "mppi_create_limits")
        elif self_collision is not None:
            sc, sf = scene.to_c(), self_collision.to_c()
            fd = None if field is None else field.to_c()
            capi.check(self._L.mppi_create_scene_self(C.byref(self.cfg), C.byref(sc), None if fd is None else C.byref(fd),
                                                      C.byref(sf), C.byref(h)), "mppi_create_scene_self")
        elif field is not None:
            sc, fd = scene.to_c(), field.to_c()
            capi.check(self._L.mppi_create_scene_field(C.byref(self.cfg), C.byref(sc), C.byref(fd), C.byref(h)),
                       "mppi_create_scene_field")
        elif scene is None:
            capi.check(self._L.mppi_create(C.byref(self.cfg), C.byref(h)), "mppi_create")
        else:
            sc = scene.to_c()
            capi.check(self._L.mppi_create_scene(C.byref(self.cfg), C.byref(sc), C.byref(h)), "mppi_create_scene")
        self._h = h
        c = self.cfg
        self.V, self.K, self.H, self.A = c.n_vehicles, c.n_samples, c.n_horizon, c.n_action
        self.state_dim = self._L.mppi_state_dim(C.byref(c))
        self.out_dim = self._L.mppi_output_dim(C.byref(c))
        self.traj_channels = self._L.mppi_traj_channels(C.byref(c))
        self._out = np.zeros((self.V, self.out_dim), np.float64)
        self._u0 = np.zeros((self.V, self.A), np.float32)
        self._stats = (capi.Stats * self.V)()
        # persistent host buffers with their ctypes pointers made once: ndarray.ctypes.data_as
        # costs ~3-4 us per call, several of them per control call (the latency path)
        self._state_buf = np.zeros((self.V, self.state_dim), np.float64)
        self._tgt_pos = np.zeros(3, np.float32)
        self._tgt_quat = np.zeros(4, np.float32)
        self._p_out, self._p_u0 = capi.dptr(self._out), capi.fptr(self._u0)
        self._p_state = capi.dptr(self._state_buf)
        self._state_flat = self._state_buf.reshape(-1)   # a view: the per-call fast path below
        self._p_tpos, self._p_tquat = capi.fptr(self._tgt_pos), capi.fptr(self._tgt_quat)
        if field is not None and field.d is not None:
            self.set_distance_field(field.d)

    # ------------------------------------------------------------------ admin
    def close(self):
        if getattr(self, "_h", None):
            self._L.mppi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------- native collective
    @staticmethod
    def comm_unique_id() -> bytes:
        """A fresh RCCL unique id (rank 0 makes it; the caller broadcasts it)."""
        buf = (C.c_uint8 * capi.COMM_ID_BYTES)()
        capi.check(capi.lib().mppi_comm_unique_id(buf), "comm_unique_id")
        return bytes(buf)

    @staticmethod
    def comm_available() -> Optional[str]:
        """None if RCCL is loadable with every entry point the engine binds, else why not."""
        L = capi.lib()
        if L.mppi_comm_available() == capi.OK:
            return None
        return L.mppi_last_error().decode(errors="replace")

    def comm_init(self, uid: bytes, timeout_ms: int = 0):
        """Join the shard communicator (collective over cfg.shard_count ranks).  Non-blocking
        init polled until ``timeout_ms`` (0: MPPI_COMM_INIT_TIMEOUT_MS, default 60 s); raises
        MPPIError(ERR_COMM) when the peers do not join in time."""
        if len(uid) != capi.COMM_ID_BYTES:
            raise ValueError("comm id must be %d bytes" % capi.COMM_ID_BYTES)
        buf = (C.c_uint8 * capi.COMM_ID_BYTES).from_buffer_copy(uid)
        capi.check(self._L.mppi_comm_init_ex(self._h, buf, int(timeout_ms)), "comm_init")

    def comm_info(self):
        """(nranks, rank) as the RCCL communicator itself reports them."""
        n, r = C.c_int32(), C.c_int32()
        capi.check(self._L.mppi_comm_info(self._h, C.byref(n), C.byref(r)), "comm_info")
        return n.value, r.value

    def exchange(self):
        capi.check(self._L.mppi_exchange(self._h), "exchange")

    def peer_open(self) -> bytes:
        """Open this rank's peer-exchange region; returns its IPC handle (mppi_peer_open)."""
        buf = (C.c_uint8 * capi.PEER_HANDLE_BYTES)()
        capi.check(self._L.mppi_peer_open(self._h, buf), "peer_open")
        return bytes(buf)

    def peer_connect(self, handles):
        """Map every rank's region (handles in rank order, this rank's own included)."""
        blob = b"".join(bytes(h) for h in handles)
        if any(len(h) != capi.PEER_HANDLE_BYTES for h in handles):
            raise ValueError("peer handles must be %d bytes each" % capi.PEER_HANDLE_BYTES)
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        capi.check(self._L.mppi_peer_connect(self._h, buf), "peer_connect")

    def peer_region(self) -> int:
        """This engine's exchange region as a device address (after peer_open; mppi_peer_region)."""
        x = C.c_uint64(0)
        capi.check(self._L.mppi_peer_region(self._h, C.byref(x)), "peer_region")
        return int(x.value)

    def peer_connect_ptrs(self, addresses):
        """In-process ranks: every rank's region address in rank order (mppi_peer_connect_ptrs)."""
        buf = (C.c_uint64 * len(addresses))(*[int(a) for a in addresses])
        capi.check(self._L.mppi_peer_connect_ptrs(self._h, buf), "peer_connect_ptrs")

    def peer_probe(self, phase: int):
        """Connection check (collective): phase 0 on every rank, a barrier, then phase 1."""
        capi.check(self._L.mppi_peer_probe(self._h, int(phase)), "peer_probe")

    def peer_status(self, reports: bool = True):
        """(sticky, reports, epoch) of the peer exchange (mppi_peer_status): ``sticky`` = this
        engine's timeout word (the given-up step's tag, 0 = none; host memory), ``reports`` = the
        timeout reports in this rank's region (one per rank, 0 = none; a device read, None when
        ``reports`` is False), ``epoch`` = the exchange epoch of the tags."""
        st, ep = C.c_uint32(0), C.c_uint32(0)
        rep = (C.c_uint64 * capi.MAX_PEERS)() if reports else None
        capi.check(self._L.mppi_peer_status(self._h, C.byref(st), rep, C.byref(ep)), "peer_status")
        return st.value, (list(rep) if reports else None), ep.value

    def peer_info(self):
        """(connected, rank, torn) of the peer exchange (mppi_peer_info): ``connected`` = the ranks whose
        word reached this rank's region in the connection probe's kernel phase, ``rank`` = this
        engine's shard rank, ``torn`` = the step tag of a step this rank's warm start came out of torn
        (some slices updated, others kept; 0 = none)."""
        n, r, t = C.c_int32(0), C.c_int32(0), C.c_uint32(0)
        capi.check(self._L.mppi_peer_info(self._h, C.byref(n), C.byref(r), C.byref(t)), "peer_info")
        return n.value, r.value, t.value

    def peer_reset(self, step: int, epoch: int):
        """Clear this rank's region and sticky word, take the agreed step counter and epoch
        (collective recovery: every rank synchronised, a barrier before and after)."""
        capi.check(self._L.mppi_peer_reset(self._h, step & 0xFFFFFFFF, epoch & 0xFFFFFFFF), "peer_reset")

    def get_step_counter(self) -> int:
        x = C.c_uint32(0)
        capi.check(self._L.mppi_get_step_counter(self._h, C.byref(x)), "get_step_counter")
        return x.value

    def set_stream(self, stream_handle: int):
        capi.check(self._L.mppi_set_stream(self._h, C.c_void_p(stream_handle)), "set_stream")

    def set_target(self, pos, quat=None, vehicle: int = 0):
        self._tgt_pos[:] = np.reshape(pos, 3)
        if quat is not None:
            self._tgt_quat[:] = np.reshape(quat, 4)
        capi.check(self._L.mppi_set_target(self._h, vehicle, self._p_tpos,
                                           None if quat is None else self._p_tquat), "set_target")

    def set_target_trajectory(self, pos, quat=None, vehicle: int = 0):
        """Target trajectory of a ``target_track`` engine: ``pos`` (H, 3), row t the position wanted
        at horizon index t, (t + 1) dt from now; ``quat`` (H, 4) xyzw rows (None: the fixed target's
        orientation on every row).  ``pos=None`` clears the table: the fixed target again."""
        p = None if pos is None else np.ascontiguousarray(pos, np.float32).reshape(self.H, 3)
        q = None if quat is None or pos is None else np.ascontiguousarray(quat, np.float32).reshape(self.H, 4)
        capi.check(self._L.mppi_set_target_trajectory(self._h, vehicle, capi.fptr(p), capi.fptr(q)),
                   "set_target_trajectory")

    def set_joint_trajectory(self, traj=None, vehicle: int = 0):
        """Joint tracking target (H, nq) of the joint_track cost term (None = zeros)."""
        t = None if traj is None else np.ascontiguousarray(traj, np.float32).reshape(self.H, -1)
        capi.check(self._L.mppi_set_joint_trajectory(self._h, vehicle, capi.fptr(t)), "set_joint_trajectory")

    def set_u_prev(self, u):
        u = np.ascontiguousarray(u, np.float32).reshape(self.V, self.H, self.A)
        capi.check(self._L.mppi_set_u_prev(self._h, capi.fptr(u)), "set_u_prev")

    def get_u_prev(self) -> np.ndarray:
        u = np.empty((self.V, self.H, self.A), np.float32)
        capi.check(self._L.mppi_get_u_prev(self._h, capi.fptr(u)), "get_u_prev")
        return u

    def set_state(self, state):
        self._state_buf[...] = np.reshape(state, (self.V, self.state_dim))
        capi.check(self._L.mppi_set_state(self._h, self._p_state), "set_state")

    def set_step_counter(self, step: int):
        capi.check(self._L.mppi_set_step_counter(self._h, step & 0xFFFFFFFF), "set_step_counter")

    # ------------------------------------------------------------------- step
    def step(self, state=None, noise=None):
        """One control step: returns (out (V,out_dim) float64, u0 (V,A), [StepStats])."""
        ps = None
        if state is not None:
            # (the control call's host overhead: a flat ndarray of the right size is copied
            #  with one slice assignment, ~1.6 us less than the reshape + broadcast)
            if type(state) is np.ndarray and state.shape == self._state_flat.shape:
                self._state_flat[:] = state
            else:
                self._state_buf[...] = np.reshape(state, (self.V, self.state_dim))
            ps = self._p_state
        n = None if noise is None else np.ascontiguousarray(noise, np.float32).reshape(
            self.V, self.K, self.H, self.A)
        capi.check(self._L.mppi_step(self._h, ps, capi.fptr(n), self._p_out, self._p_u0, self._stats),
                   "mppi_step")
        return self._out.copy(), self._u0.copy(), self.stats()

    def rollout(self, d_noise_ptr: int = 0):
        capi.check(self._L.mppi_rollout(self._h, C.c_void_p(d_noise_ptr or None)), "rollout")

    def finalize(self):
        capi.check(self._L.mppi_finalize(self._h), "finalize")

    def read_outputs(self):
        capi.check(self._L.mppi_read_outputs(self._h, self._p_out, self._p_u0, self._stats), "read_outputs")
        return self._out.copy(), self._u0.copy(), self.stats()

    def run_steps(self, n: int):
        """n asynchronous back-to-back control steps (no host sync)."""
        capi.check(self._L.mppi_run_steps(self._h, n), "run_steps")

    def synchronize(self):
        capi.check(self._L.mppi_synchronize(self._h), "synchronize")

    def set_prewarm(self, window_us: int):
        """Warm the native queue before each predicted control call (mppi_set_prewarm): for a node
        that ticks with idle gaps (100 Hz).  ``window_us`` 50 .. 5000; 0 turns it off."""
        capi.check(self._L.mppi_set_prewarm(self._h, int(window_us)), "set_prewarm")

    def prewarm(self):
        """(window_us, queue touches so far) of the prewarm."""
        us, n = C.c_int32(), C.c_int64()
        capi.check(self._L.mppi_get_prewarm(self._h, C.byref(us), C.byref(n)), "get_prewarm")
        return us.value, n.value

    def dispatch_info(self) -> str:
        """How the last run_steps / step were dispatched: "<aql | hip: why>; calls: <aql | hip>"."""
        buf = C.create_string_buffer(256)
        capi.check(self._L.mppi_dispatch_info(self._h, buf, len(buf)), "dispatch_info")
        return buf.value.decode(errors="replace")

    def kernel_info(self) -> str:
        """Which kernels the last run_steps / step ran: "batch: rollout <symbol>, finalize <symbol>,
        quiet finalize <symbol | none>, quiet rollout <symbol | none>; call: rollout <symbol>,
        finalize <symbol>"."""
        buf = C.create_string_buffer(1024)
        capi.check(self._L.mppi_kernel_info(self._h, buf, len(buf)), "kernel_info")
        return buf.value.decode(errors="replace")

    def stats(self) -> List[StepStats]:
        st = self._stats
        return [StepStats(s.rho, s.eta, s.ess, bool(s.nonfinite), bool(s.reach), s.nonfinite == 2)
                for s in ((st[0],) if self.V == 1 else st)]

    # -------------------------------------------------------------- exchange
    def exchange_slot_floats(self) -> int:
        n = C.c_int64()
        capi.check(self._L.mppi_exchange_slot_floats(self._h, C.byref(n)), "exchange_slot_floats")
        return n.value

    def bind_exchange(self, d_ptr: int):
        capi.check(self._L.mppi_bind_exchange(self._h, C.c_void_p(d_ptr)), "bind_exchange")

    # -------------------------------------------------------------- readback
    def get_costs(self) -> np.ndarray:
        S = np.empty((self.V, self.K), np.float32)
        capi.check(self._L.mppi_get_costs(self._h, capi.fptr(S)), "get_costs")
        return S

    def set_obstacles(self, centers=None, radii=None, velocities=None, vehicle: int = 0):
        """The sphere obstacles of one vehicle of a scene engine: ``centers`` (n, 3) world positions
        now, ``radii`` (n,), ``velocities`` (n, 3) m/s or None for static ones; at horizon index t an
        obstacle stands at centre + velocity (t + 1) dt.  n = 0 (or ``centers=None``) clears them."""
        c = np.zeros((0, 3), np.float32) if centers is None else np.ascontiguousarray(centers, np.float32).reshape(-1, 3)
        n = c.shape[0]
        r = np.zeros(0, np.float32) if radii is None else np.ascontiguousarray(radii, np.float32).reshape(-1)
        if r.shape[0] != n:
            raise ValueError(f"{n} centres and {r.shape[0]} radii")
        w = None if velocities is None else np.ascontiguousarray(velocities, np.float32).reshape(n, 3)
        capi.check(self._L.mppi_set_obstacles(self._h, vehicle, n, capi.fptr(c), capi.fptr(r), capi.fptr(w)),
                   "set_obstacles")

    def set_limits(self, limits: Limits):
        """Replaces a bounded engine's rotor limits (mppi_set_limits).  Takes effect on the next step."""
        if not self.has_limits:
            raise RuntimeError("engine created without limits (Engine(cfg, limits=Limits(...)))")
        lc = limits.to_c()
        capi.check(self._L.mppi_set_limits(self._h, C.byref(lc)), "set_limits")

    def get_limits(self) -> Optional[Limits]:
        """The bounds as last set, or None on an engine created without limits."""
        has, lc = C.c_int32(0), capi.Limits()
        capi.check(self._L.mppi_get_limits(self._h, C.byref(has), C.byref(lc)), "get_limits")
        return Limits.from_c(lc) if has.value else None

    def set_distance_field(self, d, origin=None):
        """Replaces a field engine's distance field: ``d`` (nz, ny, nx) metres, negative inside;
        ``origin`` (3,) moves node (0, 0, 0) (None: where it is).  Takes effect on the next step."""
        if self.field is None:
            raise RuntimeError("engine created without a field (Engine(cfg, field=DistanceField(...)))")
        d = self.field.check(d)
        o = None if origin is None else np.ascontiguousarray(origin, np.float32).reshape(3)
        capi.check(self._L.mppi_set_distance_field(self._h, capi.fptr(o), capi.fptr(d)), "set_distance_field")

    def clear_distance_field(self):
        """The field contributes nothing until the next ``set_distance_field``."""
        if self.field is None:
            raise RuntimeError("engine created without a field (Engine(cfg, field=DistanceField(...)))")
        capi.check(self._L.mppi_set_distance_field(self._h, None, None), "clear_distance_field")

    def set_occupancy(self, occ, origin=None, max_dist=None):
        """Replaces a field engine's distance field by the one of an occupancy grid: ``occ`` (nz, ny, nx)
        bool or uint8, nonzero = occupied; the transform runs on the device (mppi_set_occupancy), so only
        the bytes cross the bus.  ``max_dist`` (m) caps |d| (None: no cap); ``origin`` as in
        ``set_distance_field``.  Takes effect on the next step."""
        if self.field is None:
            raise RuntimeError("engine created without a field (Engine(cfg, field=DistanceField(...)))")
        occ = self.field.check_occupancy(occ)
        o = None if origin is None else np.ascontiguousarray(origin, np.float32).reshape(3)
        capi.check(self._L.mppi_set_occupancy(self._h, capi.fptr(o), occ.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              0.0 if max_dist is None else float(max_dist)), "set_occupancy")

    def integrate_depth(self, depth, view: DepthView, max_dist=None):
        """One depth image into a field engine's occupancy map, on the device (mppi_integrate_depth):
        ``depth`` (height, width) float32 metres along the optical axis, ``view`` its camera.  Free space
        along the rays is carved, the returns' end points are marked, and the field is rebuilt from the map
        under ``max_dist`` (None: no cap).  Takes effect on the next step."""
        if self.field is None:
            raise RuntimeError("engine created without a field (Engine(cfg, field=DistanceField(...)))")
        d, v = view.check_image(depth), view.to_c()
        capi.check(self._L.mppi_integrate_depth(self._h, C.byref(v), capi.fptr(d),
                                                0.0 if max_dist is None else float(max_dist)), "integrate_depth")

    def shift_map(self, shift, max_dist=None):
        """Moves the map's window by ``shift`` = (sx, sy, sz) nodes (mppi_shift_map): new node (ix, iy, iz) is
        old node (ix + sx, iy + sy, iz + sz), free where that falls outside; the origin moves by shift * voxel."""
        if self.field is None:
            raise RuntimeError("engine created without a field (Engine(cfg, field=DistanceField(...)))")
        s = (C.c_int32 * 3)(*check_shift(shift))
        capi.check(self._L.mppi_shift_map(self._h, s, 0.0 if max_dist is None else float(max_dist)), "shift_map")

    def get_occupancy(self) -> np.ndarray:
        """The occupancy map as it stands on the device, (nz, ny, nx) uint8 0 / 1 (all free before the first
        ``set_occupancy``, ``integrate_depth`` or ``shift_map``)."""
        if self.field is None:
            raise RuntimeError("engine created without a field (Engine(cfg, field=DistanceField(...)))")
        occ = np.empty(self.field.shape, np.uint8)
        capi.check(self._L.mppi_get_occupancy(self._h, occ.ctypes.data_as(C.POINTER(C.c_uint8))), "get_occupancy")
        return occ

    def get_distance_field(self):
        """``(d, origin)``: the field as it stands on the device, (nz, ny, nx) float32 and (3,) -- what the
        controller sees after ``set_distance_field`` or ``set_occupancy``; None while the field is cleared."""
        if self.field is None:
            raise RuntimeError("engine created without a field (Engine(cfg, field=DistanceField(...)))")
        is_set = C.c_int32(0)
        capi.check(self._L.mppi_get_distance_field(self._h, C.byref(is_set), None, None), "get_distance_field")
        if not is_set.value:
            return None
        d, o = np.empty(self.field.shape, np.float32), np.empty(3, np.float32)
        capi.check(self._L.mppi_get_distance_field(self._h, None, capi.fptr(o), capi.fptr(d)), "get_distance_field")
        return d, o

    def get_clearances(self) -> np.ndarray:
        """(V, K): every sample's min clearance to the obstacles over the horizon and the body
        spheres (+inf without obstacles); valid as ``get_costs`` is."""
        c = np.empty((self.V, self.K), np.float32)
        capi.check(self._L.mppi_get_clearances(self._h, capi.fptr(c)), "get_clearances")
        return c

    def get_self_clearances(self) -> np.ndarray:
        """(V, K): every sample's min clearance over the self-collision pairs and the horizon (+inf with
        an empty pair list); valid as ``get_costs`` is.  Self engines only."""
        if self.self_collision is None:
            raise RuntimeError("engine created without self-collision pairs (Engine(cfg, self_collision=SelfCollision(...)))")
        c = np.empty((self.V, self.K), np.float32)
        capi.check(self._L.mppi_get_self_clearances(self._h, capi.fptr(c)), "get_self_clearances")
        return c

    def get_weights(self) -> np.ndarray:
        w = np.empty((self.V, self.K), np.float32)
        capi.check(self._L.mppi_get_weights(self._h, capi.fptr(w)), "get_weights")
        return w

    def get_noise(self) -> np.ndarray:
        e = np.empty((self.V, self.K, self.H, self.A), np.float32)
        capi.check(self._L.mppi_get_noise(self._h, capi.fptr(e)), "get_noise")
        return e

    def get_trajectory(self) -> np.ndarray:
        t = np.empty((self.V, self.K, self.H, self.traj_channels), np.float32)
        capi.check(self._L.mppi_get_trajectory(self._h, capi.fptr(t)), "get_trajectory")
        return t

    def get_weighted_noise(self):
        raw = np.empty((self.V, self.H, self.A), np.float32)
        sm = np.empty_like(raw)
        capi.check(self._L.mppi_get_weighted_noise(self._h, capi.fptr(raw), capi.fptr(sm)), "get_weighted_noise")
        return raw, sm

    def get_plan(self) -> Plan:
        """The nominal plan of every vehicle (mppi_get_plan): one small kernel and four copies,
        outside the control step."""
        traj = np.empty((self.V, self.H, self.traj_channels), np.float32)
        cost_t = np.empty((self.V, self.H), np.float32)
        pos_err = np.empty_like(cost_t)
        S = np.empty(self.V, np.float32)
        capi.check(self._L.mppi_get_plan(self._h, capi.fptr(traj), capi.fptr(cost_t), capi.fptr(pos_err),
                                         capi.fptr(S)), "get_plan")
        clr = None
        if self.scene is not None:   # (k_plan wrote them with the plan above; a second, small launch and copy)
            clr = np.empty((self.V, self.H), np.float32)
            capi.check(self._L.mppi_get_plan_clearance(self._h, capi.fptr(clr)), "get_plan_clearance")
        sclr = None
        if self.self_collision is not None:
            sclr = np.empty((self.V, self.H), np.float32)
            capi.check(self._L.mppi_get_plan_self_clearance(self._h, capi.fptr(sclr)), "get_plan_self_clearance")
        return Plan(traj, cost_t, pos_err, S, self._ee_path(traj), clr, sclr)

    def _ee_path(self, traj: np.ndarray) -> np.ndarray:
        """(..., H, 3) positions out of (..., H, C) rows: the EE matrix's translation column (arm,
        whole-body) or the vehicle's position."""
        if self.cfg.model == capi.MODEL_AERIAL:   # xyz, rpy, q ahead of the EE
            return traj[..., -16:].reshape(*traj.shape[:-1], 4, 4)[..., :3, 3].copy()
        if self.cfg.model in (capi.MODEL_ARM, capi.MODEL_WHOLEBODY):
            return traj[..., self.A:].reshape(*traj.shape[:-1], 4, 4)[..., :3, 3].copy()
        return traj[..., :3].copy()

    def get_elites(self, n: int = 16, traj: bool = True) -> Elites:
        """The n lowest-cost samples of the last rollout of every vehicle with their costs, weights
        and (``traj``; needs store_trajectory) rollouts (mppi_get_elites): selected, sorted and
        gathered on the device, one copy, outside the control step."""
        n = int(n)
        idx = np.empty((self.V, max(n, 0)), np.int32)
        S = np.empty(idx.shape, np.float32)
        w = np.empty(idx.shape, np.float32)
        rows = np.empty((self.V, max(n, 0), self.H, self.traj_channels), np.float32) if traj else None
        capi.check(self._L.mppi_get_elites(self._h, n, idx.ctypes.data_as(C.POINTER(C.c_int32)), capi.fptr(S),
                                           capi.fptr(w), capi.fptr(rows)), "get_elites")
        return Elites(idx, S, w, rows, None if rows is None else self._ee_path(rows))

    # ---------------------------------------------------------------- timing
    def enable_timing(self, on: bool = True):
        capi.check(self._L.mppi_enable_timing(self._h, int(on)), "enable_timing")

    def timing(self):
        r, f = C.c_double(), C.c_double()
        rn, fn = C.c_int64(), C.c_int64()
        capi.check(self._L.mppi_get_timing(self._h, C.byref(r), C.byref(f), C.byref(rn), C.byref(fn)), "timing")
        return {"rollout_ms_total": r.value, "finalize_ms_total": f.value,
                "n_rollout": rn.value, "n_finalize": fn.value}

    def kernel_timing(self, n: int = 200):
        """(rollout_us, finalize_us): average device time per launch, launched back to back."""
        r, f = C.c_double(), C.c_double()
        capi.check(self._L.mppi_kernel_timing(self._h, n, C.byref(r), C.byref(f)), "kernel_timing")
        return r.value, f.value

    def kernel_timing_ex(self, n: int = 200):
        """(rollout_us, finalize_us, pair_us): back-to-back averages of each kernel, and of
        (rollout, finalize) pairs as a control step runs them.  Also on a shard."""
        r, f, pr = C.c_double(), C.c_double(), C.c_double()
        capi.check(self._L.mppi_kernel_timing_ex(self._h, n, C.byref(r), C.byref(f), C.byref(pr)),
                   "kernel_timing_ex")
        return r.value, f.value, pr.value

    def exchange_timing(self, n: int = 100) -> float:
        """Average all-reduce time (us) of the engine's RCCL communicator (collective)."""
        us = C.c_double()
        capi.check(self._L.mppi_exchange_timing(self._h, n, C.byref(us)), "exchange_timing")
        return us.value

    def rollout_bytes(self) -> int:
        return int(self._L.mppi_rollout_bytes(C.byref(self.cfg)))


def philox_normals(seed: int, step: int, vehicle: int, k0: int, K: int, H: int, A: int, device: int = 0):
    L = capi.lib()
    z = np.empty((K, H, A), np.float32)
    raw = np.empty((K, H, L.mppi_philox_words(A)), np.uint32)   # the words in consumption order
    capi.check(L.mppi_philox_normals(seed, step, vehicle, k0, K, H, A, device, capi.fptr(z),
                                     raw.ctypes.data_as(C.POINTER(C.c_uint32))), "philox_normals")
    return raw, z


def host_fk(chain, q, xyzquat, f64: bool = True) -> np.ndarray:
    """Single-configuration FK on the host (the check_reach path)."""
    L = capi.lib()
    cfg = capi.Config()
    fill_joints(cfg, chain)
    qq = np.ascontiguousarray(q, np.float64)
    b = np.ascontiguousarray(xyzquat, np.float64)
    T = np.empty(16, np.float32)
    capi.check(L.mppi_host_fk(cfg.joints, cfg.n_joints, capi.dptr(qq), capi.dptr(b), int(f64),
                              capi.fptr(T)), "host_fk")
    return T.reshape(4, 4)
