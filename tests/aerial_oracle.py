"""Float64 oracle of the aerial manipulator's rollout (MPPI_MODEL_AERIAL, csrc/mppi_rollout_aerial.hip) with
derived bounds, an fp32 restatement of the composition that takes planted mistakes, and the designs of
tests/test_aerial_oracle_cpu.py and tests/test_gpu_aerial.py.  Test infrastructure only; numpy / torch, no GPU.

The model: action (thrust, tau_xyz, qdd_0..6), v = u_prev + eps.  Built from the project's own oracles, each
used as it stands:
    base    tests/quad_oracle.py ``rollout`` on action dims 0..3, with its per-element running bound, validity
            mask and circular rule (EXCLUDED_CAP = 0.02, CIRCULAR_CAP = 0.01);
    joints  ``oracle.mppi_oracle.integrate`` (standard_normal_noise.py:32-50) on dims 4..10, in float64 on
            the fp32 values the device holds;
    EE      EE(k,t) = [Rz(yaw) Ry(pitch) Rx(roll) | p](k,t) M_fixed chain(q(k,t)) through ``O.chain_fk`` with
            ``mobile_dof=6``, i.e. ``O.xyzrpy_matrix`` with the per-(k,t) rpy (as obstacle_oracle.wholebody_frames
            evaluates the base), under ``O.float64_everywhere()``;
    S       ``O.pose_cost`` (pose_cost.py:24-63; weights 50, 30, 40, 30) in float64.

Bounds (nothing here is fitted to what the kernels give):
    q       TOL_Q, the project's constant for joint angles (tests/tracking_oracle.py).
    EE      the position of the end effector is p + R(rpy) r with r the end effector in the base frame,
            |r| <= rho = sum_j |xyz_j| over the chain's joint origins (every link adds at most its origin's
            length; about a metre for the Kinova).  R = Rz Ry Rx: a perturbation of one angle by d moves R r by
            at most d |r| (the derivative of an elementary rotation has norm 1), and each elementary rotation
            is formed from a sin / cos pair good to SINCOS_ABS (quad_oracle), so
                b_EE(k,t) = b_p + rho (b_roll + b_pitch + b_yaw + 3 SINCOS_ABS) + TOL_EE_WB
            per axis (b_p that axis' bound; b_* quad_oracle's), TOL_EE_WB the project's constant for the arm
            chain's own fp32 error in a mobile-base EE.
    R_EE    the rotation block likewise (every entry is bounded by the block's 2-norm error):
                b_R = (b_roll + b_pitch + b_yaw + 3 SINCOS_ABS) + ARM_ROT,
            where ARM_ROT = 7 (TOL_Q + 2 SINCOS_ABS + 8 U) + 8 U counts, per revolute joint, the joint angle's tolerance, its
            sin and cos and the eight roundings of its 3x3 update (kin_joint), and 8 U for the product with the
            fp32 target rotation.
    S       |dS| <= TOL_S |S| + sum_t w_pos(t) |b_EE(k,t)|_2 + sum_t w_ori(t) b_ori(k,t).  The orientation cost
            is the norm of eulerZYX(M), M = R_EE^T R*: yaw = atan2(m10, m00), pitch = asin(-m20), roll =
            atan2(m21, m22).  With c = sqrt(1 - m20^2) = cos(error pitch), an entry error d moves pitch by at
            most d / c and each atan2 by at most sqrt(2) d / c (both its arguments move; its gradient is 1 / c),
            so the norm moves by at most sqrt(5) d / c, first order, the way quad_oracle pushes through 1 / c_p;
            the device's atan2 (3.5 ulp at up to pi) and asinf add EULER_ABS = 1e-6 per angle:
                b_ori = sqrt(5) b_R / c + sqrt(3) EULER_ABS.
            A sample whose error rotation has |m20| + b_R > M20_MAX = 0.99 at any step is excluded (1 / c no
            longer first order), as is one quad_oracle's validity rule drops; both share EXCLUDED_CAP.

``emulate``: the composition restated in fp32 numpy (base: quad_oracle.emulate; joints: the integrator rounded to
fp32; chain and pose cost in fp32), taking planted mistakes (``variant=``):
    "fixed_attitude"  the WHOLEBODY composition: the rotation held at the measured rpy
    "row_shift"       the EE of row t under the base pose of row t - 1 (row 0: the measured pose)
    "rpy_order"       Rx Ry Rz
    "arm_offset"      the joints read from action dim 3 on
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

import quad_oracle as Q
import tracking_oracle as TO
from oracle import mppi_oracle as O

F32 = np.float32
U = Q.U
SINCOS_ABS = Q.SINCOS_ABS
EXCLUDED_CAP, CIRCULAR_CAP = Q.EXCLUDED_CAP, Q.CIRCULAR_CAP
TOL_Q, TOL_EE_WB, TOL_S, TOL_PERR_WB = TO.TOL_Q, TO.TOL_EE_WB, TO.TOL_S, TO.TOL_PERR_WB
ARM_ROT = 7 * (TOL_Q + 2 * SINCOS_ABS + 8 * U) + 8 * U
EULER_ABS = 1e-6
M20_MAX = 0.99
NQ, NA = 7, 11
WEIGHTS = (50.0, 30.0, 40.0, 30.0)
VARIANTS = ("fixed_attitude", "row_shift", "rpy_order", "arm_offset")
SIGMA = (30.0, 1.0, 1.0, 1.0) + (0.1,) * NQ


def chain_reach(chain) -> float:
    """rho = sum_j |xyz_j| over the chain (fp32 values as the engine holds them)."""
    return float(sum(np.linalg.norm(np.asarray(j.xyz, F32).astype(np.float64)) for j in chain))


# ---------------------------------------------------------------------------------------- float64 oracle
@dataclass
class Aerial:
    base: Q.Rollout           # the quadrotor oracle's rollout of dims 0..3
    q: np.ndarray             # (K, H, 7)
    ee: np.ndarray            # (K, H, 4, 4)
    S: np.ndarray             # (K,)
    cost_t: np.ndarray        # (K, H): each step's share of S
    pos_err: np.ndarray       # (K, H): L1 distance of the EE position to the target
    b_ee: np.ndarray          # (K, H, 3)
    b_rot: np.ndarray         # (K, H): b_R, on every entry of the EE's rotation block
    b_S: np.ndarray           # (K,)
    b_cost_t: np.ndarray      # (K, H)
    valid: np.ndarray         # (K, H): quad_oracle's rule and the error rotation's, cumulative in t
    m20: np.ndarray           # (K, H)


def split_state(state):
    """(x (6), v (6), q (7), qd (7)) of a packed AERIAL state row: xyz rpy q | v omega qd."""
    s = np.asarray(state, np.float64).reshape(12 + 2 * NQ)
    return s[:6], s[6 + NQ:12 + NQ], s[6:6 + NQ], s[12 + NQ:]


def rollout(chain, u, eps, state, tpos, tquat, cfg: Q.Cfg = Q.Cfg(), literal: bool = False, weights=WEIGHTS) -> Aerial:
    """u (H, 11) and eps (K, H, 11) as the device holds them (fp32); state the packed row (rounded to fp32 as
    build_vehicle_consts does); tpos (3,), tquat (4,) xyzw."""
    u = np.asarray(u, F32)
    eps = np.asarray(eps, F32)
    K, H, _ = eps.shape
    x, v, q0, qd0 = (np.asarray(a, np.float64).astype(F32).astype(np.float64) for a in split_state(state))
    ro = Q.rollout(u[:, :4], eps[..., :4], x, v, cfg, literal)
    dt = float(F32(cfg.dt))
    with O.float64_everywhere():
        acc = torch.as_tensor(u[None, :, 4:].astype(np.float64) + eps[..., 4:].astype(np.float64))
        qs = O.integrate(acc, torch.as_tensor(q0), torch.as_tensor(qd0), dt)
        full = torch.cat([torch.as_tensor(ro.pos), torch.as_tensor(ro.ang), qs], -1)
        ee = O.chain_fk(chain, full, mobile_dof=6)
        tp = torch.as_tensor(np.asarray(tpos, F32).astype(np.float64))
        tq = torch.as_tensor(np.asarray(tquat, F32).astype(np.float64))
        cp, co = O._pose_terms(ee, tp, tq)
        M = torch.matmul(torch.linalg.inv(ee[..., :3, :3]), O.quat_xyzw_matrix(tq)).numpy()
        perr = torch.sum(torch.abs(ee[..., :3, 3] - tp), -1).numpy()
        cp, co, ee, qs = cp.numpy(), co.numpy(), ee.numpy(), qs.numpy()
    wp = np.full(H, float(F32(weights[0])))
    wo = np.full(H, float(F32(weights[1])))
    wp[-1], wo[-1] = float(F32(weights[2])), float(F32(weights[3]))
    cost_t = wp * cp + wo * co
    S = cost_t.sum(-1)
    rho = chain_reach(chain)
    b_att = ro.bound_e.sum(-1) + 3 * SINCOS_ABS                       # (K, H)
    b_ee = ro.bound_p + (rho * b_att)[..., None] + TOL_EE_WB
    b_R = b_att + ARM_ROT
    m20 = M[..., 2, 0]
    ok = np.abs(m20) + b_R <= M20_MAX
    valid = ro.valid & np.logical_and.accumulate(ok, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.sqrt(np.maximum(1.0 - m20 * m20, 0.0))
        b_ori = np.where(ok, math.sqrt(5.0) * b_R / c, np.inf) + math.sqrt(3.0) * EULER_ABS
    b_t = wp * np.linalg.norm(b_ee, axis=-1) + wo * b_ori
    b_S = TOL_S * np.abs(S) + np.where(valid[:, -1], np.where(np.isfinite(b_t), b_t, 0.0).sum(-1), np.inf)
    b_cost_t = TOL_S * np.abs(S)[:, None] + b_t
    return Aerial(ro, qs, ee, S, cost_t, perr, b_ee, b_R, b_S, b_cost_t, valid, m20)


# ------------------------------------------------------------------------------------ fp32 restatement
def _rot_np(e, order: str, dtype):
    """(…, 3, 3) from rpy (…, 3): 'zyx' = Rz(yaw) Ry(pitch) Rx(roll); 'xyz' = Rx Ry Rz (the planted order)."""
    e = np.asarray(e, np.float64)
    s, c = np.sin(e).astype(dtype), np.cos(e).astype(dtype)
    sr, sp, sy, cr, cp, cy = s[..., 0], s[..., 1], s[..., 2], c[..., 0], c[..., 1], c[..., 2]
    z, o = np.zeros_like(sr), np.ones_like(sr)
    Rx = np.stack([np.stack([o, z, z], -1), np.stack([z, cr, -sr], -1), np.stack([z, sr, cr], -1)], -2)
    Ry = np.stack([np.stack([cp, z, sp], -1), np.stack([z, o, z], -1), np.stack([-sp, z, cp], -1)], -2)
    Rz = np.stack([np.stack([cy, -sy, z], -1), np.stack([sy, cy, z], -1), np.stack([z, z, o], -1)], -2)
    mm = lambda a, b: np.matmul(a, b).astype(dtype)  # noqa: E731
    return mm(mm(Rz, Ry), Rx) if order == "zyx" else mm(mm(Rx, Ry), Rz)


def _chain_np(chain, q, dtype):
    """(K, H, 4, 4): the chain product in ``dtype`` (origins from the joints' fp32 xyz / rpy; Rodrigues about the
    unit axis), joint by joint as urdfparser.py:122-163."""
    K, H, _ = q.shape
    T = np.broadcast_to(np.eye(4, dtype=dtype), (K, H, 4, 4)).copy()
    for j in chain:
        Oj = np.eye(4, dtype=dtype)
        Oj[:3, :3] = _rot_np(np.asarray(j.rpy, F32), "zyx", dtype)
        Oj[:3, 3] = np.asarray(j.xyz, F32).astype(dtype)
        L = np.broadcast_to(Oj, (K, H, 4, 4))
        if j.type in ("revolute", "continuous") and j.q_index >= 0:
            a = np.asarray(j.axis if j.axis is not None else (1.0, 0.0, 0.0), np.float64)
            a = (a / np.linalg.norm(a)).astype(dtype)
            qq = q[..., j.q_index].astype(np.float64)
            c, s = np.cos(qq).astype(dtype), np.sin(qq).astype(dtype)
            omc = (1 - c).astype(dtype)
            R = np.zeros((K, H, 4, 4), dtype)
            R[..., 3, 3] = 1
            ax = [[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]
            for r in range(3):
                for cc in range(3):
                    R[..., r, cc] = (c if r == cc else 0) + a[r] * a[cc] * omc + ax[r][cc] * s
            L = np.matmul(L, R).astype(dtype)
        T = np.matmul(T, L).astype(dtype)
    return T


def _pose_cost_np(ee, tpos, tquat, weights, dtype):
    """(S (K,), cost_t (K, H)) of pose_cost.py:24-63 in ``dtype`` (inv(R) of the orthonormal rotation as R^T)."""
    K, H = ee.shape[:2]
    with O.float64_everywhere():
        Rt = O.quat_xyzw_matrix(torch.as_tensor(np.asarray(tquat, F32).astype(np.float64))).numpy().astype(dtype)
    d = (ee[..., :3, 3] - np.asarray(tpos, F32).astype(dtype)).astype(dtype)
    cp = np.sqrt((d * d).sum(-1)).astype(dtype)
    M = np.matmul(np.swapaxes(ee[..., :3, :3], -1, -2), Rt).astype(dtype)
    yaw = np.arctan2(M[..., 1, 0], M[..., 0, 0])
    pitch = np.arcsin(np.clip(-M[..., 2, 0], -1, 1))
    roll = np.arctan2(M[..., 2, 1], M[..., 2, 2])
    co = np.sqrt((yaw * yaw + pitch * pitch + roll * roll).astype(dtype)).astype(dtype)
    wp = np.full(H, dtype(weights[0]))
    wo = np.full(H, dtype(weights[1]))
    wp[-1], wo[-1] = dtype(weights[2]), dtype(weights[3])
    ct = (wp * cp + wo * co).astype(dtype)
    return ct.sum(-1).astype(dtype), ct


def emulate(chain, u, eps, state, tpos, tquat, cfg: Q.Cfg = Q.Cfg(), literal: bool = False, weights=WEIGHTS,
            variant: Optional[str] = None) -> Dict[str, np.ndarray]:
    """The composition in float32: dict(base (K, H, 6), q (K, H, 7), ee (K, H, 4, 4), S (K), cost_t (K, H))."""
    assert variant is None or variant in VARIANTS, variant
    u = np.asarray(u, F32)
    eps = np.asarray(eps, F32)
    K, H, _ = eps.shape
    x, v, q0, qd0 = split_state(state)
    base = Q.emulate(u[:, :4], eps[..., :4], x, v, cfg, literal)["traj"]          # (K, H, 6) fp32
    off = 3 if variant == "arm_offset" else 4
    acc = (u[None, :, off:off + NQ] + eps[..., off:off + NQ]).astype(F32)           # v = u + eps, one rounding
    dt = F32(cfg.dt)
    q0, qd0 = q0.astype(F32), qd0.astype(F32)
    vel = (np.cumsum((acc * dt).astype(np.float64), 1).astype(F32) + qd0).astype(F32)
    vb = np.concatenate([np.broadcast_to(qd0, (K, 1, NQ)), vel[:, :-1]], 1)
    inc = (vb * dt + (F32(0.5) * acc) * (dt * dt)).astype(F32)
    q = (np.cumsum(inc.astype(np.float64), 1).astype(F32) + q0).astype(F32)
    arm = _chain_np(chain, q, F32)
    pose = base
    if variant == "row_shift":
        first = np.broadcast_to(np.asarray(x, np.float64).astype(F32), (K, 1, 6))
        pose = np.concatenate([first, base[:, :-1]], 1)
    rpy = pose[..., 3:]
    if variant == "fixed_attitude":
        rpy = np.broadcast_to(np.asarray(x[3:], np.float64).astype(F32), (K, H, 3))
    B = np.zeros((K, H, 4, 4), F32)
    B[..., 3, 3] = 1
    B[..., :3, :3] = _rot_np(rpy, "xyz" if variant == "rpy_order" else "zyx", F32)
    B[..., :3, 3] = pose[..., :3]
    ee = np.matmul(B, arm).astype(F32)
    S, ct = _pose_cost_np(ee, tpos, tquat, weights, F32)
    return dict(base=base, q=q, ee=ee, S=S, cost_t=ct)


# -------------------------------------------------------------------------------------------- comparison
@dataclass
class Ratios:
    """Worst err / bound per quantity over the compared elements, and the shares the rules set aside."""
    pos: float
    ang: float
    q: float
    ee: float
    rot: float
    S: float
    excluded: float
    circular: float

    def worst(self) -> float:
        return max(self.pos, self.ang, self.q, self.ee, self.rot, self.S)


def _ratio(err, bound, mask):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(np.asarray(err, np.float64)), r, np.inf)
    return np.where(mask, r, 0.0)


def compare(ao: Aerial, base, q, ee, S=None, samples=None) -> Ratios:
    """base (K, H, 6), q (K, H, 7), ee (K, H, 4, 4) or (K, H, 16) and optionally S (K,) against the oracle;
    ``samples``: the oracle's rows these arrays stand for (default: all)."""
    idx = np.arange(ao.S.shape[0]) if samples is None else np.asarray(samples)
    ro = ao.base
    sub = Q.Rollout(ro.pos[idx], ro.ang[idx], ro.vel[idx], ro.rate[idx], ro.bound_p[idx], ro.bound_e[idx], ro.bound_v[idx],
                    ro.bound_w[idx], ro.valid[idx], ro.circ[idx], {k: t[idx] for k, t in ro.terms.items()})
    rb = Q.compare(sub, base)
    valid = ao.valid[idx]
    K, H = valid.shape
    rq = _ratio(np.abs(np.asarray(q, np.float64) - ao.q[idx]), TOL_Q, np.ones((K, H, 1), bool))
    E = np.asarray(ee, np.float64).reshape(K, H, 4, 4)
    re = _ratio(np.abs(E[..., :3, 3] - ao.ee[idx][..., :3, 3]), ao.b_ee[idx], valid[..., None])
    rr = _ratio(np.abs(E[..., :3, :3] - ao.ee[idx][..., :3, :3]), ao.b_rot[idx][..., None, None], valid[..., None, None])
    rS = 0.0
    if S is not None:
        rS = float(_ratio(np.abs(np.asarray(S, np.float64) - ao.S[idx]), ao.b_S[idx], valid[:, -1]).max())
    return Ratios(rb.pos, rb.ang, float(rq.max()), float(re.max()), float(rr.max()), rS, float(1.0 - valid[:, -1].mean()),
                  rb.circular)


# ------------------------------------------------------------------------------------------------ designs
HOME = (1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0)


@dataclass(frozen=True)
class Design:
    """One state (roll, pitch of about 0.5 rad, body rates of about 2 rad/s: the attitude a rollout has leaves the
    measured one at once), target and seed."""
    name: str
    x: Sequence[float]
    v: Sequence[float]
    q: Sequence[float] = HOME
    qd: Sequence[float] = (0.1, -0.2, 0.15, 0.05, -0.1, 0.2, -0.05)
    tpos: Sequence[float] = (0.6, 0.2, 2.9)
    tquat: Sequence[float] = (0.0, 0.0, 0.0, 1.0)
    cfg: Q.Cfg = Q.Cfg()
    sigma: Tuple[float, ...] = SIGMA
    seed: int = 0

    @property
    def state(self):
        return np.asarray(tuple(self.x) + tuple(self.q) + tuple(self.v) + tuple(self.qd), np.float64)

    def inputs(self, K: int, H: int, seed: Optional[int] = None):
        """(u (H, 11), eps (K, H, 11)) fp32: the warm start around hover thrust and the injected noise."""
        rng = np.random.default_rng(4000 + (self.seed if seed is None else seed))
        sig = np.asarray(self.sigma, np.float64)
        u = np.zeros((H, NA), F32)
        u[:, 0] = Q._f(self.cfg.mass) * Q._f(self.cfg.gravity)
        u[:, 0] += (rng.normal(0.0, 1.0, H) * sig[0] / 60.0).astype(F32)
        u[:, 1:] += (rng.normal(0.0, 1.0, (H, NA - 1)) * sig[1:] / 2.0).astype(F32)
        eps = (rng.normal(0.0, 1.0, (K, H, NA)) * sig).astype(F32)
        return u, eps


DESIGNS = (
    Design("tilt_a", (0.2, -0.1, 2.5, 0.5, -0.45, 0.7), (0.3, -0.2, 0.1, 2.0, 1.2, -1.5)),
    Design("tilt_b", (-0.3, 0.4, 3.0, -0.5, 0.5, -1.2), (-0.2, 0.1, 0.3, -1.8, -1.0, 2.0), tpos=(0.1, 0.9, 3.3),
           tquat=(0.2, -0.1, 0.3, 0.9), seed=1),
)
BY_NAME = {d.name: d for d in DESIGNS}


@dataclass(frozen=True)
class Case:
    """One engine call of tests/test_gpu_aerial.py: vehicle v flies designs[v % len(designs)]."""
    tag: str
    K: int
    H: int
    V: int = 1
    designs: Tuple[str, ...] = ("tilt_a",)
    literal: bool = False

    def vehicles(self):
        out = []
        for v in range(self.V):
            d = BY_NAME[self.designs[v % len(self.designs)]]
            u, eps = d.inputs(self.K, self.H, seed=d.seed + 17 * v)
            out.append((d, u, eps))
        return out


CASES = (
    Case("K16-H32", 16, 32),                                    # one full block
    Case("K17-H20", 17, 20, designs=("tilt_b",)),               # a ragged block; H neither a power of two nor a multiple of 4
    Case("K48-H64-V2", 48, 64, V=2, designs=("tilt_a", "tilt_b")),   # the vc[v] path at the horizon cap
    Case("K16-H33", 16, 33, designs=("tilt_b",), literal=True),  # 31 pad lanes
)
