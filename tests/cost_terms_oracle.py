"""Float64 oracle of the five CostManager terms the reference ships switched off (covar, center, joint_track,
action, joint_limit: the XC rollout kernels of csrc/mppi_rollout.h and k_plan of csrc/mppi_plan.hip), one term
at a time, with a bound counted from the kernels' operations, an fp32 restatement that takes planted mistakes,
and the cases of tests/test_cost_terms_oracle_cpu.py and tests/test_gpu_cost_terms.py.  Test infrastructure
only; numpy (and torch through pose_envelope's exact integration), no GPU.

The terms (v_t = u_t + eps_t, q_t the joint positions after step t, g = fl32(gamma)):
    covar   w_cov sum_t u_t^T Sigma^-1 v_t          w_cov = fl32(w_covar lambda (1 - alpha)), not discounted
    center  sum_t g^t w_center ||q_t - q_c||^2
    track   sum_t g^t w_joint_track ||q_t - q*_t||^2   q*_t row t of the vehicle's joint-trajectory table
    action  sum_t g^t w_action ||v_t||^2
    limit   sum_t g^t penalty [some joint of q_t outside (q_lower, q_upper)]   (strict comparisons)
WHOLEBODY: covar and action over all 10 dims, the joint terms over dims 3..9.  S adds them in that order
(covar, center, track, action, limit) onto the pose cost; k_plan's cost_t adds the step's shares in the same order.

``oracle`` evaluates them in float64 on what the device receives -- the fp32 u_prev, eps, weights, q_center,
limits and table; q_t from pose_envelope.exact_arm / exact_wb; g^t and Sigma^-1 formed here (np.linalg.inv of the
fp32 Sigma) -- and carries a bound on |kernel - float64| per term, per sample and per step.  U = 2^-24 per fp32
rounding, first order, times SECOND = 1.05 for the dropped products of two errors.  The counts, each from the code:
    v = u + eps: one rounding, dv = U |v|.
    q: pose_envelope.q_rounding_bound (the integrator's arithmetic on the device's v) plus the exact integration
       of dv (the double integrator is linear: the rounded v moves q by at most the integral of |dv|).  A joint
       whose v is zero at every step of a sample is exact: its increments are sums of zeros and q0 is an fp32
       value, so dq = 0 there (the designs park a joint on its limit this way: ">" against ">=").
    g^t: std::pow on floats, one ulp (2 U); Sigma^-1 entries: the cast of the host's fp64 inverse, one ulp (2 U).
    covar, per step: y_a = sum_b s_ab v_b is NA fmaf (diagonal Sigma: one product), qd = sum_a u_a y_a NA more:
       |d qd| <= M (2 + 1 + 2 NA) U with M = sum_a |u_a| sum_b |s_ab| |v_b| (diagonal: 2 + 1 + 1 + NA).
    action, per step: s2 = sum_a v_a^2, NA fmaf on operands of relative error U: (2 + NA) U s2; the two products
       by w and g^t and the table's ulp: 4 U.
    center, track, per step: d = q - c is one rounding on top of dq: dd = dq + U |d|; the fmaf chain over NQ
       joints: sum_j (2 |d_j| dd_j + dd_j^2) + NQ U sc; the products and the table: 4 U.
    limit, per step: the product penalty g^t and the table's ulp: 3 U; the flag itself is exact or excluded.
    the sum over t: each lane adds its chunks (NCH - 1 roundings), the segment scan adds ceil(log2 LSEG) more on
       the path of every element: (ceil(log2 LSEG) + NCH - 1) U sum_t |x_t| (covar: of M_t); covar's product by
       w_cov: U |covar|.
    S: one rounding per S_seg += add after the first non-zero partial sum, U |partial|; a pose cost in front
       comes with its own bound (the GPU test: pose_envelope.TOL_S of the fp32 oracle's pose cost).
    k_plan: cost_t adds the step's shares the same way; its S is a 64-lane fold and the waves' sums:
       (6 + waves - 1) U sum_t |cost_t|.
The limit term is an indicator: a sample is excluded where some (t, j) lies within dq of a limit (``kept``), a
step of the plan likewise (``kept_t``).

``emulate`` restates the kernels' chain in fp32 (Kogge-Stone scans, fmaf where the source calls it) and takes one
planted mistake (``MISTAKES``); ``compare`` returns err / bound per term group, ``exposed`` the ratio in the group a
mistake must show in.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np

import pose_envelope as PE

U = 2.0 ** -24
SUBNORMAL = 2.0 ** -149
SECOND = 1.05
F32 = np.float32
DT = PE.DT
TERMS = ("covar", "center", "track", "action", "limit")          # the kernel's order of the sum
BITS = {"covar": "covar", "center": "center", "track": "joint_track", "action": "action", "limit": "joint_limit"}
EXCLUDED_CAP = 0.05
# the Kinova limits and centring target of mppi_config_default (joint_space_cost.py:16,71-72), as fp32
KINOVA_QC = np.array([0.0, 0.0, 0.0, (-3.0718 - 0.0698) / 2, 0.0, (3.7525 - 0.0175) / 2, 0.0], F32)
KINOVA_LO = np.array([-6.2832, 0.8203, -6.2832, 0.5236, -6.2832, 1.1345, -6.2832], F32)
KINOVA_HI = np.array([6.2832, 5.4629, 6.2832, 5.7596, 6.2832, 5.1487, 6.2832], F32)
BASE7 = np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
WB_QUAT = np.array([0.0, 0.0, 0.0, 1.0], F32)


def _f(x) -> float:
    return float(F32(x))


def _d(x):
    return np.asarray(x, np.float64)


# ------------------------------------------------------------------------------------------ configuration
@dataclass(frozen=True)
class Params:
    """The cost_weights of a case (none at its default) and lambda."""
    gamma: float = 0.95
    alpha: float = 0.25
    w_covar: float = 0.3
    w_center: float = 0.8
    w_joint_track: float = 0.7
    w_action: float = 0.02
    penalty: float = 10.0
    lam: float = 0.1

    def cost_weights(self) -> Dict[str, float]:
        return dict(cost_gamma=self.gamma, cost_alpha=self.alpha, w_covar=self.w_covar, w_center=self.w_center,
                    w_joint_track=self.w_joint_track, w_action=self.w_action, joint_limit_penalty=self.penalty)

    @property
    def w_cov(self) -> float:
        """fl32(w_covar lambda (1 - alpha)) on the config's fp32 weights and fp64 lambda (device_params)."""
        return _f(_f(self.w_covar) * (float(self.lam) * (1.0 - _f(self.alpha))))

    def weight(self, term: str) -> float:
        return {"covar": self.w_cov, "center": _f(self.w_center), "track": _f(self.w_joint_track), "action": _f(self.w_action),
                "limit": _f(self.penalty)}[term]


@dataclass(frozen=True)
class Lay:
    """The rollout's lane layout: L lanes per segment, R = 64 / L segments per wave, nch 64-lane chunks per lane,
    nw waves per block, nb blocks per vehicle, iters groups per block (mppi_debug_layout)."""
    L: int
    nch: int
    nw: int = 1
    nb: int = 1
    iters: int = 1

    @property
    def R(self):
        return 64 // self.L

    @property
    def levels(self):
        return int(math.ceil(math.log2(self.L))) + self.nch - 1


def layout_of(**config) -> Lay:
    """The layout engine creation derives for a configuration (no device)."""
    from quadrotor_manipulator_mppi_amd import _capi as capi
    from quadrotor_manipulator_mppi_amd.engine import make_config
    L = capi.lib()
    L.mppi_debug_layout.restype = C.c_int32
    L.mppi_debug_layout.argtypes = [C.POINTER(capi.Config), C.POINTER(C.c_int32), C.c_int32]
    out = (C.c_int32 * 28)()
    cfg = make_config(**config)
    assert L.mppi_debug_layout(C.byref(cfg), out, 28) == capi.OK, L.mppi_last_error().decode()
    assert out[2] == 64 // out[1]
    return Lay(L=out[1], nch=out[3], nw=out[0] // 64, nb=out[4], iters=out[5])


@dataclass
class Inputs:
    """What one vehicle's rollout receives.  ``tables`` (V, H, 7): every vehicle's joint-trajectory table as the
    device holds them (zeros where none is set); this vehicle's is tables[vehicle]."""
    model: str
    u: np.ndarray            # (H, NA) fp32
    eps: np.ndarray          # (K, H, NA) fp32
    q0: np.ndarray           # (7,) fp32-exact
    sigma: np.ndarray        # (NA, NA) fp32
    par: Params
    tables: np.ndarray
    lay: Lay
    terms: Tuple[str, ...]
    f64: bool = True
    vehicle: int = 0
    x0: np.ndarray = field(default_factory=lambda: PE.WB_X0.copy())
    qc: np.ndarray = field(default_factory=lambda: KINOVA_QC.copy())
    qlo: np.ndarray = field(default_factory=lambda: KINOVA_LO.copy())
    qhi: np.ndarray = field(default_factory=lambda: KINOVA_HI.copy())

    @property
    def qoff(self):
        return 3 if self.model == "wholebody" else 0

    @property
    def diag(self):
        s = np.asarray(self.sigma)
        return not np.any(s[~np.eye(len(s), dtype=bool)] != 0)

    @property
    def state(self):
        if self.model == "wholebody":
            return PE.wb_state(WB_QUAT, self.q0, self.x0)
        return PE.arm_state(BASE7, self.q0)


def positions(inp: Inputs, chain=None, zero_noise=False):
    """(K, H, NA) float64: the exact integration of u + eps from rest (pose_envelope.exact_arm / exact_wb)."""
    chain = PE.kinova_chain() if chain is None else chain
    eps = np.zeros_like(inp.eps[:1]) if zero_noise else inp.eps
    if inp.model == "wholebody":
        return PE.exact_wb(chain, WB_QUAT, eps, inp.u, inp.q0, inp.x0)[0]
    return PE.exact_arm(chain, BASE7, eps, inp.u, inp.q0)[0]


def _integrate(a):
    """The double integrator from rest on (K, H, A) float64 (standard_normal_noise.py:41-48)."""
    vel = np.cumsum(a * DT, axis=1)
    before = np.concatenate([np.zeros_like(vel[:, :1]), vel[:, :-1]], 1)
    return np.cumsum(before * DT + 0.5 * a * DT * DT, axis=1)


# ---------------------------------------------------------------------------------------- float64 oracle
@dataclass
class Terms:
    val: Dict[str, np.ndarray]       # term -> (K,)
    bnd: Dict[str, np.ndarray]
    val_t: Dict[str, np.ndarray]     # term -> (K, H): the step's share (k_plan's cost_t)
    bnd_t: Dict[str, np.ndarray]
    S: np.ndarray                    # (K,): pose + the enabled terms in the kernel's order
    bS: np.ndarray
    cost_t: np.ndarray               # (K, H)
    b_cost_t: np.ndarray
    kept: np.ndarray                 # (K,) bool: no (t, j) within dq of a limit (all True without the limit term)
    kept_t: np.ndarray               # (K, H)
    hit: np.ndarray                  # (K,) bool: the limit flag set at some step
    q: np.ndarray                    # (K, H, 7)
    dq: np.ndarray

    @property
    def excluded(self) -> int:
        return int((~self.kept).sum())


def _fin(b):
    return np.maximum(np.asarray(b, np.float64) * SECOND, SUBNORMAL)


def oracle(inp: Inputs, pos=None, pose=None, pose_t=None, zero_noise=False) -> Terms:
    """``pos``: positions(inp) if already formed.  ``pose`` = (S_pose (K,), bound (K,)) and ``pose_t`` = (K, H) pair:
    a pose cost in front of the sum.  ``zero_noise``: the plan's rollout (v = u, one sample)."""
    par, lay = inp.par, inp.lay
    u = _d(inp.u)
    eps = np.zeros((1,) + inp.eps.shape[1:]) if zero_noise else _d(inp.eps)
    K, H, NA = eps.shape
    QOFF, NQ = inp.qoff, 7
    v = u[None] + eps
    dv = np.zeros_like(v) if zero_noise else U * np.abs(v)      # (the plan reads u_prev itself: nothing rounds)
    pos = positions(inp, zero_noise=zero_noise) if pos is None else pos
    q = pos[..., QOFF:]
    q0 = _d(inp.q0)
    dq = PE.q_rounding_bound(q, q0) + _integrate(dv)[..., QOFF:]
    still = (np.abs(v[..., QOFF:]).max(axis=1, keepdims=True) == 0)
    dq = np.where(still, 0.0, dq)
    gt = _f(par.gamma) ** np.arange(H, dtype=np.float64)
    val_t, bnd_t, mag_t = {}, {}, {}
    if "covar" in inp.terms:
        sinv = np.linalg.inv(_d(inp.sigma))
        if inp.diag:
            sinv = np.diag(np.diag(sinv))
        y = np.einsum("ab,khb->kha", sinv, v)
        qd = (u[None] * y).sum(-1)
        M = (np.abs(u)[None] * np.einsum("ab,khb->kha", np.abs(sinv), np.abs(v))).sum(-1)
        n = (2 + 1 + 1 + NA) if inp.diag else (2 + 1 + 2 * NA)
        val_t["covar"], bnd_t["covar"], mag_t["covar"] = qd, M * U * n, M
    if "action" in inp.terms:
        x = par.weight("action") * gt * (v * v).sum(-1)
        val_t["action"], bnd_t["action"] = x, x * U * (2 + NA + 4)
    for name, w, ref in (("center", par.weight("center"), _d(inp.qc)[None, None]),
                         ("track", par.weight("track"), _d(inp.tables[inp.vehicle])[None])):
        if name not in inp.terms:
            continue
        d = q - ref
        dd = dq + U * np.abs(d)
        sc = (d * d).sum(-1)
        bsc = (2 * np.abs(d) * dd + dd * dd).sum(-1) + NQ * U * sc
        x = w * gt * sc
        val_t[name], bnd_t[name] = x, w * gt * bsc + 4 * U * x
    lo, hi = _d(inp.qlo)[None, None], _d(inp.qhi)[None, None]
    kept_t = np.ones((K, H), bool)
    hit = np.zeros(K, bool)
    if "limit" in inp.terms:
        out = ((q < lo) | (q > hi)).any(-1)
        with np.errstate(invalid="ignore"):
            near = (((np.abs(q - lo) <= dq) | (np.abs(q - hi) <= dq)) & (dq > 0)).any(-1)
        x = par.weight("limit") * gt * out
        val_t["limit"], bnd_t["limit"] = x, 3 * U * x
        kept_t, hit = ~near, out.any(-1)
    # per sample: the lanes' chunks, the segment scan, covar's weight
    val, bnd = {}, {}
    for name in val_t:
        mag = mag_t.get(name, np.abs(val_t[name]))
        T, b = val_t[name].sum(-1), bnd_t[name].sum(-1) + lay.levels * U * mag.sum(-1)
        if name == "covar":
            wc = par.weight("covar")
            T, b = wc * T, wc * b + U * np.abs(wc * T)
            bnd_t[name] = wc * bnd_t[name] + U * np.abs(wc * val_t[name])
            val_t[name] = wc * val_t[name]
        val[name], bnd[name] = T, b
    # the sums in the kernel's order
    S, bS = (np.zeros(K), np.zeros(K)) if pose is None else (_d(pose[0]).copy(), _d(pose[1]).copy())
    ct, bct = (np.zeros((K, H)), np.zeros((K, H))) if pose_t is None else (_d(pose_t[0]).copy(), _d(pose_t[1]).copy())
    for name in TERMS:
        if name not in val:
            continue
        first, first_t = (S == 0) & (bS == 0), (ct == 0) & (bct == 0)     # 0 + add is exact
        S, ct = S + val[name], ct + val_t[name]
        bS = bS + bnd[name] + np.where(first, 0.0, U * np.abs(S))
        bct = bct + bnd_t[name] + np.where(first_t, 0.0, U * np.abs(ct))
    return Terms({k: x for k, x in val.items()}, {k: _fin(b) for k, b in bnd.items()}, val_t, {k: _fin(b) for k, b in bnd_t.items()},
                 S, _fin(bS), ct, _fin(bct), kept_t.all(-1), kept_t, hit, q, dq)


def plan_S(cost_t, b_cost_t):
    """(S, bound) of k_plan's fold over one vehicle's steps (H,): a 64-lane fold per wave, then the waves' sums."""
    c = _d(cost_t)
    waves = (c.shape[-1] + 63) // 64
    return c.sum(-1), _fin(_d(b_cost_t).sum(-1) / SECOND + (6 + waves - 1) * U * np.abs(c).sum(-1))


# ------------------------------------------------------------------------------------ fp32 restatement
MISTAKES = (
    "cov_sigma", "cov_diag_shortcut", "cov_vv", "cov_uu", "cov_weight_plain", "cov_discounted",
    "act_eps", "act_u", "act_undiscounted", "act_gamma_ahead",
    "q_before_step", "wb_dims_0_6", "jt_row_ahead", "jt_vehicle0", "jt_ignored", "jt_pitch_na",
    "lim_ge", "lim_lower_only", "lim_per_joint",
    "pad_counted", "chunk2_dropped", "iter2_not_reset", "neighbour_segment")
# the term group a mistake must push outside its bound ("any": some enabled term)
SHOWS_IN = dict({m: "covar" for m in MISTAKES if m.startswith("cov_")}, **{m: "action" for m in MISTAKES if m.startswith("act_")},
                **{m: "track" for m in MISTAKES if m.startswith("jt_")}, **{m: "limit" for m in MISTAKES if m.startswith("lim_")},
                q_before_step="joint", wb_dims_0_6="joint", pad_counted="any", chunk2_dropped="any", iter2_not_reset="any",
                neighbour_segment="any")


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _scan(x, axis):
    """Inclusive Kogge-Stone scan in fp32 along ``axis`` (any length: the absent lanes are zeros)."""
    x = np.moveaxis(np.array(x, F32), axis, 0)
    d = 1
    while d < x.shape[0]:
        y = x.copy()
        y[d:] = x[d:] + x[:-d]
        x, d = y, 2 * d
    return np.moveaxis(x, 0, axis)


def _scan_chunks(x):
    """The integrator's scan over (K, H, A): 64-lane chunks, the carry added after each chunk's scan."""
    out = np.empty_like(x)
    carry = np.zeros_like(x[:, 0])
    for c in range(0, x.shape[1], 64):
        s = _scan(x[:, c:c + 64], 1)
        if c:
            s = s + carry[:, None]
        out[:, c:c + 64] = s
        carry = s[:, -1]
    return out


def _positions32(inp: Inputs, act):
    """(posf (K, H, NA) fp32, posd float64): rollout_body's NCH > 1 integrator from rest (fp contract off)."""
    dt, h2 = F32(DT), F32(0.5) * F32(DT * DT)
    vel = _scan_chunks(act * dt)
    prev = np.concatenate([np.zeros_like(vel[:, :1]), vel[:, :-1]], 1)
    c2 = _scan_chunks(prev * dt + act * h2)
    p0 = _d(inp.q0) if inp.model == "arm" else np.concatenate([_d(inp.x0), _d(inp.q0)])
    if inp.f64:
        posd = c2.astype(np.float64) + p0
        return posd.astype(F32), posd
    posf = c2 + p0.astype(F32)
    return posf, posf.astype(np.float64)


def _segment_sum(x, lay: Lay):
    """(K,) fp32: each lane adds its chunks, the segment scan, the last lane's value."""
    K, H = x.shape
    lanes = np.zeros((K, lay.L), F32)
    for c in range(lay.nch):
        part = x[:, c * 64:c * 64 + lay.L]
        lanes[:, :part.shape[1]] += part
    return _scan(lanes, 1)[:, -1]


def emulate(inp: Inputs, variant: Optional[str] = None, zero_noise=False):
    """dict(term -> (K,) fp32, term + "_t" -> (K, H), S, cost_t) of the kernels' chain in fp32 with one planted
    mistake; the pose cost is 0 (weights (0, 0, 0, 0))."""
    assert variant is None or variant in MISTAKES, variant
    par, lay = inp.par, inp.lay
    u = np.asarray(inp.u, F32)
    eps = np.zeros((1,) + inp.eps.shape[1:], F32) if zero_noise else np.asarray(inp.eps, F32)
    K, H, NA = eps.shape
    QOFF, NQ = inp.qoff, 7
    act = u[None] + eps
    ub = np.broadcast_to(u[None], act.shape)
    posf, posd = _positions32(inp, act)
    if variant == "q_before_step":
        p0 = (_d(inp.q0) if inp.model == "arm" else np.concatenate([_d(inp.x0), _d(inp.q0)]))[None, None]
        posd = np.concatenate([np.broadcast_to(p0, posd[:, :1].shape), posd[:, :-1]], 1)
        posf = posd.astype(F32)
    off = 0 if variant == "wb_dims_0_6" else QOFF
    qf, qd_ = posf[..., off:off + NQ], posd[..., off:off + NQ]
    g = F32(par.gamma)
    gts = np.power(g, np.arange(H, dtype=F32)).astype(F32)
    out = {}
    if "covar" in inp.terms:
        sinv = np.linalg.inv(_d(inp.sigma)).astype(F32)
        if variant == "cov_sigma":
            sinv = np.asarray(inp.sigma, F32)
        left = act if variant == "cov_vv" else ub
        right = ub if variant == "cov_uu" else act
        qd = np.zeros((K, H), F32)
        for a in range(NA):
            if inp.diag or variant == "cov_diag_shortcut":
                y = sinv[a, a] * right[..., a]
            else:
                y = np.zeros((K, H), F32)
                for b in range(NA):
                    y = _fma(sinv[a, b], right[..., b], y)
            qd = _fma(left[..., a], y, qd)
        if variant == "cov_discounted":
            qd = qd * gts
        out["covar_t"] = qd
    if "action" in inp.terms:
        src = eps if variant == "act_eps" else ub if variant == "act_u" else act
        s2 = np.zeros((K, H), F32)
        for a in range(NA):
            s2 = _fma(src[..., a], src[..., a], s2)
        ga = np.ones(H, F32) if variant == "act_undiscounted" else (gts * g) if variant == "act_gamma_ahead" else gts
        out["action_t"] = (F32(par.weight("action")) * s2) * ga
    rows = np.asarray(inp.tables[inp.vehicle], F32)
    if variant == "jt_row_ahead":
        rows = rows[np.minimum(np.arange(H) + 1, H - 1)]
    elif variant == "jt_vehicle0":
        rows = np.asarray(inp.tables[0], F32)
    elif variant == "jt_ignored":
        rows = np.zeros_like(rows)
    elif variant == "jt_pitch_na":
        flat = np.concatenate([np.asarray(inp.tables, F32).reshape(-1), np.zeros(H * NA * len(inp.tables), F32)])
        rows = np.stack([flat[(inp.vehicle * H + t) * NA:(inp.vehicle * H + t) * NA + NQ] for t in range(H)])
    for name, ref in (("center", np.asarray(inp.qc, F32)[None, None]), ("track", rows[None])):
        if name not in inp.terms:
            continue
        sc = np.zeros((K, H), F32)
        for j in range(NQ):
            d = qf[..., j] - ref[..., j]
            sc = _fma(d, d, sc)
        out[name + "_t"] = (F32(par.weight(name)) * sc) * gts
    if "limit" in inp.terms:
        lo, hi = _d(inp.qlo)[None, None], _d(inp.qhi)[None, None]
        qq = qd_ if inp.f64 else qf.astype(np.float64)
        above = (qq >= hi) if variant == "lim_ge" else (qq > hi)
        flags = (qq < lo) | (above & (variant != "lim_lower_only"))
        n = flags.sum(-1).astype(F32) if variant == "lim_per_joint" else flags.any(-1).astype(F32)
        out["limit_t"] = (F32(par.weight("limit")) * gts) * n
    res = {}
    S, cost_t = np.zeros(K, F32), np.zeros((K, H), F32)
    for name in TERMS:
        if name + "_t" not in out:
            continue
        x = np.array(out[name + "_t"], F32)
        xs = x.copy()
        if variant == "chunk2_dropped":
            xs[:, 64:] = 0
        T = _segment_sum(xs, lay)
        if variant == "pad_counted":
            T = T + F32(lay.L * lay.nch - H) * x[:, H - 1]
        if variant == "iter2_not_reset":     # group it of a lane starts from what group it - 1 left in the accumulator
            per = lay.nb * lay.nw * lay.R
            for k in range(per, K):
                T[k] = T[k] + T[k - per]
        if variant == "neighbour_segment":   # segment s of a wave credited with segment s - 1's sum
            k = np.arange(K)
            T = T[np.minimum((k // lay.R) * lay.R + (k % lay.R - 1) % lay.R, K - 1)]
        if name == "covar":
            wc = F32(_f(par.w_covar)) if variant == "cov_weight_plain" else F32(par.weight("covar"))
            T, x = wc * T, wc * x
        res[name], res[name + "_t"] = T, x
        S, cost_t = S + T, cost_t + x
    res["S"], res["cost_t"] = S, cost_t
    return res


# -------------------------------------------------------------------------------------------- comparison
def _ratio(err, bound, mask):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(np.asarray(err, np.float64)), r, np.inf)
    return np.where(mask, r, 0.0)


def compare(o: Terms, got: Dict[str, np.ndarray]) -> Dict[str, float]:
    """Worst err / bound per quantity in ``got``: a term's name (K,), name + "_t" (K, H), "S", "cost_t"; the samples
    (steps) the limit rule keeps."""
    r = {}
    for key, g in got.items():
        g = _d(g)
        if key in ("S", "cost_t"):
            want, b = (o.S, o.bS) if key == "S" else (o.cost_t, o.b_cost_t)
        elif key.endswith("_t"):
            want, b = o.val_t[key[:-2]], o.bnd_t[key[:-2]]
        else:
            want, b = o.val[key], o.bnd[key]
        r[key] = float(_ratio(np.abs(g - want), b, o.kept if g.ndim == 1 else o.kept_t).max())
    return r


def exposed(r: Dict[str, float], mistake: str) -> float:
    """err / bound of a planted mistake's run in the group named for it (per sample or per step, whichever is larger)."""
    grp = SHOWS_IN[mistake]
    names = {"any": TERMS, "joint": ("center", "track", "limit")}.get(grp, (grp,))
    return max([r.get(n, 0.0) for n in names] + [r.get(n + "_t", 0.0) for n in names])


# ------------------------------------------------------------------------------------------------ cases
ALL5 = TERMS
HOME = PE.HOME.astype(F32)


@dataclass(frozen=True)
class Case:
    """One engine of tests/test_gpu_cost_terms.py (and its inputs on the CPU).  ``table``: which vehicles have a
    joint-trajectory table set ("all", "v1": vehicle 1 only, "none").  ``pose``: the four pose weights."""
    tag: str
    model: str
    K: int
    H: int
    terms: Tuple[str, ...]
    f64: bool = True
    V: int = 1
    sigma: str = "full"
    bpv: int = 0
    threads: int = 0
    table: str = "all"
    pose: Tuple[float, float, float, float] = (0.0, 0.0, 0.0, 0.0)
    track: bool = False
    par: Params = Params()
    seed: int = 0

    @property
    def NA(self):
        return 10 if self.model == "wholebody" else 7

    def sigma32(self):
        rng = np.random.default_rng(77 + self.NA)
        if self.sigma == "diag":
            return np.diag(rng.uniform(0.05, 0.2, self.NA)).astype(F32)
        m = rng.normal(size=(self.NA, self.NA))
        return (0.05 * m @ m.T / self.NA + 0.08 * np.eye(self.NA)).astype(F32)

    def config(self) -> Dict:
        """make_config's arguments."""
        kw = dict(model=self.model, n_samples=self.K, n_horizon=self.H, n_vehicles=self.V, noise="injected", weights=self.pose,
                  sigma=self.sigma32(), lam=self.par.lam, blocks_per_vehicle=self.bpv, block_threads=self.threads,
                  cost_terms=tuple(BITS[t] for t in self.terms) + (("target_track",) if self.track else ()),
                  cost_weights=self.par.cost_weights())
        if self.model == "arm":
            kw["state_f64"] = self.f64
        return kw

    def tables(self):
        """(V, H, 7) fp32: each vehicle's table where one is set (a slow sweep around its start), zeros elsewhere."""
        rng = np.random.default_rng(500 + self.seed)
        tb = np.zeros((self.V, self.H, 7), F32)
        t = np.arange(1, self.H + 1)[:, None] / self.H
        for v in range(self.V):
            if self.table == "all" or (self.table == "v1" and v == 1):
                tb[v] = (self.q0(v)[None] + 0.3 * np.sin(t * rng.uniform(1.0, 4.0, 7) + v) + rng.uniform(-0.2, 0.2, 7)).astype(F32)
        return tb

    def _off(self):
        """The near limits' distance from the start: 0.2 of the spread unit noise gives a joint by the horizon's end
        (dt^2 sqrt(sum_s (H - s + 1/2)^2) ~ dt^2 sqrt(H^3 / 3)), so that either joint crosses on about two samples in five."""
        return 0.2 * DT * DT * math.sqrt(self.H ** 3 / 3.0)

    def q0(self, v=0):
        q = HOME.astype(np.float64)
        q[[0, 2, 4]] += 0.05 * v
        if "limit" in self.terms:   # joint 1 above its lower limit, joint 3 below its upper, joint 6 parked on its upper
            off = self._off()
            q[1], q[3], q[6] = float(KINOVA_LO[1]) + off, float(KINOVA_HI[3]) - off, float(KINOVA_HI[6])
        return q.astype(F32)

    def inputs(self, v=0, lay: Optional[Lay] = None) -> Inputs:
        rng = np.random.default_rng(1000 + 31 * self.seed + 7 * v + self.H)
        NA = self.NA
        u = (0.3 * rng.normal(size=(self.H, NA))).astype(F32)
        eps = rng.normal(size=(self.K, self.H, NA)).astype(F32)
        if "limit" in self.terms:   # the parked joint's control is zero on every sample
            u[:, -1], eps[..., -1] = 0, 0
            u[:, [NA - 6, NA - 4]] *= F32(0.2)   # (the two near joints: the noise, not the warm start, decides the crossing)
            if self.K == 1:   # the plan has no noise to cross with: a drift through the upper limit near H / 2, the lower near 0.7 H
                a = F32(9.3 * self._off() / (self.H * DT) ** 2)   # (9.3, not 8: the crossing falls between two steps)
                u[:, NA - 6] = -a / 2
                u[:, NA - 4] = a
        x0 = (PE.WB_X0 + 0.1 * v).astype(F32).astype(np.float64)
        lay = layout_of(**self.config()) if lay is None else lay
        return Inputs(self.model, u, eps, self.q0(v), self.sigma32(), self.par, self.tables(), lay, self.terms, self.f64 and self.model == "arm",
                      v, x0)


SHAPES = (("k64h32", dict(K=64, H=32)), ("k50h20f32", dict(K=50, H=20, f64=False)), ("k32h96", dict(K=32, H=96)),
          ("k64h64", dict(K=64, H=64)), ("looped", dict(K=64, H=32, bpv=8, threads=128)))
ARM_SINGLE = tuple(Case(f"arm-{s}-{t}", "arm", terms=(t,), seed=i, **kw) for i, (s, kw) in enumerate(SHAPES) for t in TERMS) + \
    (Case("arm-k64h32-covar-diag", "arm", 64, 32, ("covar",), sigma="diag", seed=9),)
ARM_ALL = (Case("arm-all5-pose", "arm", 64, 32, ALL5, pose=(0.5, 0.3, 0.4, 0.3), seed=11),
           Case("arm-all5-track", "arm", 64, 32, ALL5, track=True, seed=12))
WB = tuple(Case(f"wb-k32h64-{t}", "wholebody", 32, 64, (t,), seed=20 + i) for i, t in enumerate(TERMS)) + \
    (Case("wb-k32h64-all5", "wholebody", 32, 64, ALL5, seed=26),)
FLEET = (Case("fleet-v1-table", "arm", 48, 32, ("center", "track"), V=2, table="v1", seed=30),
         Case("fleet-both-tables", "arm", 48, 32, ("center", "track"), V=2, table="all", seed=31))
SELF = (Case("self-sc", "arm", 64, 32, ALL5, seed=40), Case("self-sf", "arm", 64, 32, ALL5, seed=41))
PLAN = (Case("plan-arm-f64", "arm", 1, 96, ALL5, seed=50), Case("plan-arm-f32", "arm", 1, 20, ALL5, f64=False, seed=51),
        Case("plan-wb", "wholebody", 1, 64, ALL5, seed=52))
ROLLOUT = ARM_SINGLE + ARM_ALL + WB + FLEET + SELF
BY_TAG = {c.tag: c for c in ROLLOUT + PLAN}


def declared(case: Case, lay: Lay, v: int = 0) -> Tuple[str, ...]:
    """The planted mistakes a case is declared to expose: by the terms it enables and the forms its shape reaches."""
    t = set(case.terms)
    joint = t & {"center", "track", "limit"}
    out = []
    if "covar" in t:
        out += ["cov_sigma", "cov_weight_plain", "cov_discounted"]
        out += ["cov_vv", "cov_uu"] if case.K > 1 else []     # (the plan's v is u)
        out += ["cov_diag_shortcut"] if case.sigma == "full" else []
    if "action" in t:
        out += ["act_eps", "act_undiscounted", "act_gamma_ahead"]
        out += ["act_u"] if case.K > 1 else []
    if joint:
        out += ["q_before_step"]
        out += ["wb_dims_0_6"] if case.model == "wholebody" else []
    if "track" in t:
        has = case.table == "all" or (case.table == "v1" and v == 1)
        out += ["jt_row_ahead", "jt_ignored"] if has else []
        out += ["jt_vehicle0"] if v == 1 else []
        out += ["jt_pitch_na"] if case.model == "wholebody" and has else []
    if "limit" in t:
        out += ["lim_ge", "lim_lower_only", "lim_per_joint"]
    if case.K > 1:
        out += ["pad_counted"] if case.H < lay.L * lay.nch else []
        out += ["chunk2_dropped"] if lay.nch > 1 else []
        out += ["iter2_not_reset"] if lay.iters > 1 else []
        out += ["neighbour_segment"] if lay.R > 1 else []
    return tuple(out)
