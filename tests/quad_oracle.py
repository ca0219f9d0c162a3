"""Float64 oracle of the 6-DoF quadrotor rollout with a running first-order error bound, an fp32
restatement of the kernel's chain that takes planted mistakes, and the designs of
tests/test_quad_oracle_cpu.py and tests/test_gpu_quad_envelope.py.  Test infrastructure only; numpy, no GPU.

The recurrence (csrc/mppi_rollout_quad.hip:9-25, one step in csrc/mppi_quad_step.h; x = (p, rpy), v = (v, omega),
thrust and torques u + eps):
    step 0:  omega_0 = omega + dt I^-1 tau_0,  v_0 = v + dt (g + (R(rpy) f_0 - kd v) / m),
             rpy_0 = rpy + dt J(rpy) omega (the measured rates, no wrap),  p_0 = p + dt v (the measured velocity)
    t >= 1:  omega_t = omega_{t-1} + dt I^-1 tau_t,  rpy_t = wrap(rpy_{t-1} + dt J(rpy_{t-1}) omega_t),
             v_t = v_{t-1} + dt (g + (R(rpy_{t-1}) f_t - kd v_{t-1}) / m),  p_t = p_{t-1} + dt v_t
    literal mode: the closed-form inv(J) in place of J for t >= 1;  wrap(x) = x - 2 pi rint(x / 2 pi).

``rollout`` evaluates it in float64 on the fp32 values the device holds (u, eps, the rounded state, fl32(dt),
fl32(1/m), fl32(1/I_j), fl32(kd), fl32(g)), so what separates it from the kernel is arithmetic alone, and carries
a bound on |fp32 chain - float64| per element: every operation of quad_axis_step pushes its operands' bounds
through the absolute partial derivatives and adds its own rounding.  The constants, each from the code:
    U = 2^-24 relative per add or multiply, one per operation as the source writes them (the compiler contracts
        some into FMAs; an FMA only removes a rounding).  Multiplying by the exact 1 or 0 of a lane constant
        (a0, the 1 of row 2's 1/c_p) and adding an exact 0 (g on axes 0 and 1, column 0 of J on rows 1, 2) round
        nothing and are not counted.
    v = u + eps: one rounding.
    v_rcp_f32 (the shared 1/c_p): 2 U / |c| (1 ulp) plus the propagated dc / (|c| (|c| - dc)).
    sin, cos: the angle's bound (|d sin| <= |d angle|) plus SINCOS_ABS = 2.6e-7, the project's recorded maximum
        of sincos_joint for an fp32 angle (csrc/mppi_fk.h:66-69, profiles/r01/sincos_accuracy.txt).  It is a
        record, not a derivation, and was taken over [-3 pi, 3 pi]; sincos_joint's reduction (rint and two FMAs
        against a two-term 1/2pi) hands the hardware the same interval [-1/2, 1/2] revolutions for any angle, so
        it is SUPPOSED to carry to the design that starts at 48 rad.
    the wrap: |n| |fl32(2 pi) - 2 pi| + 2 U |en| for n = rint(en / 2 pi) (the product and the subtraction).
The bound is kept per source (TERMS: roundings, SINCOS_ABS, the wrap's constant), so an excess can be traced to
one of them; it is multiplied by SECOND = 1.05 for the neglected second-order terms and floored at one fp32
subnormal (exact zeros compare as 0 <= floor).

Validity.  An element of sample k at step t is compared while, at every step s <= t, the bound on cos(pitch)
of the attitude that step used is at most 1% of |cos pitch|: beyond that the terms the first order drops
(relative perturbations above 1% through 1/c_p) are no longer a few percent of it.  ``Rollout.valid`` is that
mask; a case may lose at most EXCLUDED_CAP of its samples to it.

Angles are compared as stored, not modulo 2 pi -- a wrap at the wrong step is a bug the user sees -- except
where the float64 pre-wrap value lies within the element's bound of an odd multiple of pi: there either branch
of rint is right, and the comparison is circular (``Rollout.circ``; at most CIRCULAR_CAP of a case's angle
elements).

The cost (csrc/mppi_rollout_quad.hip: d = p - target, fmaf(d, d, stage) over t < H - 1, the last step's square
apart, the three axes summed, w_stage stage + w_term term).  With b = bound_p + U |d| (the subtraction's own
rounding),
    |dS| <= sum w (2 |d| b + b^2) + (H + 3) U S
the second term for the squares, the fmaf chain, the three-axis sum and the two weights.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

U = 2.0 ** -24
SUBNORMAL = 2.0 ** -149
SINCOS_ABS = 2.6e-7
SECOND = 1.05
PITCH_REL = 0.01
EXCLUDED_CAP = 0.02
CIRCULAR_CAP = 0.01
TERMS = ("round", "sincos", "wrap")
NT = len(TERMS)
F32 = np.float32
TWO_PI_32 = float(F32(6.283185307179586))
INV_2PI_32 = F32(0.15915494309189535)
D_2PI = abs(TWO_PI_32 - 2.0 * math.pi)


def _f(x) -> float:
    return float(F32(x))


# ------------------------------------------------------------------------------------------ configuration
@dataclass(frozen=True)
class Cfg:
    """The rigid body and the step as mppi_config holds them (quad_mass, quad_inertia, quad_kd, quad_gravity: fp32)."""
    dt: float = 0.01
    mass: float = 14.7
    inertia: Tuple[float, float, float] = (1.57, 3.93, 2.59)
    kd: float = 0.0
    gravity: float = 9.81

    def device(self):
        """(dt, 1/m, 1/I, kd, g) as DevParams holds them (mppi_layout.cpp: (float)(1.0 / (double)c.quad_mass))."""
        return (_f(self.dt), _f(1.0 / _f(self.mass)), tuple(_f(1.0 / _f(i)) for i in self.inertia), _f(self.kd),
                _f(self.gravity))

    def quad(self, literal: bool) -> Dict:
        """make_config's ``quad`` argument."""
        return dict(quad_mass=self.mass, quad_inertia=self.inertia, quad_kd=self.kd, quad_gravity=self.gravity,
                    quad_literal_jinv=bool(literal))


# ------------------------------------------------------------------------- values that carry their bound
class _B:
    """A float64 (or longdouble) value and the per-source bound on |fp32 chain - value| (..., NT)."""
    __slots__ = ("v", "b")

    def __init__(self, v, b=None):
        self.v = v
        self.b = np.zeros(np.shape(v) + (NT,)) if b is None else b

    @property
    def tot(self):
        return self.b.sum(-1)


def _a(v):
    return np.abs(np.asarray(v, np.float64))


def _own(v, b):
    """+ the operation's own rounding."""
    b = np.array(b, np.float64)
    b[..., 0] += U * _a(v)
    return _B(v, b)


def _add(x: _B, y: _B) -> _B:
    return _own(x.v + y.v, x.b + y.b)


def _sub(x: _B, y: _B) -> _B:
    return _own(x.v - y.v, x.b + y.b)


def _mul(x: _B, y: _B) -> _B:
    return _own(x.v * y.v, _a(x.v)[..., None] * y.b + _a(y.v)[..., None] * x.b)


def _cmul(c, x: _B) -> _B:
    """An exact fp32 constant times x."""
    return _own(c * x.v, abs(float(c)) * x.b)


def _cadd(c, x: _B) -> _B:
    return _own(c + x.v, x.b)


def _neg(x: _B) -> _B:
    return _B(-x.v, x.b)


def _div(x: _B, y: _B) -> _B:
    """IEEE division (the host's quad_outputs)."""
    return _own(x.v / y.v, x.b / _a(y.v)[..., None] + _a(x.v / (y.v * y.v))[..., None] * y.b)


def _sin(x: _B, own=None) -> _B:
    v = np.sin(x.v)
    b = np.array(x.b, np.float64)
    if own is None:
        b[..., 1] += SINCOS_ABS
    else:
        b[..., 0] += own * _a(v)
    return _B(v, b)


def _cos(x: _B, own=None) -> _B:
    v = np.cos(x.v)
    b = np.array(x.b, np.float64)
    if own is None:
        b[..., 1] += SINCOS_ABS
    else:
        b[..., 0] += own * _a(v)
    return _B(v, b)


def _rcp(c: _B) -> _B:
    """v_rcp_f32: 1 ulp of its own, and dc / (|c| (|c| - dc)) from the operand.  Where dc >= |c| the bound is
    +inf (the element is outside the validity rule long before)."""
    ac, dc = _a(c.v), c.tot
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.where(ac > dc, ac * (ac - dc), 0.0)
        b = np.where(den[..., None] > 0, c.b / den[..., None], np.inf)
        v = 1.0 / c.v
        b[..., 0] += 2.0 * U / ac
    return _B(v, b)


def _two_pi(dtype):
    return 8 * np.arctan(dtype(1))


def _wrap(x: _B):
    """(wrapped, circular): x - 2 pi rint(x / 2 pi); circular where x lies within the result's bound of an odd
    multiple of pi."""
    tp = _two_pi(x.v.dtype.type)
    n = np.rint(x.v / tp)
    v = x.v - tp * n
    b = np.array(x.b, np.float64)
    b[..., 0] += 2.0 * U * _a(x.v)
    b[..., 2] += np.abs(n).astype(np.float64) * D_2PI
    half = tp / 2
    m = 2 * np.rint((x.v / half - 1) / 2) + 1                       # the nearest odd multiple of pi
    circ = _a(x.v - m * half) <= b.sum(-1) * SECOND
    return _B(v, b), circ


# ---------------------------------------------------------------------------------------- float64 oracle
@dataclass
class Rollout:
    pos: np.ndarray        # (K, H, 3) each
    ang: np.ndarray
    vel: np.ndarray
    rate: np.ndarray
    bound_p: np.ndarray
    bound_e: np.ndarray
    bound_v: np.ndarray
    bound_w: np.ndarray
    valid: np.ndarray      # (K, H): the validity rule
    circ: np.ndarray       # (K, H, 3): angle elements compared modulo 2 pi
    terms: Dict[str, np.ndarray] = field(default_factory=dict)   # quantity -> (K, H, 3, NT), before SECOND


def _jrates(e, w, literal_now):
    """(Euler rates, cos pitch) of attitude e (three _B) under body rates w."""
    sr, sp, _ = (_sin(x) for x in e)
    cr, cp, _ = (_cos(x) for x in e)
    ox, oy, oz = w
    if literal_now:   # inv(J) = [[1, 0, -s_p], [0, c_r, s_r c_p], [0, -s_r, c_r c_p]]
        d0 = _sub(ox, _mul(sp, oz))
        d1 = _add(_mul(cr, oy), _mul(_mul(sr, cp), oz))
        d2 = _sub(_mul(_mul(cr, cp), oz), _mul(sr, oy))
    else:             # J = [[1, s_r t, c_r t], [0, c_r, -s_r], [0, s_r / c_p, c_r / c_p]], t = s_p / c_p
        ic = _rcp(cp)
        f0 = _mul(ic, sp)
        d0 = _add(_mul(_mul(cr, f0), oz), _add(_mul(_mul(sr, f0), oy), ox))
        d1 = _add(_mul(_neg(sr), oz), _mul(cr, oy))
        d2 = _add(_mul(_mul(cr, ic), oz), _mul(_mul(sr, ic), oy))
    return [d0, d1, d2], cp


def rollout(u, eps, x0, v0, cfg: Cfg = Cfg(), literal: bool = False, dtype=np.float64) -> Rollout:
    """u (H, 4) and eps (K, H, 4) as the device holds them (fp32); x0 = (p, rpy), v0 = (v, omega), rounded to
    fp32 as build_vehicle_consts does.  ``dtype``: np.longdouble for the CPU test's cross-check."""
    u = np.asarray(u, F32)
    eps = np.asarray(eps, F32)
    K, H, _ = eps.shape
    dt, im, iinv, kd, g = cfg.device()
    x = np.asarray(x0, np.float64).astype(F32).astype(dtype)
    vv = np.asarray(v0, np.float64).astype(F32).astype(dtype)
    full = lambda s: _B(np.full(K, s, dtype))  # noqa: E731
    p, e = [full(x[j]) for j in range(3)], [full(x[3 + j]) for j in range(3)]
    v, w = [full(vv[j]) for j in range(3)], [full(vv[3 + j]) for j in range(3)]
    w_meas = list(w)
    out = {q: np.zeros((K, H, 3), np.float64) for q in "pevw"}
    bnd = {q: np.zeros((K, H, 3, NT), np.float64) for q in "pevw"}
    valid, circ = np.zeros((K, H), bool), np.zeros((K, H, 3), bool)
    ok = np.ones(K, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(H):
            first = t == 0
            ctl = [_own(u[t, a].astype(dtype) + eps[:, t, a].astype(dtype), np.zeros((K, NT))) for a in range(4)]
            thr = ctl[0]
            w = [_add(w[j], _cmul(dt, _cmul(iinv[j], ctl[1 + j]))) for j in range(3)]
            d, cp = _jrates(e, w_meas if first else w, literal and not first)
            ok = ok & (cp.tot <= PITCH_REL * _a(cp.v))
            sr, sp, sy = (_sin(a) for a in e)      # (again: the attitude before the step)
            cr, _, cy = (_cos(a) for a in e)
            en = [_add(e[j], _cmul(dt, d[j])) for j in range(3)]
            if not first:
                for j in range(3):
                    en[j], circ[:, t, j] = _wrap(en[j])
            spcr = _mul(sp, cr)
            r = [_add(_mul(cy, spcr), _mul(sy, sr)), _sub(_mul(sy, spcr), _mul(cy, sr)), _mul(cp, cr)]
            for j in range(3):
                a = _cmul(im, _sub(_mul(r[j], thr), _cmul(kd, v[j])))
                if j == 2:
                    a = _cadd(-g, a)
                nv = _add(v[j], _cmul(dt, a))
                p[j] = _add(p[j], _cmul(dt, v[j] if first else nv))
                v[j] = nv
            e = en
            valid[:, t] = ok
            for q, s in (("p", p), ("e", e), ("v", v), ("w", w)):
                for j in range(3):
                    out[q][:, t, j] = s[j].v
                    bnd[q][:, t, j] = s[j].b
    tot = {q: np.maximum(np.where(np.isfinite(b.sum(-1)), b.sum(-1), np.inf) * SECOND, SUBNORMAL) for q, b in bnd.items()}
    return Rollout(out["p"], out["e"], out["v"], out["w"], tot["p"], tot["e"], tot["v"], tot["w"], valid, circ,
                   dict(pos=bnd["p"], ang=bnd["e"], vel=bnd["v"], rate=bnd["w"]))


def rollout_values(u, eps, x0, v0, cfg: Cfg = Cfg(), literal: bool = False, dtype=np.longdouble):
    """The recurrence alone in ``dtype``, written independently of ``rollout`` (arrays over the axes, J and R as
    matrices): (pos, ang, vel, rate), each (K, H, 3)."""
    u = np.asarray(u, F32).astype(dtype)
    eps = np.asarray(eps, F32).astype(dtype)
    K, H, _ = eps.shape
    dt, im, iinv, kd, g = (np.asarray(c, np.float64).astype(dtype) for c in cfg.device())
    x = np.asarray(x0, np.float64).astype(F32).astype(dtype)
    vv = np.asarray(v0, np.float64).astype(F32).astype(dtype)
    p, e = np.tile(x[:3], (K, 1)), np.tile(x[3:], (K, 1))
    v, w = np.tile(vv[:3], (K, 1)), np.tile(vv[3:], (K, 1))
    w_meas = w.copy()
    gv = np.array([0, 0, -g], dtype)
    tp = _two_pi(dtype)
    out = [np.zeros((K, H, 3), dtype) for _ in range(4)]
    for t in range(H):
        ctl = u[t] + eps[:, t]
        w = w + dt * (iinv * ctl[:, 1:])
        J = jacobian(e)
        if literal and t > 0:
            J = inv_jacobian(e)
        R = rotation(e)
        en = e + dt * np.einsum("kij,kj->ki", J, w_meas if t == 0 else w)
        if t > 0:
            en = en - tp * np.rint(en / tp)
        nv = v + dt * (gv + im * (R[:, :, 2] * ctl[:, :1] - kd * v))
        p = p + dt * (v if t == 0 else nv)
        v, e = nv, en
        for o, s in zip(out, (p, e, v, w)):
            o[:, t] = s
    return tuple(out)


def jacobian(e):
    """Body rates -> Euler rates (drone.py:114-124), (..., 3) rpy -> (..., 3, 3)."""
    sr, cr, sp, cp = np.sin(e[..., 0]), np.cos(e[..., 0]), np.sin(e[..., 1]), np.cos(e[..., 1])
    z, o = np.zeros_like(sr), np.ones_like(sr)
    t = sp / cp
    return np.stack([np.stack([o, sr * t, cr * t], -1), np.stack([z, cr, -sr], -1), np.stack([z, sr / cp, cr / cp], -1)], -2)


def inv_jacobian(e):
    """The closed form the literal mode applies (csrc/mppi_rollout_quad.hip:24)."""
    sr, cr, sp, cp = np.sin(e[..., 0]), np.cos(e[..., 0]), np.sin(e[..., 1]), np.cos(e[..., 1])
    z, o = np.zeros_like(sr), np.ones_like(sr)
    return np.stack([np.stack([o, z, -sp], -1), np.stack([z, cr, sr * cp], -1), np.stack([z, -sr, cr * cp], -1)], -2)


def rotation(e):
    """R = Rz(yaw) Ry(pitch) Rx(roll) (drone.py:126-154)."""
    sr, cr, sp, cp = np.sin(e[..., 0]), np.cos(e[..., 0]), np.sin(e[..., 1]), np.cos(e[..., 1])
    sy, cy = np.sin(e[..., 2]), np.cos(e[..., 2])
    return np.stack([np.stack([cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], -1),
                     np.stack([sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr], -1),
                     np.stack([-sp, cp * sr, cp * cr], -1)], -2)


# ------------------------------------------------------------------------------------------------ cost
def cost(pos, bound_p, targets, w_stage: float = 100.0, w_term: float = 20.0):
    """(S, bound, cost_t, bound_t, pos_err, bound_err) of positions (..., H, 3) against ``targets`` (3,) or (H, 3):
    S as the rollout forms it; cost_t and pos_err (the L1 distance) per step as the plan kernel does, cost_t
    under the same count at H = 1 (square, two adds, the weight) and pos_err under two adds."""
    pos = np.asarray(pos, np.float64)
    H = pos.shape[-2]
    tg = np.asarray(targets, F32).astype(np.float64)
    d = pos - tg
    b = np.asarray(bound_p, np.float64) + U * np.abs(d)
    wt = np.full(H, _f(w_stage))
    wt[-1] = _f(w_term)
    c_t = wt * (d * d).sum(-1)
    b_t = wt * (2 * np.abs(d) * b + b * b).sum(-1)
    S = c_t.sum(-1)
    e1 = np.abs(d).sum(-1)
    return (S, np.maximum(b_t.sum(-1) + (H + 3) * U * S, SUBNORMAL), c_t, np.maximum(b_t + 4 * U * c_t, SUBNORMAL),
            e1, np.maximum(b.sum(-1) + 2 * U * e1, SUBNORMAL))


# ------------------------------------------------------------------------------- the host's first step
def first_step_outputs(x, v, u0, cfg: Cfg = Cfg()):
    """(out, bound): the 12 outputs of the host's quad_outputs (csrc/mppi_engine.cpp) -- the model's step 0
    under u0 in fp32 -- in float64, the bound counted from that function's operations: one U per add, multiply
    or divide, std::sin / std::cos on float at 1 ulp (2 U relative)."""
    dt, im, iinv, kd, g = cfg.device()
    x = [_B(np.float64(F32(a))) for a in x]
    v = [_B(np.float64(F32(a))) for a in v]
    u0 = [_B(np.float64(F32(a))) for a in u0]
    sr, sp, sy = (_sin(a, 2 * U) for a in x[3:])
    cr, cp, cy = (_cos(a, 2 * U) for a in x[3:])
    tp = _div(sp, cp)
    r02 = _add(_mul(_mul(cy, sp), cr), _mul(sy, sr))
    r12 = _sub(_mul(_mul(sy, sp), cr), _mul(cy, sr))
    r22 = _mul(cp, cr)
    wx, wy, wz = v[3:]
    dr = _add(_add(wx, _mul(_mul(sr, tp), wy)), _mul(_mul(cr, tp), wz))
    dp = _sub(_mul(cr, wy), _mul(sr, wz))
    dy = _add(_mul(_div(sr, cp), wy), _mul(_div(cr, cp), wz))
    out = [_add(x[j], _cmul(dt, v[j])) for j in range(3)]
    out += [_add(x[3 + j], _cmul(dt, d)) for j, d in enumerate((dr, dp, dy))]
    for j, r in enumerate((r02, r12, r22)):
        a = _cmul(im, _sub(_mul(r, u0[0]), _cmul(kd, v[j])))
        if j == 2:
            a = _cadd(-g, a)
        out.append(_add(v[j], _cmul(dt, a)))
    out += [_add(v[3 + j], _cmul(dt, _cmul(iinv[j], u0[1 + j]))) for j in range(3)]
    return (np.array([float(o.v) for o in out]),
            np.maximum(np.array([float(o.tot) for o in out]) * SECOND, SUBNORMAL))


# ------------------------------------------------------------------------------------ fp32 restatement
MISTAKES = ("step0_new_rates", "prev_rates", "step0_new_velocity", "R_new_attitude", "drag_new_velocity", "drag_sign",
            "wrap_step0", "no_wrap", "gravity_axis1", "Q_sign_swapped", "row2_tan", "literal_jinv02_sign", "noise_ahead",
            "term_on_Hm2")
# the quantity a mistake must push outside the bound ("all": every one of pos, ang and S)
SHOWS_IN = {"step0_new_rates": "ang", "prev_rates": "ang", "step0_new_velocity": "pos", "R_new_attitude": "pos",
            "drag_new_velocity": "pos", "drag_sign": "pos", "wrap_step0": "ang", "no_wrap": "ang", "gravity_axis1": "pos",
            "Q_sign_swapped": "pos", "row2_tan": "yaw", "literal_jinv02_sign": "roll", "noise_ahead": "all",
            "term_on_Hm2": "S"}


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def emulate(u, eps, x0, v0, cfg: Cfg = Cfg(), literal: bool = False, targets=(0.0, 0.0, 0.0), w_stage=100.0, w_term=20.0,
            mistake: Optional[str] = None, noise_rng=None):
    """quad_axis_step and the rollout's cost in float32, operation by operation in the kernel's order (fmaf
    where the source calls it).  sin and cos: the float64 value (+ uniform noise in +-SINCOS_ABS from
    ``noise_rng``) rounded to fp32; 1/c_p: the rounded quotient.  Returns dict(traj (K, H, 6), vel, rate, S)."""
    assert mistake is None or mistake in MISTAKES, mistake
    u = np.asarray(u, F32)
    eps = np.asarray(eps, F32)
    K, H, _ = eps.shape
    dt, im, iinv, kd, g = (F32(c) if np.isscalar(c) else np.asarray(c, F32) for c in cfg.device())
    x = np.asarray(x0, np.float64).astype(F32)
    vv = np.asarray(v0, np.float64).astype(F32)
    p, e = np.tile(x[:3], (K, 1)), np.tile(x[3:], (K, 1))
    v, w = np.tile(vv[:3], (K, 1)), np.tile(vv[3:], (K, 1))
    w_meas = w.copy()
    gv = np.zeros(3, F32)
    gv[1 if mistake == "gravity_axis1" else 2] = -g
    tg = np.broadcast_to(np.asarray(targets, F32), (H, 3))
    two_pi, zero = F32(6.283185307179586), F32(0)

    def sincos(a):
        s, c = np.sin(a.astype(np.float64)), np.cos(a.astype(np.float64))
        if noise_rng is not None:
            s = s + noise_rng.uniform(-SINCOS_ABS, SINCOS_ABS, s.shape)
            c = c + noise_rng.uniform(-SINCOS_ABS, SINCOS_ABS, c.shape)
        return s.astype(F32), c.astype(F32)

    def euler_rates(e, ww, lit):
        s, c = sincos(e)
        sr, sp, cr, cp = s[:, 0], s[:, 1], c[:, 0], c[:, 1]
        ox, oy, oz = ww[:, 0], ww[:, 1], ww[:, 2]
        if lit:
            d0 = ox + sp * oz if mistake == "literal_jinv02_sign" else ox - sp * oz
            d1 = cr * oy + (sr * cp) * oz
            d2 = (cr * cp) * oz - sr * oy
        else:
            ic = (F32(1) / cp).astype(F32)
            f0, f2 = ic * sp, ic
            if mistake == "row2_tan":
                f0, f2 = f2, f0
            d0 = _fma(cr * f0, oz, _fma(sr * f0, oy, ox))
            d1 = _fma(-sr, oz, _fma(cr, oy, zero))
            d2 = _fma(cr * f2, oz, _fma(sr * f2, oy, zero))
        return np.stack([d0, d1, d2], -1)

    def thrust_axis(e):
        s, c = sincos(e)
        sr, sp, sy, cr, cp, cy = s[:, 0], s[:, 1], s[:, 2], c[:, 0], c[:, 1], c[:, 2]
        q0, q1 = (-sy, cy) if mistake == "Q_sign_swapped" else (sy, -cy)
        return np.stack([_fma(cy, sp * cr, q0 * sr), _fma(sy, sp * cr, q1 * sr), cp * cr], -1)

    def wrap(en):
        return en - two_pi * np.rint(en * INV_2PI_32)

    traj, vel, rate = np.zeros((K, H, 6), F32), np.zeros((K, H, 3), F32), np.zeros((K, H, 3), F32)
    stage, term = np.zeros((K, 3), F32), np.zeros((K, 3), F32)
    for t in range(H):
        first = t == 0
        row = eps[:, t]
        if mistake == "noise_ahead":   # (the tile's spare row H: taken as zeros)
            row = eps[:, t + 1] if t + 1 < H else np.zeros_like(eps[:, 0])
        ctl = u[t] + row
        thr, tau = ctl[:, :1], ctl[:, 1:]
        w_old = w
        w = w + dt * (iinv * tau)
        if first:
            ww = w if mistake == "step0_new_rates" else w_meas
        else:
            ww = w_old if mistake == "prev_rates" else w
        en = e + dt * euler_rates(e, ww, literal and not first)
        if (not first and mistake != "no_wrap") or (first and mistake == "wrap_step0"):
            en = wrap(en)
        rj = thrust_axis(en if mistake == "R_new_attitude" else e)
        drag = kd * v
        a = gv + im * (rj * thr - drag) if mistake != "drag_sign" else gv + im * (rj * thr + drag)
        nv = v + dt * a
        if mistake == "drag_new_velocity":   # v_t = v_{t-1} + dt (g + (R f - kd v_t) / m), one fixed-point pass
            nv = v + dt * (gv + im * (rj * thr - kd * nv))
        p = p + dt * (nv if (not first or mistake == "step0_new_velocity") else v)
        v, e = nv, en
        traj[:, t, :3], traj[:, t, 3:], vel[:, t], rate[:, t] = p, e, v, w
        dd = p - tg[t]
        last = (t == H - 2) if mistake == "term_on_Hm2" else (t == H - 1)
        if last:
            term = dd * dd
        else:
            stage = _fma(dd, dd, stage)
    st = (stage[:, 0] + stage[:, 1]) + stage[:, 2]
    tm = (term[:, 0] + term[:, 1]) + term[:, 2]
    return dict(traj=traj, vel=vel, rate=rate, S=(F32(w_stage) * st) + (F32(w_term) * tm))


# -------------------------------------------------------------------------------------------- comparison
@dataclass
class Ratios:
    """Worst err / bound per quantity over the compared elements, and the shares the rules set aside."""
    pos: float
    ang: float
    roll: float
    yaw: float
    S: float
    excluded: float       # share of samples the validity rule drops at some step
    circular: float       # share of angle elements compared modulo 2 pi
    worst: Dict[str, object]

    def of(self, name: str) -> float:
        if name == "all":
            return min(self.pos, self.ang, self.S)
        return getattr(self, name)


def _ratio(err, bound, mask):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isfinite(np.asarray(err, np.float64)), r, np.inf)   # a non-finite value is outside any bound
    r = np.where(mask, r, 0.0)
    return r


def compare(ro: Rollout, traj, S=None, targets=None, w_stage=100.0, w_term=20.0) -> Ratios:
    """traj (K, H, 6) = (p, rpy) and optionally S (K,) against the oracle: every (k, t, channel) the validity
    rule keeps; S of the samples valid to the last step."""
    traj = np.asarray(traj, np.float64)
    K, H, _ = traj.shape
    m3 = np.broadcast_to(ro.valid[..., None], (K, H, 3))
    rp = _ratio(np.abs(traj[..., :3] - ro.pos), ro.bound_p, m3)
    d = np.abs(traj[..., 3:] - ro.ang)
    with np.errstate(invalid="ignore"):
        d = np.where(ro.circ, np.minimum(d, np.abs(2 * math.pi - d)), d)
    re = _ratio(d, ro.bound_e, m3)
    rS = 0.0
    worst = {}
    if S is not None:
        S0, bS = cost(ro.pos, ro.bound_p, targets, w_stage, w_term)[:2]
        r = _ratio(np.abs(np.asarray(S, np.float64) - S0), bS, ro.valid[:, -1])
        rS = float(r.max())
    for name, r, terms in (("pos", rp, ro.terms["pos"]), ("ang", re, ro.terms["ang"])):
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        worst[name] = dict(at=tuple(int(a) for a in i), ratio=float(r[i]),
                           terms={n: float(x) for n, x in zip(TERMS, terms[i])})
    return Ratios(float(rp.max()), float(re.max()), float(re[..., 0].max()), float(re[..., 2].max()), rS,
                  float(1.0 - ro.valid[:, -1].mean()), float((ro.circ & m3).sum() / max(1, m3.sum())), worst)


def exposed(r: Ratios, mistake: str) -> float:
    """err / bound of a planted mistake's run in the quantity named for it."""
    return r.of(SHOWS_IN[mistake])


# ------------------------------------------------------------------------------------------------ designs
HOVER_X, HOVER_V = (0.2, -0.1, 2.5, 0.05, -0.08, 0.7), (0.3, -0.2, 0.1, 0.2, -0.1, 0.05)
HOVER_TARGET = (0.5, 0.4, 3.0)


@dataclass(frozen=True)
class Design:
    """One (state, rates, configuration) with the noise scale, the nominal thrust (None: hover thrust m g), the
    target and the two planted mistakes its GPU case first shows it would catch."""
    name: str
    x: Sequence[float]
    v: Sequence[float]
    exposes: Tuple[str, str]
    cfg: Cfg = Cfg()
    sigma: Tuple[float, float, float, float] = (30.0, 1.0, 1.0, 1.0)
    thrust: Optional[float] = None
    target: Sequence[float] = HOVER_TARGET
    seed: int = 0

    def inputs(self, K: int, H: int, seed: Optional[int] = None):
        """(u (H, 4), eps (K, H, 4)) fp32: the warm start around the nominal thrust and the injected noise."""
        rng = np.random.default_rng(1000 + (self.seed if seed is None else seed))
        thrust = _f(self.cfg.mass) * _f(self.cfg.gravity) if self.thrust is None else self.thrust
        sig = np.asarray(self.sigma, np.float64)
        u = np.zeros((H, 4), F32)
        u[:, 0] = thrust
        u[:, 0] += (rng.normal(0.0, 1.0, H) * sig[0] / 60.0).astype(F32)
        u[:, 1:] += (rng.normal(0.0, 1.0, (H, 3)) * sig[1:] / 2.0).astype(F32)
        eps = (rng.normal(0.0, 1.0, (K, H, 4)) * sig).astype(F32)
        return u, eps

    @property
    def state(self):
        return np.asarray(tuple(self.x) + tuple(self.v), np.float64)


BODY2 = Cfg(dt=0.02, mass=1.2, inertia=(0.01, 0.02, 0.015), kd=0.0, gravity=3.71)
DESIGNS = (
    Design("hover", HOVER_X, HOVER_V, ("step0_new_velocity", "term_on_Hm2")),
    Design("pitch_p120", (0.2, -0.1, 2.5, 2.5, 1.2, -0.4), (0.3, -0.2, 0.1, 0.3, 0.2, -0.1), ("row2_tan", "Q_sign_swapped")),
    Design("pitch_p145", (0.2, -0.1, 2.5, 1.0, 1.45, 0.3), (0.3, -0.2, 0.1, 0.1, -0.15, 0.1), ("row2_tan", "step0_new_rates")),
    Design("pitch_m145", (0.2, -0.1, 2.5, -2.0, -1.45, 2.0), (0.3, -0.2, 0.1, -0.1, -0.1, 0.2), ("R_new_attitude", "prev_rates")),
    Design("yaw_wrap", (0.2, -0.1, 2.5, 0.05, -0.08, 3.1), (0.3, -0.2, 0.1, 0.2, -0.1, 3.0), ("no_wrap", "noise_ahead")),
    Design("roll_cross", (0.2, -0.1, 2.5, 3.13, -0.08, 0.7), (0.3, -0.2, 0.1, 3.0, -0.1, 0.05), ("wrap_step0", "no_wrap")),
    Design("roll_spin", (0.2, -0.1, 2.5, 0.05, -0.08, 0.7), (0.3, -0.2, 0.1, 20.0, -0.1, 0.05), ("no_wrap", "R_new_attitude")),
    Design("tumbling", HOVER_X, HOVER_V, ("prev_rates", "step0_new_rates"), sigma=(30.0, 40.0, 40.0, 40.0)),
    Design("drag_near", (0.1, -0.05, 0.2, 0.05, -0.08, 0.7), (8.0, -3.0, 2.0, 0.2, -0.1, 0.05),
           ("drag_sign", "drag_new_velocity"), cfg=Cfg(kd=5.0)),
    Design("drag_far", (100.0, -98.0, 101.0, 0.05, -0.08, 0.7), (3.0, -2.0, 1.0, 0.2, -0.1, 0.05),
           ("drag_sign", "step0_new_velocity"), cfg=Cfg(kd=0.5), target=(100.5, -97.6, 101.5)),
    Design("big_angles", (0.2, -0.1, 2.5, 48.0, -47.5, 40.0), HOVER_V, ("wrap_step0", "Q_sign_swapped")),
    Design("body2", (0.2, -0.1, 2.5, 0.3, -0.4, 1.1), (0.3, -0.2, 0.1, 0.4, -0.3, 0.2), ("gravity_axis1", "noise_ahead"),
           cfg=BODY2, sigma=(3.0, 0.004, 0.008, 0.006)),
    Design("free_fall", (0.2, -0.1, 2.5, 0.6, -0.5, 0.7), (0.3, -0.2, 0.1, 0.5, -0.4, 0.3), ("gravity_axis1", "term_on_Hm2"),
           sigma=(0.0, 1.0, 1.0, 1.0), thrust=0.0),
    Design("far_target", HOVER_X, HOVER_V, ("step0_new_velocity", "gravity_axis1"), target=(30.2, -40.1, 2.5)),
)
BY_NAME = {d.name: d for d in DESIGNS}
LITERAL_EXPOSES = ("literal_jinv02_sign", "prev_rates")   # what a literal-mode case shows instead of J's own rows
# states a fleet's vehicles cycle through (the default rigid body: a fleet shares one configuration)
FLEET = tuple(d for d in DESIGNS if d.cfg == Cfg() and d.thrust is None and d.name not in ("far_target", "tumbling"))


def exposes(design: Design, literal: bool) -> Tuple[str, str]:
    """The two mistakes a case names: in literal mode J's rows are replaced where they are not run at t >= 1."""
    ms = tuple(m for m in design.exposes if not (literal and m == "row2_tan"))
    return (ms + LITERAL_EXPOSES)[:2] if literal else ms


def helix(start, H: int, step: float = 0.5, turn: float = 0.4):
    """(H, 3) fp32 target rows: a helix of ``step`` metres per row from ``start``, every row different."""
    t = np.arange(1, H + 1, dtype=np.float64)
    r = step * 0.8 / turn
    rows = np.stack([r * np.sin(turn * t), r * (1 - np.cos(turn * t)), 0.6 * step * t], -1) + np.asarray(start, np.float64)
    return rows.astype(F32)


# -------------------------------------------------------------------------------------------- GPU cases
@dataclass(frozen=True)
class Case:
    """One engine call of tests/test_gpu_quad_envelope.py: vehicle v flies designs[v % len(designs)] with its own
    seed, warm start and target.  ``shape``: the block shape launch_quad must pick (wide: 512 threads, one
    dynamics wave; narrow: 256 threads, one; four: 256 threads, four dynamics waves).  ``track``: the target
    moves along a helix (k_rollout_quad_tt)."""
    tag: str
    designs: Tuple[str, ...]
    K: int
    H: int
    V: int = 1
    literal: bool = False
    shape: str = "wide"
    track: bool = False

    def vehicles(self):
        """Per vehicle: (design, u (H, 4), eps (K, H, 4), target (3,) or (H, 3))."""
        out = []
        for v in range(self.V):
            d = BY_NAME[self.designs[v % len(self.designs)]]
            u, eps = d.inputs(self.K, self.H, seed=d.seed + 17 * v)
            tg = np.asarray(d.target, np.float64) + 0.05 * v * np.array([1.0, -1.0, 0.5])
            if self.track:
                tg = helix(np.asarray(d.x[:3]) + 0.01 * v, self.H)
            out.append((d, u, eps, tg.astype(F32)))
        return out


def _mode(lit):
    return "lit" if lit else "J"


DYNAMICS = tuple(Case(f"{d.name}-{_mode(lit)}", (d.name,), 100, 64, literal=lit) for d in DESIGNS for lit in (False, True))
LOOPS = tuple(Case(f"{n}-H{H}-{_mode(lit)}", (n,), 100, H, literal=lit)
              for n in ("hover", "yaw_wrap") for H in (3, 4, 5, 6, 7, 33) for lit in (False, True))
_FLEET = tuple(d.name for d in FLEET)
BLOCKS = (Case("narrow-V1-K8200-H4", ("hover",), 8200, 4, shape="narrow"),
          Case("narrow-V1-K8200-H4-lit", ("yaw_wrap",), 8200, 4, literal=True, shape="narrow"),
          Case("narrow-V40-K250-H8", _FLEET, 250, 8, V=40, shape="narrow"),
          Case("four-V65-K250-H8", _FLEET, 250, 8, V=65, shape="four"),
          Case("four-V70-K232-H8", _FLEET, 232, 8, V=70, literal=True, shape="four"))
TRACK = tuple(Case(f"track-{n}-H{H}-{_mode(lit)}", (n,), 100, H, literal=lit, track=True)
              for n, lit in (("hover", False), ("pitch_p145", False), ("yaw_wrap", True)) for H in (5, 64)) + \
    (Case("track-four-V65-K250-H8", _FLEET, 250, 8, V=65, shape="four", track=True),)
PHILOX = Case("philox-K100-H33", ("hover",), 100, 33)
PHILOX_SIGMA = ((30.0, 0.3, -0.2, 0.1), (0.3, 1.0, 0.2, -0.1), (-0.2, 0.2, 1.2, 0.3), (0.1, -0.1, 0.3, 0.8))
PLAN = tuple((n, H, lit) for n in ("hover", "pitch_p145", "yaw_wrap", "drag_near") for H in (3, 17, 64) for lit in (False, True))


def plan_exposes(design: Design, literal: bool) -> Tuple[str, str]:
    """The two mistakes a plan case names (the plan reads no noise: gravity on axis 1 stands in for the noise row)."""
    return tuple(m for m in exposes(design, literal) + ("gravity_axis1", "step0_new_velocity") if m != "noise_ahead")[:2]
