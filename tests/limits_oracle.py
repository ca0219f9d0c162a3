"""The rotor limits' arithmetic (include/mppi_hip.h, csrc/mppi_limits.h) in numpy float32, and the bounds the
limits tests place on the oracles' designs.  Test infrastructure only; numpy, no GPU.

For u = u_prev[t][a] and the draw eps, every operation one fp32 operation:
    a0   = fl(u + eps)
    v'   = min(max(a0, lo), hi)
    eps' = (a0 == v') ? eps : fl(v' - u)
    c    = (a0 == v') ? a0  : min(max(fl(u + eps'), lo), hi)
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F32 = np.float32
DIMS = ("thrust", "tau_x", "tau_y", "tau_z")


@dataclass
class Applied:
    eps_eff: np.ndarray   # (K, H, 4) float32
    ctl: np.ndarray       # (K, H, 4) float32
    low: np.ndarray       # (4,): the share of (k, t) whose a0 fell below lo, per dim
    high: np.ndarray      # (4,): the share above hi


def apply(u, eps, lo, hi) -> Applied:
    """u (H, 4), eps (K, H, 4), lo (4,), hi (4,): the four lines in float32, and the saturated share per dim and side."""
    u = np.asarray(u, F32)[None]
    eps = np.asarray(eps, F32)
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    assert u.dtype == eps.dtype == lo.dtype == hi.dtype == F32 and eps.shape[1:] == u.shape[1:] and u.shape[2] == 4
    a0 = u + eps
    v = np.minimum(np.maximum(a0, lo), hi)
    same = a0 == v
    with np.errstate(invalid="ignore"):   # (inf - inf where an infinite u meets an open bound: not a design here)
        e = np.where(same, eps, v - u).astype(F32)
        c = np.where(same, a0, np.minimum(np.maximum(u + e, lo), hi)).astype(F32)
    assert a0.dtype == v.dtype == e.dtype == c.dtype == F32
    n = float(eps.shape[0] * eps.shape[1])
    return Applied(e, c, (a0 < lo).sum((0, 1)) / n, (a0 > hi).sum((0, 1)) / n)


def percentile_bounds(u, eps, q=(15.0, 85.0)):
    """(lo (4,), hi (4,)) float32 at the q-th percentiles of fl(u + eps) over a case, per dim."""
    a0 = (np.asarray(u, F32)[None] + np.asarray(eps, F32)).reshape(-1, 4)
    return np.percentile(a0, q[0], axis=0).astype(F32), np.percentile(a0, q[1], axis=0).astype(F32)


def design_bounds(u, eps, sigma):
    """(lo, hi, bounded) a design is tested under: the 15th / 85th percentile of fl(u + eps) per rotor dim; a dim
    whose noise scale is 0 (every a0 of a row the same number: nothing for a percentile to separate) left open."""
    lo, hi = percentile_bounds(np.asarray(u)[..., :4], np.asarray(eps)[..., :4])
    open_ = np.asarray(sigma)[:4] == 0
    return np.where(open_, F32(-np.inf), lo).astype(F32), np.where(open_, F32(np.inf), hi).astype(F32), ~open_


def controls(u, eps, lo, hi):
    """(eps' spliced into eps, the fp32 control of every dim): dims 0..3 by ``apply``, the rest fl(u + eps).  u (H, A),
    eps (K, H, A), A >= 4."""
    u, eps = np.asarray(u, F32), np.asarray(eps, F32)
    ap = apply(u[:, :4], eps[..., :4], lo, hi)
    eff = eps.copy()
    eff[..., :4] = ap.eps_eff
    ctl = (u[None] + eps).astype(F32)
    ctl[..., :4] = ap.ctl
    return eff, ctl, ap
