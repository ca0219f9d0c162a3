"""Rotor limits on the GPU (mppi_create_limits): k_rollout_quad_b, k_rollout_quad_tt_b, k_rollout_aerial_b, the
bounded plans, the host's clamp of u0 and mppi_set_limits on both dispatch paths, against tests/limits_oracle.py
(the four lines in numpy float32) and, for what the dynamics integrate, tests/quad_oracle.py and
tests/aerial_oracle.py under their own bounds and caps: the oracles are called with u = 0 and eps = the fp32
control of every dim (c on the rotor dims, fl(u + eps) on the joints), so no tolerance here is new.

The bounds of a case are the 15th and 85th percentile of its own fl(u + eps) per rotor dim (limits_oracle.
design_bounds; tests/test_capi_limits_cpu.py holds the designs to 10..20% saturation on each side), so a kernel
that ignores a side, or a dim, fails; every rollout case first shows that the unclamped controls are outside the
oracle's bound on what the engine returned.  Each comparison prints its worst err / bound as a JSON row."""
import json
import os
import subprocess
import sys
import ctypes as C

import numpy as np
import pytest

import aerial_oracle as A
import limits_oracle as LO
import quad_oracle as Q
import softmin_oracle as SO
from conftest import ROOT

pytestmark = pytest.mark.gpu
INF = float("inf")
QSIGMA = np.float32([30.0, 1.0, 1.0, 1.0])


def _log(**row):
    print(json.dumps(dict(side="gpu", **row)))


def _limits(lo, hi):
    from quadrotor_manipulator_mppi_amd.engine import Limits
    return Limits((float(lo[0]), float(hi[0])), tuple((float(lo[a]), float(hi[a])) for a in (1, 2, 3)))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------- stored noise, bit for bit
def _stored_noise_case(model, K, H, sel_blocks, sigma, d, u, seed):
    """A Philox engine with store_noise under the percentile bounds of its own draw: get_noise() on the rotor dims is
    limits_oracle.apply of the library's own draw times sigma, on the other dims the plain draw."""
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config, philox_normals
    A_ = len(sigma)
    kw = dict(model=model, n_samples=K, n_horizon=H, noise="philox", store_noise=True, seed=seed, sigma=sigma, dt=d.cfg.dt,
              quad=d.cfg.quad(False), store_trajectory=False)
    draws = {k0: philox_normals(seed, 0, 0, k0, 64, H, A_)[1] * sigma for k0 in sel_blocks}
    pooled = np.concatenate([draws[k0] for k0 in sel_blocks])
    lo, hi, bounded = LO.design_bounds(u, pooled, sigma)
    assert bounded.all()
    e = Engine(make_config(**kw), limits=_limits(lo, hi))
    if model == "aerial":
        e.set_target(np.float32(d.tpos), np.float32(d.tquat))
    else:
        e.set_target(np.float32(d.target))
    e.set_u_prev(u[None])
    assert e.get_step_counter() == 0
    out, u0, st = e.step(d.state)
    assert not st[0].nonfinite
    got = e.get_noise()[0]
    info = e.kernel_info().split("call:")[-1]
    for k0 in sel_blocks:
        eff, _, ap = LO.controls(u, draws[k0], lo, hi)
        assert (ap.low >= 0.05).all() and (ap.high >= 0.05).all(), (k0, ap.low, ap.high)
        assert np.array_equal(_bits(got[k0:k0 + 64, :, :4]), _bits(eff[..., :4])), (model, K, k0, "rotor dims")
        assert np.array_equal(_bits(got[k0:k0 + 64, :, 4:]), _bits(draws[k0][..., 4:])), (model, K, k0, "joint dims")
        assert not np.array_equal(got[k0:k0 + 64, :, :4], draws[k0][..., :4])
    e.close()
    return info


def test_stored_noise_quadrotor():
    d = Q.BY_NAME["hover"]
    u, _ = d.inputs(1, 20)
    info = _stored_noise_case("quadrotor", 64, 20, (0,), QSIGMA, d, u, 0xB0B)
    assert "k_rollout_quad_bILb1ELb0ELi1ELi512E" in info, info


@pytest.mark.parametrize("K,blocks,sym", [(64, (0,), "ILb1ELb0ELi1ELi512E"), (16400, (0, 8160, 16400 - 64), "ILb1ELb0ELi4ELi256E")],
                         ids=["K64-512", "K16400-four-wave"])
def test_stored_noise_aerial(K, blocks, sym):
    d = A.DESIGNS[0]
    u, _ = d.inputs(1, 20)
    info = _stored_noise_case("aerial", K, 20, blocks, np.float32(A.SIGMA), d, u, 0xA3F1)
    assert "k_rollout_aerial_b" + sym in info, info


# ---------------------------------------------------------- rollouts inside the oracles' own bounds; the finalize
def _check_finalize(tag, v, e, S, eff, u, lo, hi, lay, window, st):
    """The finalize saw eps': softmin_oracle.reduce on the GPU's own S and the effective noise, within that file's
    bounds; and u_prev_old + w_eps_raw, a convex combination of in-bounds controls, within [lo, hi] up to its bound
    on w_eps_raw."""
    red = SO.reduce(S, eff, float(e.cfg.lambda_), window, 2, u)
    bnd = SO.bounds(red, eff, lay)
    raw, sm = e.get_weighted_noise()
    got = dict(w_eps_raw=raw[v], w_eps=sm[v], u_prev=e.get_u_prev()[v], eta=st.eta, ess=st.ess)
    assert np.float32(st.rho) == np.float32(red.rho), (tag, v)
    r = SO.ratios(got, red, bnd)
    _log(case=tag, vehicle=v, **{"softmin_" + k: round(x, 4) for k, x in r.items()})
    assert max(r.values()) <= 1.0, (tag, v, r)
    mean = u[:, :4].astype(np.float64) + raw[v][:, :4].astype(np.float64)
    b = bnd.w_eps_raw[:, :4]
    assert (mean >= lo.astype(np.float64) - b).all() and (mean <= hi.astype(np.float64) + b).all(), (tag, v)


QUAD_CASES = [(d.name, lit, 64, 32) for d in Q.DESIGNS for lit in (False, True)] + [("hover", False, 8208, 32)]


@pytest.mark.parametrize("name,literal,K,H", QUAD_CASES, ids=[f"{n}-{Q._mode(lit)}-K{K}" for n, lit, K, _ in QUAD_CASES])
def test_quadrotor_rollout_inside_the_oracle_bounds(name, literal, K, H):
    """K = 64: one 512-thread block form; K = 8208: the smallest K of the 256-thread form (513 blocks)."""
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    d = Q.BY_NAME[name]
    u, eps = d.inputs(K, H)
    lo, hi, bounded = LO.design_bounds(u, eps, d.sigma)
    kw = dict(model="quadrotor", n_samples=K, n_horizon=H, noise="injected", dt=d.cfg.dt, quad=d.cfg.quad(literal))
    lay = SO.layout_of(**kw)
    wide = lay.nb <= 512
    assert wide == (K == 64)
    e = Engine(make_config(**kw), limits=_limits(lo, hi))
    w = (float(e.cfg.w_stage_pos), float(e.cfg.w_term_pos))
    tg = np.float32(d.target)
    e.set_target(tg)
    e.set_u_prev(u[None])
    out, u0, st = e.step(d.state, eps[None])
    assert f"k_rollout_quad_bILb1ELb{int(literal)}ELi1ELi{512 if wide else 256}E" in e.kernel_info().split("call:")[-1], e.kernel_info()
    assert not st[0].nonfinite
    traj, S = e.get_trajectory()[0], e.get_costs()[0]
    eff, ctl, ap = LO.controls(u, eps, lo, hi)
    assert (ap.low[bounded] >= 0.10).all() and (ap.high[bounded] >= 0.10).all()
    sel = np.arange(K) if K == 64 else np.r_[0:64, K // 2:K // 2 + 64, K - 64:K]   # (the large case: first, middle, last samples)
    zero = np.zeros_like(u)
    ro = Q.rollout(zero, ctl[sel], d.x, d.v, d.cfg, literal)
    r = Q.compare(ro, traj[sel], S[sel], tg, *w)
    _log(case=f"quad-{name}-{Q._mode(literal)}-K{K}", pos=round(r.pos, 4), ang=round(r.ang, 4), S=round(r.S, 4), excluded=r.excluded,
         circular=r.circular)
    assert r.excluded <= Q.EXCLUDED_CAP and r.circular <= Q.CIRCULAR_CAP, (name, r.excluded, r.circular)
    assert max(r.pos, r.ang, r.S) <= 1.0, (name, r)
    # the case can fail: the unclamped controls are outside the bound on what the engine returned
    un = Q.compare(Q.rollout(u, eps[sel], d.x, d.v, d.cfg, literal), traj[sel], S[sel], tg, *w)
    assert max(un.pos, un.ang, un.S) > 1.0, (name, un)
    if K == 64:
        _check_finalize(f"quad-{name}", 0, e, S, eff, u, lo, hi, SO.Layout(R=16, nw=1, iters=1, nb=lay.nb, quad=True),
                        SO.SAVGOL["quadrotor"], st[0])
    e.close()


def test_quadrotor_tracking_rollout_is_bounded():
    """k_rollout_quad_tt_b: the bounded body under a moving target."""
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    d = Q.BY_NAME["hover"]
    K, H = 64, 20
    u, eps = d.inputs(K, H)
    lo, hi, _ = LO.design_bounds(u, eps, d.sigma)
    tg = Q.helix(np.asarray(d.x[:3]), H)
    e = Engine(make_config(model="quadrotor", n_samples=K, n_horizon=H, noise="injected", dt=d.cfg.dt, quad=d.cfg.quad(False),
                           cost_terms=("target_track",)), limits=_limits(lo, hi))
    w = (float(e.cfg.w_stage_pos), float(e.cfg.w_term_pos))
    e.set_target(tg[0])
    e.set_target_trajectory(tg)
    e.set_u_prev(u[None])
    out, u0, st = e.step(d.state, eps[None])
    assert "k_rollout_quad_tt_bILb1ELb0ELi1ELi512E" in e.kernel_info().split("call:")[-1], e.kernel_info()
    traj, S = e.get_trajectory()[0], e.get_costs()[0]
    _, ctl, _ = LO.controls(u, eps, lo, hi)
    r = Q.compare(Q.rollout(np.zeros_like(u), ctl, d.x, d.v, d.cfg, False), traj, S, tg, *w)
    assert max(r.pos, r.ang, r.S) <= 1.0 and r.excluded <= Q.EXCLUDED_CAP, r
    un = Q.compare(Q.rollout(u, eps, d.x, d.v, d.cfg, False), traj, S, tg, *w)
    assert max(un.pos, un.ang, un.S) > 1.0
    e.close()


AERIAL_CASES = A.CASES + (A.Case("K64-H32-V3", 64, 32, V=3, designs=("tilt_a", "tilt_b")),)


@pytest.mark.parametrize("case", AERIAL_CASES, ids=[c.tag for c in AERIAL_CASES])
def test_aerial_rollout_inside_the_oracle_bounds(case, kinova_chain):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    veh = case.vehicles()
    d0 = veh[0][0]
    # the bounds are engine-wide: the percentiles of the vehicles' pooled fl(u + eps)
    pooled = np.concatenate([(u[None] + eps)[..., :4] for _, u, eps in veh])
    lo, hi, _ = LO.design_bounds(np.zeros((case.H, 4), np.float32), pooled, d0.sigma)
    e = Engine(make_config(model="aerial", n_samples=case.K, n_horizon=case.H, n_vehicles=case.V, noise="injected", dt=d0.cfg.dt,
                           quad=d0.cfg.quad(case.literal)), limits=_limits(lo, hi))
    for v, (d, u, eps) in enumerate(veh):
        e.set_target(np.float32(d.tpos), np.float32(d.tquat), vehicle=v)
    e.set_u_prev(np.stack([u for _, u, _ in veh]))
    out, u0, st = e.step(np.stack([d.state for d, _, _ in veh]), np.stack([eps for _, _, eps in veh]))
    sym = f"k_rollout_aerial_bILb{int(case.V == 1)}ELb{int(case.literal)}ELi1ELi512E"
    assert sym in e.kernel_info().split("call:")[-1], e.kernel_info()
    traj, S = e.get_trajectory(), e.get_costs()
    for v, (d, u, eps) in enumerate(veh):
        assert not st[v].nonfinite
        eff, ctl, ap = LO.controls(u, eps, lo, hi)
        assert (ap.low >= 0.05).all() and (ap.high >= 0.05).all(), (case.tag, v, ap.low, ap.high)
        base, q, ee = traj[v][..., :6], traj[v][..., 6:13], traj[v][..., 13:].reshape(case.K, case.H, 4, 4)
        ao = A.rollout(kinova_chain, np.zeros_like(u), ctl, d.state, d.tpos, d.tquat, d.cfg, case.literal)
        r = A.compare(ao, base, q, ee, S[v])
        _log(case="aerial-" + case.tag, vehicle=v, pos=round(r.pos, 4), ang=round(r.ang, 4), q=round(r.q, 4), ee=round(r.ee, 4),
             rot=round(r.rot, 4), S=round(r.S, 4), excluded=r.excluded, circular=r.circular)
        assert r.excluded <= A.EXCLUDED_CAP and r.circular <= A.CIRCULAR_CAP, (case.tag, v, r)
        assert r.worst() <= 1.0, (case.tag, v, r)
        un = A.compare(A.rollout(kinova_chain, u, eps, d.state, d.tpos, d.tquat, d.cfg, case.literal), base, q, ee, S[v])
        assert un.worst() > 1.0, (case.tag, v, un)
        _check_finalize("aerial-" + case.tag, v, e, S[v], eff, u, lo, hi,
                        SO.Layout(R=16, nw=1, iters=1, nb=(case.K + 15) // 16, quad=True), 9, st[v])
        # u0: the raw row 0 clamped on the rotor dims, as it is on the joints; the base's outputs are its first step
        un_ = e.get_u_prev()[v]
        assert np.array_equal(u0[v, :4], np.minimum(np.maximum(un_[0, :4], lo), hi)) and np.array_equal(u0[v, 4:], un_[0, 4:])
        want, b = Q.first_step_outputs(d.x, d.v, u0[v, :4], d.cfg)
        assert (np.abs(out[v, :12] - want) <= b).all(), (case.tag, v)
    e.close()


# ------------------------------------------------------------------------------------------- the output clamp
def test_u0_is_clamped_where_savgol_carries_the_warm_start_past_a_bound():
    from quadrotor_manipulator_mppi_amd import _capi as capi
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    d = Q.BY_NAME["hover"]
    K, H = 64, 20
    cfg = make_config(model="quadrotor", n_samples=K, n_horizon=H, noise="injected", dt=d.cfg.dt, quad=d.cfg.quad(False))
    W = cfg.savgol_window
    row = {5: 2, 9: 4}[W]
    taps = np.zeros(W, np.float32)
    assert capi.lib().mppi_savgol_coefficients(W, cfg.savgol_order, capi.fptr(taps)) == 0
    # row r's share of the smoothed row 0 (softmin_oracle.reduce: mirrored padding, the taps flipped): taps[half - r]
    red = SO.reduce(np.zeros(1, np.float32), np.eye(H, dtype=np.float32)[row][None, :, None], 0.1, W, cfg.savgol_order, np.zeros((H, 1)), taps=taps)
    assert red.w_eps[0, 0] < 0 and red.w_eps[0, 0] == pytest.approx(float(taps[W // 2 - row]), rel=1e-6), (taps, red.w_eps[:, 0])
    lo, hi = np.float32([100.0, -INF, -INF, -INF]), np.float32([400.0, INF, INF, INF])
    u = np.zeros((H, 4), np.float32)
    u[:, 0] = 144.0
    u[0, 0] = lo[0]
    eps = np.zeros((K, H, 4), np.float32)
    eps[:, row, 0] = 50.0
    e = Engine(cfg, limits=_limits(lo, hi))
    e.set_target(np.float32(d.target))
    e.set_u_prev(u[None])
    out, u0, st = e.step(d.state, eps[None])
    raw0 = e.get_u_prev()[0, 0, 0]
    assert raw0 < lo[0] and raw0 == pytest.approx(100.0 + 50.0 * float(red.w_eps[0, 0]), abs=1e-3), raw0   # the raw warm start
    assert u0[0, 0] == lo[0] and np.array_equal(u0[0, 1:], e.get_u_prev()[0, 0, 1:])
    want, b = Q.first_step_outputs(d.x, d.v, u0[0], d.cfg)
    assert (np.abs(out[0, :12] - want) <= b).all()
    raw_want, _ = Q.first_step_outputs(d.x, d.v, e.get_u_prev()[0, 0], d.cfg)
    assert (np.abs(out[0, :12] - raw_want) > b).any(), "the outputs of the raw row would pass too"
    e.close()


# ------------------------------------------------------------------------------------------------- the plan
def _warm_start_outside(d, H):
    """(u with rows outside the bounds, lo, hi, the clamped rows): the design's warm start plus one sample of its noise."""
    u, eps = d.inputs(1, H)
    u2 = (u + eps[0]).astype(np.float32)
    lo, hi, _ = LO.design_bounds(u2, np.zeros((1,) + u2.shape, np.float32), d.sigma)
    _, ctl, ap = LO.controls(u2, np.zeros((1,) + u2.shape, np.float32), lo, hi)
    assert (ap.low >= 0.10).all() and (ap.high >= 0.10).all()
    return u2, lo, hi, ctl[0]


@pytest.mark.parametrize("literal", [False, True], ids=["J", "lit"])
def test_quadrotor_plan_is_the_plan_of_the_clamped_warm_start(literal):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    d, H = Q.BY_NAME["hover"], 20
    u2, lo, hi, ctl = _warm_start_outside(d, H)
    e = Engine(make_config(model="quadrotor", n_samples=64, n_horizon=H, dt=d.cfg.dt, quad=d.cfg.quad(literal)), limits=_limits(lo, hi))
    w = (float(e.cfg.w_stage_pos), float(e.cfg.w_term_pos))
    tg = np.float32(d.target)
    e.set_target(tg)
    e.set_u_prev(u2[None])
    e.set_state(d.state)
    p = e.get_plan().vehicle(0)
    zero = np.zeros((1, H, 4), np.float32)

    def ratios(rows):
        ro = Q.rollout(rows, zero, d.x, d.v, d.cfg, literal)
        assert ro.valid.all()
        S, bS, c_t, b_t, e1, b_e1 = Q.cost(ro.pos[0], ro.bound_p[0], tg, *w)
        ee = np.abs(p.traj[:, 3:].astype(np.float64) - ro.ang[0])
        ee = np.where(ro.circ[0], np.minimum(ee, np.abs(2 * np.pi - ee)), ee)
        return dict(pos=float(np.max(np.abs(p.traj[:, :3].astype(np.float64) - ro.pos[0]) / ro.bound_p[0])),
                    ang=float(np.max(ee / ro.bound_e[0])), cost_t=float(np.max(np.abs(p.cost_t - c_t) / b_t)),
                    pos_err=float(np.max(np.abs(p.pos_err - e1) / b_e1)), S=float(abs(float(p.S) - S) / bS))

    r = ratios(ctl)
    _log(case=f"plan-quad-{Q._mode(literal)}", **{k: round(x, 4) for k, x in r.items()})
    assert max(r.values()) <= 1.0, r
    assert max(ratios(u2).values()) > 1.0, "the plan of the raw warm start would pass too"
    e.close()


def test_aerial_plan_is_the_plan_of_the_clamped_warm_start(kinova_chain):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    d, H = A.DESIGNS[0], 20
    u2, lo, hi, ctl = _warm_start_outside(d, H)
    e = Engine(make_config(model="aerial", n_samples=64, n_horizon=H, dt=d.cfg.dt, quad=d.cfg.quad(False)), limits=_limits(lo, hi))
    e.set_target(np.float32(d.tpos), np.float32(d.tquat))
    e.set_u_prev(u2[None])
    e.set_state(d.state)
    p = e.get_plan().vehicle(0)
    zero = np.zeros((1, H, 11), np.float32)

    def worst(rows):
        ao = A.rollout(kinova_chain, rows, zero, d.state, d.tpos, d.tquat, d.cfg)
        assert ao.valid.all()
        r = A.compare(ao, p.traj[None, :, :6], p.traj[None, :, 6:13], p.traj[None, :, 13:].reshape(1, H, 4, 4), np.float32([p.S]))
        ct = np.abs(p.cost_t - ao.cost_t[0]) / ao.b_cost_t[0]
        perr = np.abs(p.pos_err - ao.pos_err[0]) / A.TOL_PERR_WB
        return max(r.worst(), float(ct.max()), float(perr.max()))

    x = worst(ctl)
    _log(case="plan-aerial", worst=round(x, 4))
    assert x <= 1.0
    assert worst(u2) > 1.0, "the plan of the raw warm start would pass too"
    e.close()


# ---------------------------------------------------------------------------------------------- the identity
@pytest.mark.parametrize("model", ["quadrotor", "aerial"])
def test_infinite_bounds_equal_the_plain_engine_bit_for_bit(model):
    from quadrotor_manipulator_mppi_amd import _capi as capi
    from quadrotor_manipulator_mppi_amd.engine import Engine, Limits, make_config
    d = Q.BY_NAME["hover"] if model == "quadrotor" else A.DESIGNS[0]
    u, _ = d.inputs(1, 32)
    kw = dict(model=model, n_samples=256, n_horizon=32, seed=23, store_noise=True, dt=d.cfg.dt, quad=d.cfg.quad(False))
    plain, open_ = Engine(make_config(**kw)), Engine(make_config(**kw), limits=Limits())
    assert open_.get_limits() == Limits() and plain.get_limits() is None
    with pytest.raises(RuntimeError):
        plain.set_limits(Limits())
    lc = Limits().to_c()
    assert capi.lib().mppi_set_limits(plain._h, C.byref(lc)) == capi.ERR_STATE   # MPPI_ERR_STATE on an engine created without limits
    for e in (plain, open_):
        if model == "aerial":
            e.set_target(np.float32(d.tpos), np.float32(d.tquat))
        else:
            e.set_target(np.float32(d.target))
        e.set_u_prev(u[None])
    for step in range(2):
        a, b = plain.step(d.state), open_.step(d.state)
        assert "_b" not in plain.kernel_info().split("call:")[-1].split(",")[0] and "_bI" in open_.kernel_info().split("call:")[-1]
        assert np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)), step
        for name in ("get_costs", "get_trajectory", "get_noise", "get_u_prev"):
            x, y = getattr(plain, name)(), getattr(open_, name)()
            assert np.isfinite(x).all() and np.array_equal(_bits(x), _bits(y)), (step, name)
    assert not np.array_equal(plain.get_u_prev()[0], u)
    pa, pb = plain.get_plan(), open_.get_plan()
    assert np.array_equal(_bits(pa.traj), _bits(pb.traj)) and np.array_equal(_bits(pa.S), _bits(pb.S))
    plain.close()
    open_.close()


# ---------------------------------------------------------------- set_limits takes effect on the next step
def test_set_limits_takes_effect_on_the_next_control_call():
    """A control call (native packets where the queue is available: the limits buffer is reached through a pointer, no
    resident argument block is rewritten) under the bounds set just before it: the stored noise is the oracle's
    under the new bounds and the warm start the call started from."""
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config, philox_normals
    d = Q.BY_NAME["hover"]
    K, H, seed = 64, 20, 91
    u, _ = d.inputs(1, H)
    e = Engine(make_config(model="quadrotor", n_samples=K, n_horizon=H, seed=seed, store_noise=True, sigma=QSIGMA, dt=d.cfg.dt,
                           quad=d.cfg.quad(False)), limits=_limits([0, -INF, -INF, -INF], [400.0, INF, INF, INF]))
    e.set_target(np.float32(d.target))
    e.set_u_prev(u[None])
    for step, (lo, hi) in enumerate((([120.0, -0.5, -INF, -1.0], [160.0, 0.5, INF, 1.0]), ([130.0, -2.0, -0.2, -INF], [150.0, 2.0, 0.2, INF]),
                                     ([-INF] * 4, [INF] * 4))):
        lo, hi = np.float32(lo), np.float32(hi)
        before = e.get_u_prev()[0]
        e.set_limits(_limits(lo, hi))
        assert e.get_limits() == _limits(lo, hi)
        assert e.get_step_counter() == step
        e.step(d.state)
        draw = philox_normals(seed, step, 0, 0, K, H, 4)[1] * QSIGMA
        ap = LO.apply(before, draw, lo, hi)
        assert np.array_equal(_bits(e.get_noise()[0]), _bits(ap.eps_eff)), (step, e.dispatch_info())
        if step < 2:
            assert ap.low[0] > 0.05 and ap.high[0] > 0.05
    _log(case="set_limits-call", dispatch=e.dispatch_info())
    e.close()


_BATCH_CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import limits_oracle as LO
import quad_oracle as Q
from quadrotor_manipulator_mppi_amd.engine import Engine, Limits, make_config
d = Q.BY_NAME["hover"]
K, H = 64, 20
u = np.zeros((H, 4), np.float32)   # constant rows: SavGol (taps summing to 1, mirrored ends) maps a constant row to itself
u[:, 0] = 144.0
e = Engine(make_config(model="quadrotor", n_samples=K, n_horizon=H, seed=5, dt=d.cfg.dt, quad=d.cfg.quad(False)),
           limits=Limits(thrust=(0.0, 400.0)))
w = (float(e.cfg.w_stage_pos), float(e.cfg.w_term_pos))
tg = np.float32(d.target)
e.set_target(tg)
e.set_u_prev(u[None])
e.set_state(d.state)
e.run_steps(3)
e.synchronize()
wide = float(np.ptp(e.get_costs()[0]))
# bounds of one point: every sample integrates the same controls, whatever the warm start and the draw
point = np.float32([150.0, 0.25, -0.125, 0.0625])
e.set_u_prev(u[None])
e.set_limits(Limits((150.0, 150.0), ((0.25, 0.25), (-0.125, -0.125), (0.0625, 0.0625))))
e.run_steps(3)
e.synchronize()
info, kern = e.dispatch_info(), e.kernel_info()
S, traj = e.get_costs()[0], e.get_trajectory()[0]
ro = Q.rollout(np.zeros((H, 4), np.float32), np.broadcast_to(point, (K, H, 4)), d.x, d.v, d.cfg, False)
r = Q.compare(ro, traj, S, tg, *w)
up = e.get_u_prev()[0]
print(json.dumps(dict(dispatch=info, kernels=kern, wide_ptp=wide, point_ptp=float(np.ptp(S)), same=bool((traj == traj[:1]).all()),
                      worst=max(r.pos, r.ang, r.S), excluded=r.excluded, u_prev_err=float(np.abs(up - point).max()))))
e.close()
"""


def test_set_limits_takes_effect_on_the_next_native_batch():
    """run_steps(3) with MPPI_DISPATCH=aql in a fresh child process: a batch under wide bounds, then set_limits to bounds
    of one point and a second batch.  Its last step's samples all integrate that point (their trajectories are one
    trajectory, the oracle's), and from a warm start of constant rows, after three steps whose every sample's v' is the
    point, the warm start is the point: a batch that had kept the old bounds for any of its steps would leave neither."""
    env = dict(os.environ, MPPI_DISPATCH="aql")
    r = subprocess.run([sys.executable, "-c", _BATCH_CHILD, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    row = json.loads(r.stdout.strip().splitlines()[-1])
    _log(case="set_limits-batch", **row)
    assert row["dispatch"].startswith("aql"), row
    assert "k_rollout_quad_b" in row["kernels"].split(";")[0] and "quiet rollout none" in row["kernels"], row
    assert row["wide_ptp"] > 0 and row["point_ptp"] == 0 and row["same"], row
    assert row["worst"] <= 1.0 and row["excluded"] <= Q.EXCLUDED_CAP, row
    assert row["u_prev_err"] <= 1e-3, row   # (u + sum_k w_k eps'_k and its SavGol of a constant row: roundings of 150 N)


# ------------------------------------------------------------------------------------------ the drop-in classes
def test_dropin_classes_step_within_the_default_bounds():
    import torch
    from quadrotor_manipulator_mppi_amd.engine import Limits
    from quadrotor_manipulator_mppi_amd.mppi_solver import aerial_mppi, quadrotor_mppi
    hi = float(np.float32(2.0) * (np.float32(14.7) * np.float32(9.81)))
    q, a = Q.BY_NAME["hover"], A.DESIGNS[0]
    mq = quadrotor_mppi.MPPI(n_samples=64, n_timestep=20, seed=5, limits=True)
    mq.set_state(q.x[:6], q.v[:6])
    ma = aerial_mppi.MPPI(n_samples=64, n_horizon=20, seed=5, limits=True)
    ma.set_state(a.x, a.v)
    ma.update_joint(a.q, a.qd)
    ma.target_pose.pose = torch.tensor(a.tpos, dtype=torch.float32)
    ma.target_pose.orientation = torch.tensor(a.tquat, dtype=torch.float32)
    for m in (mq, ma):
        m.compute_control_input()
        assert m.get_limits() == Limits(thrust=(0.0, hi)) == m._engine.get_limits()
        assert 0.0 <= float(m.u[0]) <= hi and "_bI" in m._engine.kernel_info().split("call:")[-1]
        tight = Limits(thrust=(150.0, 151.0), torque=((-0.0078125, 0.0078125),) * 3)   # (fp32 values: get_limits returns them as set)
        m.set_limits(tight)
        eng = m._engine
        m.compute_control_input()
        assert m._engine is eng and eng.get_limits() == tight
        un = m.u.numpy()
        assert 150.0 <= un[0] <= 151.0 and (np.abs(un[1:4]) <= 0.0078125).all(), un
        m._engine.close()
