"""The 6-DoF quadrotor on the GPU against tests/quad_oracle.py: k_rollout_quad, k_rollout_quad_tt, k_plan's
quadrotor path and the host's quad_outputs, each compared with the float64 recurrence within the running bound
that file derives (its docstring: the constants are counted from quad_axis_step's operations; nothing here is
tuned to what the kernels give).

Every case compares every (k, t, channel) of get_trajectory() the validity rule keeps -- the ragged last
samples included -- and get_costs(), asserts that the stats report nothing non-finite, and first asserts on its
own inputs, on the CPU, that the two planted mistakes named for its design would fail it.  The cases and their
inputs are quad_oracle's tables (DYNAMICS, LOOPS, BLOCKS, TRACK, PHILOX, PLAN); tests/test_quad_oracle_cpu.py
holds the same inputs to the exclusion caps from the reference arithmetic alone.
The block shape of each case is asserted from the layout words (mppi_debug_layout: nb, iters) and from the
symbol the call ran (kernel_info).
With QUAD_ENVELOPE_LOG set every err / bound is appended to that file (profiles/r20/quad_envelope)."""
import json
import os

import numpy as np
import pytest

import quad_oracle as Q
import softmin_oracle as SO

pytestmark = pytest.mark.gpu

SHAPES = {"wide": (1, 512), "narrow": (1, 256), "four": (4, 256)}   # dynamics waves, threads


def _log(row):
    print(json.dumps(row))
    path = os.environ.get("QUAD_ENVELOPE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _config(case, cfg, **extra):
    kw = dict(model="quadrotor", n_samples=case.K, n_horizon=case.H, n_vehicles=case.V, noise="injected", dt=cfg.dt,
              quad=cfg.quad(case.literal))
    if case.track:
        kw["cost_terms"] = ("target_track",)
    kw.update(extra)
    return kw


def _shape(kw):
    """The block shape launch_quad takes for a configuration, from the layout words."""
    lay = SO.layout_of(**kw)
    V = kw.get("n_vehicles", 1)
    assert lay.iters in (1, 4), lay
    return ("four" if lay.iters == 4 else "wide" if lay.nb * V <= 512 else "narrow"), lay


def _assert_discriminates(case, d, u, eps, tg, ro, w):
    for m in Q.exposes(d, case.literal):
        bad = Q.emulate(u, eps, d.x, d.v, d.cfg, case.literal, tg, w[0], w[1], mistake=m)
        r = Q.exposed(Q.compare(ro, bad["traj"], bad["S"], tg, *w), m)
        assert r > 1.0, (case.tag, d.name, "does not expose", m, r)


def _check_vehicle(case, v, d, ro, traj, S, tg, w, st):
    assert not st.nonfinite, (case.tag, v, "stats.nonfinite")
    r = Q.compare(ro, traj, S, tg, *w)
    _log(dict(side="gpu", case=case.tag, vehicle=v, design=d.name, pos=round(r.pos, 4), ang=round(r.ang, 4), S=round(r.S, 4),
              excluded=r.excluded, circular=r.circular, bound_p=float(np.where(ro.valid[..., None], ro.bound_p, 0).max()),
              bound_e=float(np.where(ro.valid[..., None], ro.bound_e, 0).max())))
    assert r.excluded <= Q.EXCLUDED_CAP and r.circular <= Q.CIRCULAR_CAP, (case.tag, v, d.name, r.excluded, r.circular)
    assert max(r.pos, r.ang, r.S) <= 1.0, (case.tag, v, d.name, r)
    return r


def _check_outputs(case, d, out, u0):
    want, b = Q.first_step_outputs(d.x, d.v, u0, d.cfg)
    err = np.abs(np.asarray(out[:12], np.float64) - want)
    _log(dict(side="gpu", case=case.tag, design=d.name, outputs=round(float(np.max(err / b)), 4)))
    assert (err <= b).all(), (case.tag, d.name, "outputs", err / b)


def _check_reduction(case, lay, e, v, S, eps, u, st, got):
    """The record-derived quantities against softmin_oracle.reduce on the GPU's own S, within that file's bound."""
    lam = float(e.cfg.lambda_)
    red = SO.reduce(S, eps, lam, SO.SAVGOL["quadrotor"], 2, u)
    bnd = SO.bounds(red, eps, SO.Layout(R=16, nw=SHAPES[case.shape][0], iters=1, nb=lay.nb, quad=True))
    assert np.float32(st.rho) == np.float32(red.rho), (case.tag, v, st.rho, red.rho)
    r = SO.ratios(dict(got, eta=st.eta, ess=st.ess), red, bnd)
    _log(dict(side="gpu", case=case.tag, vehicle=v, **{"softmin_" + k: round(x, 4) for k, x in r.items()}))
    assert max(r.values()) <= 1.0, (case.tag, v, r)


def _fly(case):
    """One control call of a case, every vehicle against its own oracle: (engine, vehicles, oracles, weights)."""
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    veh = case.vehicles()
    cfg = veh[0][0].cfg
    kw = _config(case, cfg)
    shape, lay = _shape(kw)
    assert shape == case.shape, (case.tag, shape, lay)
    e = Engine(make_config(**kw))
    w = (float(e.cfg.w_stage_pos), float(e.cfg.w_term_pos))
    oracles = []
    for v, (d, u, eps, tg) in enumerate(veh):
        assert d.cfg == cfg, "a fleet shares one rigid body"
        ro = Q.rollout(u, eps, d.x, d.v, d.cfg, case.literal)
        if v == 0:
            _assert_discriminates(case, d, u, eps, tg, ro, w)
        oracles.append(ro)
        e.set_target(tg[0] if case.track else tg, vehicle=v)
        if case.track:
            e.set_target_trajectory(tg, vehicle=v)
    U0 = np.stack([u for _, u, _, _ in veh])
    EPS = np.stack([eps for _, _, eps, _ in veh])
    e.set_u_prev(U0)
    out, u0, st = e.step(np.stack([d.state for d, _, _, _ in veh]), EPS)
    nw, nt = SHAPES[shape]
    sym = f"k_rollout_quad{'_tt' if case.track else ''}ILb{int(case.V == 1)}ELb{int(case.literal)}ELi{nw}ELi{nt}E"
    assert sym in e.kernel_info().split("call:")[-1], (case.tag, sym, e.kernel_info())
    traj, S = e.get_trajectory(), e.get_costs()
    assert traj.shape == (case.V, case.K, case.H, 6)
    for v, (d, u, eps, tg) in enumerate(veh):
        _check_vehicle(case, v, d, oracles[v], traj[v], S[v], tg, w, st[v])
    if case.V == 1:
        _check_outputs(case, veh[0][0], out[0], u0[0])
    else:
        wts, (raw, sm), un = e.get_weights(), e.get_weighted_noise(), e.get_u_prev()
        for v, (d, u, eps, tg) in enumerate(veh):
            _check_reduction(case, lay, e, v, S[v], eps, u, st[v], dict(w=wts[v], w_eps_raw=raw[v], w_eps=sm[v], u_prev=un[v]))
    return e, veh, oracles, w


# ------------------------------------------------------------------------- the dynamics designs, K = 100, H = 64
@pytest.mark.parametrize("case", Q.DYNAMICS, ids=[c.tag for c in Q.DYNAMICS])
def test_dynamics_designs_inside_the_bound(case):
    _fly(case)[0].close()


# ------------------------------------------------------------------- the tails of the by-four step loop, H = 3 .. 33
@pytest.mark.parametrize("case", Q.LOOPS, ids=[c.tag for c in Q.LOOPS])
def test_loop_shapes_inside_the_bound(case):
    _fly(case)[0].close()


# --------------------------------------------------- 256-thread blocks of one and of four dynamics waves; the fleets
@pytest.mark.parametrize("case", Q.BLOCKS, ids=[c.tag for c in Q.BLOCKS])
def test_block_shapes_inside_the_bound(case):
    _fly(case)[0].close()


# ------------------------------------------------------------------------------------------------ device noise
def test_device_noise_tile_is_the_stored_noise():
    """Philox noise through a non-diagonal Sigma, stored and read back: the trajectory and S are the oracle's
    on the stored eps, so the LDS tile the dynamics read is what the full-matrix path stored."""
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    case = Q.PHILOX
    d, u, _, tg = case.vehicles()[0]
    kw = _config(case, d.cfg, noise="philox", sigma=np.asarray(Q.PHILOX_SIGMA, np.float32), store_noise=True, seed=77)
    shape, _ = _shape(kw)
    assert shape == "wide"
    e = Engine(make_config(**kw))
    w = (float(e.cfg.w_stage_pos), float(e.cfg.w_term_pos))
    e.set_target(tg)
    e.set_u_prev(u[None])
    out, u0, st = e.step(d.state)
    eps = e.get_noise()[0]
    assert np.isfinite(eps).all() and np.abs(eps[..., 1:]).max() > 0.5, "no stored noise"
    # the full matrix mixes the columns: eps is not a diagonal scaling of four independent normals
    c = np.corrcoef(eps.reshape(-1, 4).T)
    assert abs(c[1, 2]) > 0.05, c
    ro = Q.rollout(u, eps, d.x, d.v, d.cfg, case.literal)
    _assert_discriminates(case, d, u, eps, tg, ro, w)
    shifted = Q.rollout(u, np.roll(eps, 1, axis=0), d.x, d.v, d.cfg, case.literal)   # (a tile of another sample's noise fails)
    assert Q.compare(shifted, e.get_trajectory()[0]).pos > 1.0
    _check_vehicle(case, 0, d, ro, e.get_trajectory()[0], e.get_costs()[0], tg, w, st[0])
    _check_outputs(case, d, out[0], u0[0])
    e.close()


# ------------------------------------------------------------------------------------------------ the plan kernel
def _check_plan(tag, p, ro, tg, w):
    """Planes, cost_t, pos_err and S of one vehicle's plan against the oracle's zero-noise sample."""
    assert ro.valid.all(), tag
    S, bS, c_t, b_t, e1, b_e1 = Q.cost(ro.pos[0], ro.bound_p[0], tg, *w)
    ep = np.abs(p.traj[:, :3].astype(np.float64) - ro.pos[0])
    ee = np.abs(p.traj[:, 3:].astype(np.float64) - ro.ang[0])
    ee = np.where(ro.circ[0], np.minimum(ee, np.abs(2 * np.pi - ee)), ee)
    r = dict(pos=float(np.max(ep / ro.bound_p[0])), ang=float(np.max(ee / ro.bound_e[0])),
             cost_t=float(np.max(np.abs(p.cost_t - c_t) / b_t)), pos_err=float(np.max(np.abs(p.pos_err - e1) / b_e1)),
             S=float(abs(float(p.S) - S) / bS))
    _log(dict(side="gpu", case=tag, **{k: round(x, 4) for k, x in r.items()}))
    assert np.isfinite(p.traj).all() and np.isfinite(p.cost_t).all()
    assert max(r.values()) <= 1.0, (tag, r)


@pytest.mark.parametrize("name,H,literal", Q.PLAN, ids=[f"{n}-H{H}-{Q._mode(lit)}" for n, H, lit in Q.PLAN])
def test_plan_inside_the_bound(name, H, literal):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    d = Q.BY_NAME[name]
    u, _ = d.inputs(1, H)
    zero = np.zeros((1, H, 4), np.float32)
    tag = f"plan-{name}-H{H}-{Q._mode(literal)}"
    e = Engine(make_config(model="quadrotor", n_samples=64, n_horizon=H, dt=d.cfg.dt, quad=d.cfg.quad(literal)))
    w = (float(e.cfg.w_stage_pos), float(e.cfg.w_term_pos))
    tg = np.asarray(d.target, np.float32)
    ro = Q.rollout(u, zero, d.x, d.v, d.cfg, literal)
    for m in Q.plan_exposes(d, literal):   # the mistakes, on the plan's own inputs
        bad = Q.emulate(u, zero, d.x, d.v, d.cfg, literal, tg, *w, mistake=m)
        assert Q.exposed(Q.compare(ro, bad["traj"], bad["S"], tg, *w), m) > 1.0, (tag, m)
    e.set_target(tg)
    e.set_u_prev(u[None])
    e.set_state(d.state)
    _check_plan(tag, e.get_plan().vehicle(0), ro, tg, w)
    e.close()


# ------------------------------------------------------------------------------------------------ a moving target
@pytest.mark.parametrize("case", Q.TRACK, ids=[c.tag for c in Q.TRACK])
def test_tracking_inside_the_bound(case):
    """k_rollout_quad_tt under a helix of 0.5 m per row: S against the cost over the rows, and the plan's
    pos_err and cost_t against row t."""
    e, veh, oracles, w = _fly(case)
    for v, (d, u, eps, tg) in enumerate(veh):
        if case.V > 1:   # a row off by one, or another vehicle's table, is far outside the bound
            other = np.roll(tg, 1, axis=0)
            assert Q.compare(oracles[v], e.get_trajectory()[v], e.get_costs()[v], other, *w).S > 1.0
    e.set_u_prev(np.stack([u for _, u, _, _ in veh]))
    plan = e.get_plan()
    for v, (d, u, eps, tg) in enumerate(veh):
        ro = Q.rollout(u, np.zeros((1, case.H, 4), np.float32), d.x, d.v, d.cfg, case.literal)
        _check_plan(f"{case.tag}-plan-v{v}", plan.vehicle(v), ro, tg, w)
    e.close()
