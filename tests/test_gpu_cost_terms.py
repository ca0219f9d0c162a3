"""The five CostManager terms (covar, center, joint_track, action, joint_limit) of the extended rollout kernels and
k_plan on the GPU against tests/cost_terms_oracle.py, one term at a time: pose weights (0, 0, 0, 0) make the pose cost
exactly 0, so S is the enabled terms alone.  Every bound is that file's (counted there from the kernels' operations;
nothing here is tuned to what the kernels give); tests/test_cost_terms_oracle_cpu.py holds the same cases to the
sizing rules and shows that each planted mistake would fail them.

Each comparison prints its worst err / bound as a JSON row (profiles/cost_terms/README.txt)."""
import json
import re
from dataclasses import replace

import numpy as np
import pytest

import cost_terms_oracle as CT
import pose_envelope as PE
import softmin_oracle as SO

pytestmark = pytest.mark.gpu

WINDOW, ORDER = 9, 2   # the arm's and the whole-body's smoothing (mppi_config_default)


def _log(**row):
    print(json.dumps(dict(side="gpu", **row)))


def _symbol(case, lay, name=None):
    """The rollout symbol a case must run: the extended k_rollout (XC = 1), or the named tracking / self kernel."""
    from quadrotor_manipulator_mppi_amd import _capi as capi
    m = capi.MODEL_WHOLEBODY if case.model == "wholebody" else capi.MODEL_ARM
    f64 = int(case.f64 and case.model == "arm")
    head = f"ILi{m}ELi{case.NA}ELi{lay.nch}ELi{lay.L}ELb{f64}ELb{int(case.V == 1)}E"
    if name is None and case.track:
        name = "k_rollout_tt"
    return re.compile(r"k_rollout(_s)?" + head + "Lb1E" if name is None else name + head + "Ev")


def _engine(case, scene=None, field=None, self_collision=None, **extra):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    cfg = make_config(**dict(case.config(), **extra))
    # what the oracle takes for the device's centring target and limits is what the config holds
    assert np.array_equal(np.float32(cfg.q_center[:7]), CT.KINOVA_QC) and np.array_equal(np.float32(cfg.q_lower[:7]), CT.KINOVA_LO)
    assert np.array_equal(np.float32(cfg.q_upper[:7]), CT.KINOVA_HI)
    e = Engine(cfg, scene=scene, field=field, self_collision=self_collision)   # (zero pose weights are accepted)
    e.set_target(np.float32(PE.TPOS), np.float32(PE.TQUAT))
    for v in range(1, case.V):
        e.set_target(np.float32(PE.TPOS), np.float32(PE.TQUAT), vehicle=v)
    return e


def _set_tables(e, tables, which):
    for v in range(len(tables)):
        e.set_joint_trajectory(tables[v] if which[v] else None, vehicle=v)


def _step(case, e, inps):
    e.set_u_prev(np.stack([i.u for i in inps]))
    return e.step(np.stack([i.state for i in inps]), np.stack([i.eps for i in inps]))


def _check(case, e, inps, st, u0, tag=None, pose=None):
    """S of every vehicle against the oracle on the kept samples, then the finalize given the GPU's own S."""
    tag = tag or case.tag
    S = e.get_costs()
    raw, sm = e.get_weighted_noise()
    lay = SO.layout_of(**case.config())
    out = []
    for v, inp in enumerate(inps):
        assert not st[v].nonfinite, (tag, v)
        o = CT.oracle(inp, pose=None if pose is None else pose[v])
        assert o.excluded <= CT.EXCLUDED_CAP * case.K, (tag, v, o.excluded)
        got = {"S": S[v]}
        if len(case.terms) == 1 and pose is None:   # S is that term, bit for bit
            got[case.terms[0]] = S[v]
        r = CT.compare(o, got)
        _log(case=tag, vehicle=v, excluded=o.excluded, hit=int((o.kept & o.hit).sum()), **{k: round(x, 4) for k, x in r.items()})
        assert np.isfinite(S[v]).all(), (tag, v)
        assert max(r.values()) <= 1.0, (tag, v, r)
        red = SO.reduce(S[v], inp.eps, case.par.lam, WINDOW, ORDER, inp.u)
        bnd = SO.bounds(red, inp.eps, lay)
        fin = dict(w=e.get_weights()[v], w_eps_raw=raw[v], w_eps=sm[v], u_prev=e.get_u_prev()[v], eta=st[v].eta, ess=st[v].ess)
        assert np.float32(st[v].rho) == np.float32(red.rho), (tag, v, st[v].rho, red.rho)
        rs = SO.ratios(fin, red, bnd)
        _log(case=tag, vehicle=v, **{"softmin_" + k: round(x, 4) for k, x in rs.items()})
        assert max(rs.values()) <= 1.0, (tag, v, rs)
        assert np.array_equal(u0[v], fin["u_prev"][0]), (tag, v)
        out.append(o)
    return out


def _fly(case, e=None, name=None, **engine):
    """Create (or take) the case's engine, set what the case sets, step, assert the symbol, check."""
    e = _engine(case, **engine) if e is None else e
    inps = [case.inputs(v) for v in range(case.V)]
    tables = inps[0].tables
    _set_tables(e, tables, [case.table == "all" or (case.table == "v1" and v == 1) for v in range(case.V)])
    out, u0, st = _step(case, e, inps)
    info = e.kernel_info().split("call:")[-1]
    assert _symbol(case, inps[0].lay, name).search(info), (case.tag, info)
    return e, inps, _check(case, e, inps, st, u0)


# ------------------------------------------------------------------------------ ARM, one term per engine
@pytest.mark.parametrize("case", CT.ARM_SINGLE, ids=[c.tag for c in CT.ARM_SINGLE])
def test_arm_one_term(case):
    e, inps, _ = _fly(case)
    lay = inps[0].lay
    shape = case.tag.split("-")[1]
    assert (lay.L, lay.nch, lay.iters) == {"k64h32": (32, 1, 1), "k50h20f32": (32, 1, 1), "k32h96": (64, 2, 1), "k64h64": (64, 1, 1),
                                           "looped": (32, 1, 2)}[shape], lay
    if case.terms == ("track",):   # set_joint_trajectory(None): the zero table again
        e.set_joint_trajectory(None)
        zero = replace(case, table="none")
        zin = [zero.inputs(0)]
        assert not zin[0].tables.any() and np.array_equal(zin[0].eps, inps[0].eps)
        out, u0, st = _step(zero, e, zin)
        _check(zero, e, zin, st, u0, tag=case.tag + "-cleared")
    e.close()


# ------------------------------------------------------------------- ARM, the five together: the sum's order
def test_arm_all_five_on_a_pose_cost():
    """Small pose weights: S = pose + the five in the kernel's order.  The pose cost is the fp32 oracle's under the
    project's relative tolerance (pose_envelope.TOL_S), the terms' bounds on top."""
    case = CT.BY_TAG["arm-all5-pose"]
    e = _engine(case)
    inp = case.inputs(0)
    _set_tables(e, inp.tables, [True])
    out, u0, st = _step(case, e, [inp])
    assert _symbol(case, inp.lay).search(e.kernel_info().split("call:")[-1]), e.kernel_info()
    ref = PE.oracle_arm(PE.kinova_chain(), CT.BASE7, inp.eps, PE.TPOS, PE.TQUAT, w=case.pose, f64=True, u_prev=inp.u,
                        q0=inp.q0.astype(np.float64))
    Sp = ref["S"].numpy().astype(np.float64)
    o = _check(case, e, [inp], st, u0, pose=[(Sp, PE.TOL_S * np.abs(Sp))])[0]
    share = np.median(Sp / o.S)
    _log(case=case.tag, pose_share_of_S=round(float(share), 4))
    assert 0.0 < share < 0.5   # (the terms, not the pose cost, carry the comparison)
    e.close()


def test_arm_all_five_with_target_track():
    case = CT.BY_TAG["arm-all5-track"]
    e = _engine(case)
    t = np.arange(case.H)[:, None] / case.H
    e.set_target_trajectory(np.float32(PE.TPOS) + np.float32(0.2 * t * [1.0, -1.0, 0.5]), np.tile(np.float32(PE.TQUAT), (case.H, 1)))
    _fly(case, e)
    e.close()


# -------------------------------------------------------------------------------------------- WHOLEBODY
@pytest.mark.parametrize("case", CT.WB, ids=[c.tag for c in CT.WB])
def test_wholebody(case):
    e, inps, _ = _fly(case)
    assert (inps[0].lay.L, inps[0].lay.nch) == (64, 1) and not inps[0].diag and inps[0].sigma.shape == (10, 10)
    e.close()


# ------------------------------------------------------------------------------------------------ fleet
def test_fleet_tables_per_vehicle():
    """V = 2, different states: a table for vehicle 1 only (vehicle 0 reads zeros), then for both -- the same engine."""
    one, both = CT.FLEET
    e, inps, _ = _fly(one)
    assert not inps[0].tables[0].any() and inps[1].tables[1].any() and not np.array_equal(inps[0].q0, inps[1].q0)
    _fly(both, e)
    e.close()


# --------------------------------------------------------------------------------------- self engines
def _self_engine_parts(with_field):
    """A scene of two spheres 10 m apart on the base and the last link, paired; no obstacles; a field 5 m from anything."""
    from quadrotor_manipulator_mppi_amd.engine import DistanceField, Scene, SelfCollision
    scene = Scene(((-1, (0.0, 0.0, -10.0), 0.05), (6, (0.0, 0.0, 0.0), 0.05)), penalty=0.0)
    fd = DistanceField.from_function(lambda X, Y, Z: 5.0 + 0.0 * X, (4, 4, 4), 1.0, (-2.0, -2.0, -1.0)) if with_field else None
    return dict(scene=scene, field=fd, self_collision=SelfCollision(((0, 1),), penalty=0.0))


@pytest.mark.parametrize("case,name", list(zip(CT.SELF, ("k_rollout_sc", "k_rollout_sf"))), ids=[c.tag for c in CT.SELF])
def test_self_engines_read_the_weights_late(case, name):
    """The self kernels take w_cen, w_jt, lim_pen and w_cov through late_arg: all five bits, pairs that stay apart (the
    obstacle and self terms add exactly nothing), S against the oracle; then each weight changed through cost_weights
    changes S by that term only."""
    case = replace(case, threads=256)
    parts = _self_engine_parts(name == "k_rollout_sf")
    e, inps, (o,) = _fly(case, name=name, **parts)
    assert np.all(e.get_self_clearances()[0] > 5.0) and np.all(np.isposinf(e.get_clearances()[0]) | (e.get_clearances()[0] > 1.0))
    S1 = e.get_costs()[0].astype(np.float64)
    e.close()
    for fld, term, val in (("w_covar", "covar", 0.9), ("w_center", "center", 0.3), ("w_joint_track", "track", 1.9), ("w_action", "action", 0.05),
                           ("penalty", "limit", 25.0)):
        other = replace(case, par=replace(case.par, **{fld: val}), tag=f"{case.tag}-{fld}")
        e2, _, (o2,) = _fly(other, name=name, **parts)
        S2 = e2.get_costs()[0].astype(np.float64)
        e2.close()
        for t in CT.TERMS:
            assert (t == term) != np.array_equal(o.val[t], o2.val[t]), (fld, t)
        err = np.abs((S2 - S1) - (o2.val[term] - o.val[term]))
        ratio = float(np.where(o.kept, err / (o.bS + o2.bS), 0.0).max())
        _log(case=other.tag, changed=term, dS=round(ratio, 4))
        assert ratio <= 1.0, (fld, ratio)


# ------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("case", CT.PLAN, ids=[c.tag for c in CT.PLAN])
def test_plan_per_step(case):
    """get_plan: the zero-noise rollout of a non-zero u_prev with the table set; cost_t per step and S."""
    inp = case.inputs(0)
    e = _engine(replace(case, K=64))
    _set_tables(e, inp.tables, [True])
    e.set_u_prev(inp.u[None])
    e.set_state(inp.state)
    plan = e.get_plan()
    o = CT.oracle(inp, zero_noise=True)
    assert o.kept_t.all() and o.hit[0] and inp.tables.any() and inp.u.any()
    r = CT.compare(o, {"cost_t": plan.cost_t})
    S, bS = CT.plan_S(o.cost_t[0], o.b_cost_t[0])
    r["S"] = float(abs(float(plan.S[0]) - S) / bS)
    _log(case=case.tag, **{k: round(x, 4) for k, x in r.items()})
    assert np.isfinite(plan.cost_t).all() and max(r.values()) <= 1.0, (case.tag, r)
    e.close()


# ------------------------------------------------------------------------------------------------ batch
def test_batch_with_a_table_equals_hip_steps(monkeypatch):
    """set_joint_trajectory, then run_steps(3) on the default dispatch: u_prev bit for bit what three step calls
    under MPPI_DISPATCH=hip leave (device noise)."""
    case = replace(CT.BY_TAG["arm-all5-track"], track=False, tag="batch")
    inp = case.inputs(0)

    def make(mode):
        if mode:
            monkeypatch.setenv("MPPI_DISPATCH", mode)
        else:
            monkeypatch.delenv("MPPI_DISPATCH", raising=False)
        e = _engine(case, noise="philox", seed=23)
        e.set_joint_trajectory(inp.tables[0])
        e.set_u_prev(inp.u[None])
        e.set_state(inp.state)
        return e

    a = make(None)
    a.run_steps(3)
    a.synchronize()
    ua = a.get_u_prev()
    h = make("hip")
    for _ in range(3):
        h.step(inp.state)
    assert h.dispatch_info().endswith("calls: hip"), h.dispatch_info()
    uh = h.get_u_prev()
    _log(case="batch", dispatch=a.dispatch_info(), kernels=a.kernel_info().split(";")[0])
    assert np.isfinite(ua).all() and not np.array_equal(ua[0], inp.u)
    assert np.array_equal(ua.view(np.uint32), uh.view(np.uint32))
    # and the table is read: without it the batch ends elsewhere
    z = make("hip")
    z.set_joint_trajectory(None)
    for _ in range(3):
        z.step(inp.state)
    assert not np.array_equal(z.get_u_prev(), uh)
    for eng in (a, h, z):
        eng.close()
