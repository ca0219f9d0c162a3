"""GPU tests of distance-field environments (mppi_create_scene_field, mppi_set_distance_field): the
voxel field's term in the field rollout kernels (k_rollout_df), the plan kernel, the C-ABI and the engine.

A. against the float64 CPU oracle (tests/field_oracle.py), on injected noise, at the smallest shapes
   that reach each kernel form; the grid is 24 x 20 x 16 at 0.05 m.  The field of a case is placed on
   the oracle's own frames of that case (field_oracle.place): a wall slab ahead of the last body
   sphere's path, met near the horizon's end, united with a sphere blob by the mid-chain sphere.
   Before a case looks at the GPU it asserts on the oracle alone that a third of the samples carry the
   field term and that each of five mistakes (axes swapped, cell-centred nodes, nearest node, no radius,
   no origin) would show at more than 100 x the tolerance (field_oracle.assert_case_can_fail).
B. the clamp (spheres leaving the grid) and the indicator (penalty 1e4).
C. identities and updates with no oracle of their own: the cleared and the all-far field against a
   scene engine, a set between two calls, an origin-only update, the dispatch paths, the plan.
D. behaviour: a short closed loop towards a target behind a wall, with and without the field.

Tolerances: field_oracle's docstring.
"""
import numpy as np
import pytest
import torch

import field_oracle as FO
import obstacle_oracle as OO
import pose_envelope as PE
import test_gpu_obstacles as TG
import test_gpu_target_track as TT
import tracking_oracle as TO
from oracle import mppi_oracle as O

pytestmark = pytest.mark.gpu

BASE, HOME, QD = TT.BASE, TT.HOME, TT.QD
ARM_BODY, GEN_BODY, DRONE_BODY = TG.ARM_BODY, TG.GEN_BODY, TG.DRONE_BODY
ARM_STATE, Q_FULL, V_FULL = TG.ARM_STATE, TG.Q_FULL, TG.V_FULL
NO_OBS = OO.Obstacles.of([])


def _desc(field, data=False):
    from quadrotor_manipulator_mppi_amd.engine import DistanceField
    return DistanceField(field.dims, field.voxel, field.origin, field.d if data else None)


def _engine(spec, field, **kw):
    """A field engine with the field's grid and no data yet (field None: a scene engine)."""
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    return Engine(make_config(**kw), scene=TG._scene(spec), field=None if field is None else _desc(field))


# ================================================================================ A. oracle: the arm
ARM_CASES = {
    "f64-h32": dict(K=64, H=32, f64=True),
    "f32-h20-k50": dict(K=50, H=20, f64=False),                                     # pad lanes, a ragged K
    "h96": dict(K=32, H=96, f64=True, blob_gap=0.04, r_blob=0.05, half_w=0.12, s_hint=4000.0),   # two chunks
    "looped": dict(K=64, H=32, f64=True, blocks_per_vehicle=8, block_threads=128),  # iters = 2
    "spheres": dict(K=64, H=32, f64=True, spheres=True),                            # sphere obstacles as well
    "track": dict(K=64, H=32, f64=True, track=True),                                # a moving target as well
    "terms": dict(K=64, H=32, f64=True, cost_terms=("center", "joint_limit"), enabled=("center", "limit"), w_center=0.05),
    # spheres leave the grid: it ends 3 cm short of the hand sphere's end position, and is moved off the base
    "clamp": dict(K=64, H=32, f64=True, shift=(0.0, 0.0, 0.25), clip_last=0.03),
    "indicator": dict(K=64, H=32, f64=True, penalty=OO.PENALTY, sigma=1.0, gap=0.005, blob_gap=0.03),
}


def _arm_case(monkeypatch, name, q_home=None):
    c = dict(ARM_CASES[name])
    K, H, f64 = c.pop("K"), c.pop("H"), c.pop("f64")
    spec = OO.SceneSpec(ARM_BODY, penalty=c.pop("penalty", 0.0))
    terms = O.CostTerms(enabled=c.pop("enabled", ()))
    extra, track, sig = tuple(c.pop("cost_terms", ())), c.pop("track", False), c.pop("sigma", 0.1)
    place_kw = {k: c.pop(k) for k in ("gap", "blob_gap", "r_blob", "half_w", "thick", "shift", "clip_last") if k in c}
    place_kw["s_hint"] = c.pop("s_hint", 1000.0)   # (the pose cost these cases' term rides on)
    spheres, w_cen = c.pop("spheres", False), c.pop("w_center", None)
    if w_cen is not None:   # (a light centering term: S stays small enough for the field term to show)
        terms.centering_weight = w_cen
        c["cost_weights"] = {"w_center": w_cen}
    chain = TT._chain()
    torch.manual_seed(len(name) + H)
    u = torch.randn(H, 7) * 0.05
    noise = O.draw_noise(K, H, torch.eye(7) * sig)
    pos, quat = np.asarray(TG.ARM_TPOS, np.float32), np.asarray(TO.TQUAT, np.float32)
    if track:
        pos, quat = TT._arm_tables(TT._arm_ee0(chain, Q_FULL, f64), H, 0)
    qs = O.integrate((u.unsqueeze(0) + noise).double(), torch.as_tensor(Q_FULL[7:]), torch.as_tensor(V_FULL[6:]), 0.01)
    frames = OO.arm_frames(chain, qs, BASE)
    if not track:   # (the target on the EE's path: a small pose cost, so the term is not lost in TOL_S |S|)
        pos = TG._centre(frames, (len(chain) - 1, (0.0, 0.0, 0.0), 0.0), H // 2).astype(np.float32)
    field = FO.place(frames, spec, H, **place_kw)
    obs = TG._place(frames, spec, H).only([1, 2]) if spheres else NO_OBS   # the moving sphere and the far one
    q_full = Q_FULL if q_home is None else np.array(BASE + list(q_home))

    def step(variant=None, fld=field, o=obs):
        return FO.arm_step(monkeypatch, chain, q_full, V_FULL, u, noise, pos, quat, spec, o, fld, f64=f64, terms=terms,
                           variant=variant)
    eng = dict(model="arm", n_samples=K, n_horizon=H, noise="injected", state_f64=f64,
               cost_terms=(("target_track",) if track else ()) + extra, **c)
    return dict(K=K, H=H, spec=spec, u=u, noise=noise, pos=pos, quat=quat, track=track, obs=obs, field=field, step=step,
                eng=eng, frames=frames, chain=chain)


def _run_arm(c, e, field="case", origin=None, state=ARM_STATE):
    TG._arm_target(c, e)
    if len(c["obs"].radii):
        e.set_obstacles(c["obs"].centers, c["obs"].radii, c["obs"].velocities)
    if isinstance(field, str):   # "case": the case's own field
        e.set_distance_field(c["field"].d, origin)
    elif field is not None:
        e.set_distance_field(field, origin)
    e.set_u_prev(c["u"].numpy())
    return e.step(state, c["noise"].numpy()[None])


def _check_arm(c, e, ref, what, out, u0, st):
    TG._check_clr(e, 0, ref, ref["obs"]["tol_clr"], what)
    u0_tol = TG._check_softmin(e, 0, ref, c["noise"].numpy(), 9, what)
    TT._close(u0[0], ref["u_prev_out"].numpy()[0], atol=u0_tol, what=what + " u0")
    err = float(np.abs(u0[0] - ref["u_prev_out"].numpy()[0]).max()) + 1e-7
    TT._close(out[0, 7:], ref["vdes"], atol=err * 0.01 + 1e-7, what=what + " vdes")
    TT._close(out[0, :7], ref["qdes"], atol=err * 1e-4 + 1e-7, what=what + " qdes")
    assert not st[0].nonfinite


@pytest.mark.parametrize("name", [n for n in ARM_CASES if n not in ("indicator", "clamp")])
def test_arm_field_matches_oracle(monkeypatch, name):
    c = _arm_case(monkeypatch, name)
    what = f"arm field {name}"
    ref = c["step"]()
    FO.assert_case_can_fail(c["step"], ref, what=what)
    if name == "spheres":   # the joint sum and the joint min: both parts present
        assert np.mean(ref["obs"]["S"] - ref["obs"]["S_field"] > 0.0) >= 0.25
    e = _engine(c["spec"], c["field"], **c["eng"])
    out, u0, st = _run_arm(c, e)
    _check_arm(c, e, ref, what, out, u0, st)


def test_arm_spheres_leave_the_grid(monkeypatch):
    """The clamp: the grid is placed so that some body sphere is outside it on at least a quarter of the
    (k, t) rows (asserted on the oracle); the GPU matches the clamped oracle."""
    c = _arm_case(monkeypatch, "clamp")
    ref = c["step"]()
    frac = FO.outside_fraction(c["frames"], c["spec"], c["field"])
    print(f"clamp: some body sphere outside the grid on {100 * frac:.0f}% of the (k, t) rows (need 25%)")
    assert frac >= 0.25
    FO.assert_case_can_fail(c["step"], ref, what="arm field clamp")
    e = _engine(c["spec"], c["field"], **c["eng"])
    out, u0, st = _run_arm(c, e)
    _check_arm(c, e, ref, "arm field clamp", out, u0, st)


def test_arm_field_indicator(monkeypatch):
    """penalty 1e4: S and the sign of clr on the samples whose float64 min |g| is >= 1e-4 m: at least
    95% of K kept, at least 10% of K on each side of the flag (asserted on the oracle)."""
    c = _arm_case(monkeypatch, "indicator")
    K = c["K"]
    ref = c["step"]()
    ob = ref["obs"]
    kept = ob["gabs"] >= 1e-4
    hit = ob["clr"] < 0.0
    print(f"field indicator: kept {kept.sum()} of {K}; hit {np.sum(kept & hit)}, clear {np.sum(kept & ~hit)}")
    assert kept.sum() >= 0.95 * K and np.sum(kept & hit) >= 0.1 * K and np.sum(kept & ~hit) >= 0.1 * K
    e = _engine(c["spec"], c["field"], **c["eng"])
    _, _, st = _run_arm(c, e)
    TG._close_S(e.get_costs()[0], ref, "field indicator", kept)
    clr = e.get_clearances()[0]
    assert np.array_equal(clr[kept] < 0.0, hit[kept])
    TG._check_clr(e, 0, ref, ob["tol_clr"], "field indicator")
    assert not st[0].nonfinite


# ============================================================= generic chain, whole-body, drone, fleet
def test_generic_chain_field_matches_oracle(monkeypatch):
    K, H = 64, 32
    chain_d, chain = PE.GENERIC_CHAIN, PE.joints(PE.GENERIC_CHAIN)
    spec = OO.SceneSpec(GEN_BODY, penalty=0.0)
    q0 = np.array([0.4, -0.7, 0.9, 1.1, 0.05, -0.6, 0.3])
    qd0 = np.array(QD) * np.array([1, 1, 1, 1, 0.2, 1, 1])
    q_full, v_full = np.concatenate([BASE, q0]), np.concatenate([np.zeros(6), qd0])
    torch.manual_seed(10)
    u = torch.randn(H, 7) * 0.05
    noise = O.draw_noise(K, H, torch.eye(7) * 0.1)
    qs = O.integrate((u.unsqueeze(0) + noise).double(), torch.as_tensor(q0), torch.as_tensor(qd0), 0.01)
    field = FO.place(OO.arm_frames(chain, qs, BASE), spec, H)
    step = lambda variant=None: FO.arm_step(monkeypatch, chain, q_full, v_full, u, noise, TO.TPOS, TO.TQUAT, spec, NO_OBS,  # noqa: E731
                                            field, variant=variant)
    ref = step()
    FO.assert_case_can_fail(step, ref, what="generic chain field")
    e = _engine(spec, field, model="arm", n_samples=K, n_horizon=H, noise="injected", chain=chain_d)
    e.set_target(TO.TPOS, TO.TQUAT)
    e.set_distance_field(field.d)
    e.set_u_prev(u.numpy())
    _, _, st = e.step(np.concatenate([BASE, q0, qd0]), noise.numpy()[None])
    TG._check_clr(e, 0, ref, ref["obs"]["tol_clr"], "generic chain field")
    TG._check_softmin(e, 0, ref, noise.numpy(), 9, "generic chain field")
    assert not st[0].nonfinite


def test_wholebody_field_matches_oracle(monkeypatch):
    """K = 32, H = 64: a full 64-lane segment; the base sphere rides on p_drone(k, t)."""
    K, H = 32, 64
    chain = TT._chain()
    rpy = O.base_rpy_from_quat(TT.WB_QUAT)
    spec = OO.SceneSpec(((-1, (0.0, 0.0, 0.15), 0.20),) + ARM_BODY[1:], penalty=0.0)
    torch.manual_seed(64)
    u = torch.randn(H, 10) * 0.05
    noise = O.draw_noise(K, H, torch.from_numpy(TT.WB_SIGMA))
    s0 = torch.as_tensor(np.asarray(TT.WB_X + HOME, np.float64))
    d0 = torch.as_tensor(np.asarray(TG.WB_VX + QD, np.float64))
    qs = O.integrate((u.unsqueeze(0) + noise).double(), s0, d0, 0.01)
    frames = OO.wholebody_frames(chain, qs, rpy.double().numpy())
    tpos = TG._centre(frames, (len(chain) - 1, (0.0, 0.0, 0.0), 0.0), H // 2).astype(np.float32)
    field = FO.place(frames, spec, H, tol_ee=TO.TOL_EE_WB, s_hint=2000.0, r_blob=0.04, half_w=0.1, thick=0.1, blob_gap=0.03)
    step = lambda variant=None: FO.wholebody_step(monkeypatch, chain, TT.WB_X, TG.WB_VX, HOME, QD, rpy, u, noise,  # noqa: E731
                                                  tpos, TO.TQUAT, spec, NO_OBS, field, variant=variant)
    ref = step()
    FO.assert_case_can_fail(step, ref, what="wholebody field")
    e = _engine(spec, field, model="wholebody", n_samples=K, n_horizon=H, noise="injected", sigma=TT.WB_SIGMA)
    e.set_target(tpos, TO.TQUAT)
    e.set_distance_field(field.d)
    e.set_u_prev(u.numpy())
    _, _, st = e.step(np.array(TT.WB_X + TT.WB_QUAT + HOME + TG.WB_VX + QD, np.float64), noise.numpy()[None])
    TG._check_clr(e, 0, ref, ref["obs"]["tol_clr"], "wholebody field")
    TG._check_softmin(e, 0, ref, noise.numpy(), 9, "wholebody field")
    assert not st[0].nonfinite


def test_drone_field_matches_oracle(monkeypatch):
    K, H = 64, 32
    spec = OO.SceneSpec(DRONE_BODY, penalty=0.0)
    torch.manual_seed(32)
    u = torch.randn(H, 3)
    noise = O.draw_noise(K, H, torch.from_numpy(TT.DRONE_SIG))
    traj = O.integrate((noise + u).double(), torch.as_tensor(np.asarray(TT.DRONE_X, np.float64)),
                       torch.as_tensor(np.asarray(TT.DRONE_V, np.float64)), 0.01)
    field = FO.place(OO.drone_frames(traj), spec, H, tol_ee=TO.TOL_POS)
    step = lambda variant=None: FO.drone_step(monkeypatch, TT.DRONE_X, TT.DRONE_V, u, noise, TG.DRONE_TGT, spec, NO_OBS,  # noqa: E731
                                              field, variant=variant)
    ref = step()
    FO.assert_case_can_fail(step, ref, what="drone field")
    e = _engine(spec, field, model="drone", n_samples=K, n_horizon=H, noise="injected", sigma=TT.DRONE_SIG)
    e.set_target(TG.DRONE_TGT)
    e.set_distance_field(field.d)
    e.set_u_prev(u.numpy())
    _, _, st = e.step(np.array(TT.DRONE_X + TT.DRONE_V, np.float64), noise.numpy()[None])
    TG._check_clr(e, 0, ref, ref["obs"]["tol_clr"], "drone field")
    TG._check_softmin(e, 0, ref, noise.numpy(), 5, "drone field")
    assert not st[0].nonfinite


HOME_2 = [1.54, 1.73, 0.03, 4.37, 0.03, 4.68, 0.03]   # the fleet's second state: a few hundredths of a radian off HOME


def test_fleet_one_field_two_states(monkeypatch):
    """V = 2: one engine-wide field, a state per vehicle, each vehicle against its own oracle."""
    c0 = _arm_case(monkeypatch, "f64-h32")
    c1 = _arm_case(monkeypatch, "f64-h32", q_home=HOME_2)
    refs = [c0["step"](), c1["step"](None, c0["field"])]
    FO.assert_case_can_fail(c0["step"], refs[0], what="fleet vehicle 0")
    assert float(np.max(np.abs(refs[0]["obs"]["S"] - refs[1]["obs"]["S"]))) > 1.0   # the two states differ in the term
    assert np.mean(refs[1]["obs"]["S_field"] > 0.0) >= 0.25
    V = 2
    e = _engine(c0["spec"], c0["field"], n_vehicles=V, **c0["eng"])
    for v in range(V):
        TG._arm_target(c0, e, v)
    e.set_distance_field(c0["field"].d)
    e.set_u_prev(np.tile(c0["u"].numpy(), (V, 1, 1)))
    states = np.stack([ARM_STATE, np.concatenate([BASE, HOME_2, QD])])
    e.step(states, np.tile(c0["noise"].numpy()[None], (V, 1, 1, 1)))
    for v in range(V):
        TG._close_S(e.get_costs()[v], refs[v], f"field fleet vehicle {v}")
        TG._check_clr(e, v, refs[v], refs[v]["obs"]["tol_clr"], f"field fleet vehicle {v}")


# ================================================================================== C. identities
def test_cleared_and_far_fields_equal_the_scene_engine(monkeypatch):
    """Before any set, after clear_distance_field() and with d = 10 m everywhere a field engine's S equals
    a scene engine's on the same inputs (rtol 1e-6, as the scene engine against the tracking one)."""
    c = _arm_case(monkeypatch, "spheres")
    scene = _engine(c["spec"], None, **c["eng"])
    _run_arm(c, scene, field=None)
    S_scene, clr_scene = scene.get_costs()[0], scene.get_clearances()[0]
    e = _engine(c["spec"], c["field"], **c["eng"])
    _run_arm(c, e, field=None)
    TT._close(e.get_costs()[0], S_scene, rtol=1e-6, what="field engine before any set vs the scene engine")
    assert np.array_equal(e.get_costs()[0].view(np.uint32), S_scene.view(np.uint32)), "a cleared field adds nothing: the same bits"
    assert np.array_equal(e.get_clearances()[0], clr_scene)
    _run_arm(c, e)
    assert np.max(np.abs(e.get_costs()[0] - S_scene)) > 1.0, "the set field shows"
    e.clear_distance_field()
    _run_arm(c, e, field=None)
    TT._close(e.get_costs()[0], S_scene, rtol=1e-6, what="field engine after clear vs the scene engine")
    assert np.array_equal(e.get_costs()[0].view(np.uint32), S_scene.view(np.uint32))
    assert np.array_equal(e.get_clearances()[0], clr_scene)
    _run_arm(c, e, field=np.full(c["field"].d.shape, 10.0, np.float32))
    TT._close(e.get_costs()[0], S_scene, rtol=1e-6, what="all-far field vs the scene engine")
    assert np.array_equal(e.get_clearances()[0], clr_scene)   # (the spheres are nearer than 10 m)
    # the C entry point's own statuses (the Python wrapper refuses an engine without a field before the call)
    from quadrotor_manipulator_mppi_amd import _capi as capi
    with pytest.raises(RuntimeError):
        scene.set_distance_field(c["field"].d)
    assert capi.lib().mppi_set_distance_field(scene._h, None, capi.fptr(c["field"].d)) == capi.ERR_STATE
    assert capi.lib().mppi_set_distance_field(scene._h, None, None) == capi.ERR_STATE
    bad = np.full(c["field"].d.shape, 10.0, np.float32)
    bad[3, 2, 1] = np.nan
    assert capi.lib().mppi_set_distance_field(e._h, None, capi.fptr(bad)) == capi.ERR_INVALID_ARG
    assert capi.lib().mppi_set_distance_field(e._h, capi.fptr(np.float32([0.0, np.inf, 0.0])), None) == capi.ERR_INVALID_ARG
    with pytest.raises(capi.MPPIError):
        e.set_distance_field(bad)
    _run_arm(c, e, field=None)   # the refused calls changed nothing: still the all-far field
    TT._close(e.get_costs()[0], S_scene, rtol=1e-6, what="after the refused calls")


def test_a_new_field_and_a_new_origin_between_calls(monkeypatch):
    c = _arm_case(monkeypatch, "f64-h32")
    e = _engine(c["spec"], c["field"], **c["eng"])
    _run_arm(c, e, field=np.full(c["field"].d.shape, 10.0, np.float32))
    S_far = e.get_costs()[0].copy()
    _run_arm(c, e)   # set_distance_field between two control calls: in effect on the second
    ref = c["step"]()
    TG._close_S(e.get_costs()[0], ref, "after set_distance_field")
    assert np.max(np.abs(e.get_costs()[0] - S_far)) > 1.0
    # the origin alone: the same data one and a half voxels along x, half a voxel back along z
    moved = FO.Field(c["field"].dims, c["field"].voxel, c["field"].origin + np.float32([0.075, 0.0, -0.025]), c["field"].d)
    ref_m = c["step"](None, moved)
    assert np.max(np.abs(ref_m["S"].numpy() - ref["S"].numpy())) > 1.0
    _run_arm(c, e, origin=moved.origin)
    TG._close_S(e.get_costs()[0], ref_m, "after an origin-only update")
    TG._check_clr(e, 0, ref_m, ref_m["obs"]["tol_clr"], "after an origin-only update")


@pytest.mark.parametrize("model", ["arm", "wholebody"])
def test_field_dispatch_paths_and_batches(monkeypatch, model):
    """K = 256, H = 32, Philox noise: native and HIP dispatch give bit-equal S, clearances and u_prev;
    after run_steps(3) they are the last step's (three single steps of a twin engine end on the same bits)."""
    from quadrotor_manipulator_mppi_amd.engine import DistanceField
    body = ARM_BODY if model == "arm" else ((-1, (0.0, 0.0, 0.15), 0.20),) + ARM_BODY[1:]
    spec = OO.SceneSpec(body)
    if model == "arm":
        state, origin = ARM_STATE, (-0.9, -0.3, 0.9)
    else:
        state, origin = np.array(TT.WB_X + TT.WB_QUAT + HOME + TG.WB_VX + QD, np.float64), tuple(np.array(TT.WB_X) - [0.6, 0.5, 0.2])
    # a floor 0.25 m under the grid's mid-height and a box in it
    fld = DistanceField.from_boxes([((-9.0, -9.0, -9.0), (9.0, 9.0, origin[2] + 0.15)),
                                    ((origin[0] + 0.2, origin[1] + 0.2, origin[2]), (origin[0] + 0.5, origin[1] + 0.5, origin[2] + 0.5))],
                                   FO.DIMS, FO.VOXEL, origin)
    got = {}
    for mode, batch in (("hip", True), ("aql", True), ("hip", False), ("aql", False)):
        monkeypatch.setenv("MPPI_DISPATCH", mode)
        from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
        e = Engine(make_config(model=model, n_samples=256, n_horizon=32, seed=11), scene=TG._scene(spec), field=fld)
        e.set_target(TO.TPOS, TO.TQUAT)
        e.set_state(state)
        for _ in range(1 if batch else 3):
            e.run_steps(3 if batch else 1)
            e.synchronize()
        got[(mode, batch)] = (e.get_costs()[0], e.get_clearances()[0], e.get_u_prev()[0])
        e.close()
    ref = got[("hip", False)]
    assert np.isfinite(ref[1]).all() and ref[1].min() < 0.5, "the field is met"
    for key in (("hip", True), ("aql", True), ("aql", False)):
        for a, b in zip(got[key], ref):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), key


@pytest.mark.parametrize("name", ["f64-h32", "spheres"])
def test_plan_carries_the_field_term(monkeypatch, name):
    """get_plan of a field engine: cost_t minus the no-field plan is the oracle's x on the zero-noise
    rollout, Plan.clearance its per-step min; sum(cost_t) == S."""
    c = _arm_case(monkeypatch, name)
    H = c["H"]
    zero = torch.zeros(1, H, 7)
    ref = FO.arm_step(monkeypatch, c["chain"], Q_FULL, V_FULL, c["u"], zero, c["pos"], c["quat"], c["spec"], c["obs"], c["field"])
    ref0 = FO.arm_step(monkeypatch, c["chain"], Q_FULL, V_FULL, c["u"], zero, c["pos"], c["quat"], c["spec"], c["obs"], None)
    ob = ref["obs"]
    assert np.sum(ob["x"][0] - ref0["obs"]["x"][0] > 0.0) >= H // 8, "the plan must meet the field"
    e = _engine(c["spec"], c["field"], **c["eng"])
    TG._arm_target(c, e)
    if len(c["obs"].radii):
        e.set_obstacles(c["obs"].centers, c["obs"].radii, c["obs"].velocities)
    e.set_u_prev(c["u"].numpy())
    e.set_state(ARM_STATE)
    base = e.get_plan()
    e.set_distance_field(c["field"].d)
    plan = e.get_plan()
    S_ref = float(ref["S"][0])
    tol_S = TO.TOL_S * abs(S_ref) + ob["bound"][0]
    print(f"field plan {name}: S {plan.S[0]:.4f} vs {S_ref:.4f} (tol {tol_S:.2e})")
    assert abs(float(plan.S[0]) - S_ref) <= tol_S
    TT._close(plan.cost_t[0] - base.cost_t[0], ob["x"][0] - ref0["obs"]["x"][0], atol=tol_S, what=f"field plan {name} share of cost_t")
    TT._close(plan.clearance[0], ob["clr_t"][0], atol=ob["tol_clr"], what=f"field plan {name} clearance")
    assert abs(float(plan.cost_t[0].astype(np.float64).sum()) - float(plan.S[0])) <= 1e-5 * abs(float(plan.S[0]))


# ================================================================================== D. behaviour
def test_the_arm_keeps_clear_of_a_wall_on_its_path():
    """60 control calls (K = 1024, H = 32, device noise), each fed its own output as the next state: the
    target lies 0.40 m ahead, behind a wall slab (0.3 m x 0.3 m, 0.2 m thick) whose face stands 0.06 m off
    the hand sphere, across the straight line to the target.  With the field the executed path's min
    clearance to the wall and every call's plan clearance stay > 0; without it (a scene engine, no obstacles) the arm goes through.
    Sized and seeded as test_gpu_obstacles' sphere on the path.  On the CPU oracle (two seeds of its own
    noise) the executed outcomes were +0.007 / +0.017 m with the field (the plans' min over the loop
    +0.009 / +0.018 m) and -0.12 m without.  An unbounded wall at these weights is entered by 3 cm on the
    oracle as on the GPU (the term is a cost, not a barrier, and the arm cannot go round)."""
    chain = TT._chain()
    K, H, N, sig = 1024, 32, 60, 2.0
    spec = OO.SceneSpec(ARM_BODY, w_obs=1000.0, margin=0.10)
    hand = spec.body[-1]
    fk = lambda q: OO.arm_frames(chain, torch.as_tensor(np.asarray(q, np.float64)).view(1, 1, 7), BASE)  # noqa: E731
    fr0 = fk(HOME)
    d = np.array([-0.6, -0.3, -0.74]) / np.linalg.norm([-0.6, -0.3, -0.74])
    tpos = (fr0[7][0, 0, :3, 3].numpy() + 0.40 * d).astype(np.float32)
    tquat = TO.quat_of(fr0[7][0, 0, :3, :3].numpy()).astype(np.float32)
    c_hand = TG._centre(fr0, hand, 0)
    p_mid = c_hand + d * (hand[2] + 0.06 + 0.10)   # a 0.2 m slab, its face 0.06 m ahead of the hand sphere
    e1 = np.cross(d, [0.0, 0.0, 1.0]) / np.linalg.norm(np.cross(d, [0.0, 0.0, 1.0]))
    e2, half = np.cross(d, e1), np.array([0.15, 0.15, 0.10])

    def slab(X, Y, Z):
        L = np.stack([X, Y, Z], -1) - p_mid
        q = np.abs(np.stack([L @ e1, L @ e2, L @ d], -1)) - half
        return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)
    span = FO.VOXEL * (np.asarray(FO.DIMS) - 1.0)
    field = FO.rasterise(slab, FO.DIMS, FO.VOXEL, np.float32(c_hand + 0.1 * d - 0.5 * span))
    got = {}
    for with_field in (True, False):
        e = _engine(spec, field if with_field else None, model="arm", n_samples=K, n_horizon=H,
                    sigma=np.eye(7, dtype=np.float32) * sig, seed=7)
        e.set_target(tpos, tquat)
        if with_field:
            e.set_distance_field(field.d)
        state = np.concatenate([BASE, HOME, np.zeros(7)])
        clr, plan = [], []
        for _ in range(N):
            out, _, st = e.step(state)
            assert not st[0].nonfinite
            state = np.concatenate([BASE, out[0, :7], out[0, 7:14]])
            clr.append(float(FO.term(fk(out[0, :7]), spec, NO_OBS, field, 0.01, TO.TOL_EE)["clr"][0]))
            if with_field:
                plan.append(float(e.get_plan().clearance.min()))
        if with_field:
            print(f"the plans' min clearance over the loop {min(plan):+.4f} m")
            assert min(plan) > 0.0, ("the plan keeps a positive clearance on every call", min(plan))
        got[with_field] = min(clr)
        e.close()
    print(f"executed path's min clearance to the wall: with the field {got[True]:+.4f} m, without {got[False]:+.4f} m")
    assert got[True] > 0.0, got
    assert got[False] < 0.0, got
