"""GPU tests of obstacle avoidance (mppi_create_scene, mppi_set_obstacles): the sphere scene's term in
the scene rollout kernels (k_rollout_ob), the plan kernel, the C-ABI and the engine.

A. against the float64 CPU oracle (tests/obstacle_oracle.py), on injected noise, at the smallest shapes
   that reach each code path.  The obstacles of a case are placed on the oracle's own frames of that
   case (``_place``): a static one half a margin off the last body sphere at the horizon's end, one
   crossing the mid-chain sphere's neighbourhood at 1 m/s, one 10 m away.  Before a case looks at the
   GPU it asserts on the oracle alone that a third of the samples carry the term and that each of four
   mistakes (row time t for t + 1, frames shifted by one, no margin, no offsets) would show at more than
   100 x the tolerance (obstacle_oracle.assert_case_can_fail).
B. the indicator (penalty 1e4): S compared where the float64 min |g| is >= 1e-4 m.
C. identities with no oracle: no obstacles, the far obstacle, the plain tracking engine, the dispatch
   paths, batches, a new set between calls, the plan.
D. behaviour: 60 closed-loop control calls past an obstacle on the hand's path, with and without the scene.

Tolerances: obstacle_oracle's docstring (the project's own, tests/tracking_oracle.py).
"""
import numpy as np
import pytest
import torch

import obstacle_oracle as OO
import pose_envelope as PE
import test_gpu_target_track as TT
import tracking_oracle as TO
from oracle import mppi_oracle as O

pytestmark = pytest.mark.gpu

BASE, HOME, QD = TT.BASE, TT.HOME, TT.QD
FAR = ((10.0, 10.0, 10.0), 0.5, (0.0, 0.0, 0.0))
# nine body spheres on the Kinova chain's frames -1 .. 7 (0: the fixed joint the base swallows)
ARM_BODY = ((-1, (0.0, 0.0, -0.05), 0.09), (0, (0.0, 0.02, 0.08), 0.07), (1, (0.0, 0.0, 0.0), 0.05),
            (2, (0.0, -0.1, 0.0), 0.05), (3, (0.0, 0.03, -0.04), 0.05), (4, (0.0, 0.1, 0.0), 0.05),
            (5, (0.0, 0.0, 0.0), 0.05), (6, (0.0, 0.0, 0.0), 0.05), (7, (0.0, 0.0, -0.1), 0.04))
# the ten-joint generic chain: spheres on the mid-chain fixed joint's frame (3) and the prismatic joint's (5)
GEN_BODY = ((-1, (0.0, 0.0, 0.0), 0.08), (0, (0.0, 0.03, 0.0), 0.06), (1, (0.0, 0.0, 0.0), 0.05), (3, (0.02, 0.0, -0.05), 0.05),
            (4, (0.02, 0.0, -0.03), 0.05), (5, (0.0, 0.0, 0.1), 0.05), (7, (0.0, 0.0, 0.0), 0.05), (9, (0.0, 0.0, -0.08), 0.04))
DRONE_BODY = ((-1, (0.0, 0.0, 0.0), 0.30), (-1, (0.2, 0.0, -0.1), 0.10))


def _scene(spec):
    from quadrotor_manipulator_mppi_amd.engine import Scene
    return Scene(spec.body, spec.w_obs, spec.margin, spec.penalty)


def _engine(spec, **kw):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    return Engine(make_config(**kw), scene=None if spec is None else _scene(spec))


def _centre(frames, b, t):
    """The mean over the samples of body sphere b's centre at row t (float64)."""
    f, o, _ = b
    T = frames[f].double()
    c = T[:, t, :3, :3] @ torch.as_tensor(np.asarray(o, np.float64)) + T[:, t, :3, 3]
    return c.mean(dim=0).numpy()


def _place(frames, spec, H, dt=0.01, gap=None, end_gap=-0.12, r_move=0.10):
    """The case's three obstacles on the oracle's frames (module docstring).  gap: the static
    obstacle's clearance to the last sphere's mean position at the horizon's end (default: half the
    margin).  The moving one comes in at 1 m/s along the line through the mid-chain sphere's centre and
    stands at clearance end_gap to that sphere's mean end position at row H - 1: the hinge it leaves at
    the horizon's end is what tells row time t from t + 1 (over a whole pass the two sums telescope)."""
    gap = 0.5 * spec.margin if gap is None else gap
    last, mid = spec.body[-1], spec.body[len(spec.body) // 2]
    # the static one ahead of the last sphere, on its line of motion: met at the horizon's end only
    n1 = _centre(frames, last, H - 1) - _centre(frames, last, 0)
    n1 = n1 / np.linalg.norm(n1) if np.linalg.norm(n1) > 1e-6 else np.array([0.48, 0.6, 0.64])
    c_static = _centre(frames, last, H - 1) + n1 * (last[2] + 0.05 + gap)
    # the moving one from outside, along the line from the first sphere (the base) through the mid one
    n2 = _centre(frames, mid, H - 1) - _centre(frames, spec.body[0], H - 1)
    n2 = n2 / np.linalg.norm(n2) if np.linalg.norm(n2) > 1e-6 else np.array([0.0, -0.6, 0.8])
    vel = -1.0 * n2
    c_end = _centre(frames, mid, H - 1) + n2 * (mid[2] + r_move + end_gap)
    c_move = c_end - vel * H * dt
    return OO.Obstacles.of([(c_static, 0.05, (0.0, 0.0, 0.0)), (c_move, r_move, vel), FAR])


def _close_S(S, ref, what, kept=None):
    S_ref, ob = ref["S"].double().numpy(), ref["obs"]
    lim = TO.TOL_S * np.abs(S_ref) + ob["bound"]
    err = np.abs(np.asarray(S, np.float64) - S_ref)
    if kept is not None:
        err, lim = err[kept], lim[kept]
    print(f"{what} S: max err / bound {np.max(err / lim):.3f}, max err {err.max():.3e}, n_act max {ob['n_act'].max():.0f}")
    assert np.all(err <= lim), f"{what} S: {np.sum(err > lim)} / {err.size} beyond TOL_S |S| + w_obs TOL_C n_act"


def _check_softmin(e, v, ref, noise, window, what):
    """tests/test_gpu_target_track.py's _check_softmin with the S comparison under this term's bound."""
    noise = np.asarray(noise)
    S, S_ref = e.get_costs()[v], ref["S"].numpy()
    _close_S(S, ref, what)
    srt = np.sort(S_ref.astype(np.float64))
    gap = float(srt[1] - srt[0])
    raw, sm = e.get_weighted_noise()
    raw, sm, u_new = raw[v], sm[v], e.get_u_prev()[v]
    # (a) the reduction given the GPU's own costs
    w_own = O.softmin(torch.from_numpy(S), TO.LAM).numpy()
    TT._close(e.get_weights()[v], w_own, rtol=1e-5, atol=1e-9, what=what + " w | S_gpu")
    TT._close(raw, np.einsum("k,kha->ha", w_own.astype(np.float64), noise), rtol=1e-5, atol=1e-7, what=what + " w_eps | S_gpu")
    # (b) end to end within the softmin's conditioning
    dS = float(np.max(np.abs(S.astype(np.float64) - S_ref)))
    bound = TT._amplified_bound(dS, ref["w"].numpy().astype(np.float64), noise, TO.LAM)
    print(f"{what}: top-2 cost gap {gap:.3f}, max |dS| {dS:.3e}")
    assert np.all(np.abs(raw - ref["w_eps_raw"].numpy()) <= bound), what + ": w_eps beyond the conditioning bound"
    sm_bound = np.abs(O.savgol(torch.from_numpy(bound.astype(np.float32)), window, 2).numpy()) + 4 * bound.max()
    assert np.all(np.abs(sm - ref["w_eps"].numpy()) <= sm_bound), what + ": SavGol(w_eps) beyond the bound"
    TT._close(u_new, ref["u_prev_out"].numpy(), atol=float(sm_bound.max()) + 1e-6, what=what + " u_prev")
    return float(sm_bound.max()) + 1e-6


def _check_clr(e, v, ref, tol, what):
    clr = e.get_clearances()[v].astype(np.float64)
    err = np.abs(clr - ref["obs"]["clr"])
    print(f"{what} clearance: max err {err.max():.3e} (tol {tol:.1e}), range {clr.min():.4f} .. {clr.max():.4f}")
    assert np.all(err <= tol), what


# ================================================================================ A. oracle: the arm
ARM_STATE = np.concatenate([BASE, HOME, QD])
# (a target position near the EE's path: a small pose cost, so the term is not lost in TOL_S |S|)
ARM_TPOS = [-0.3, 0.3, 1.0]
Q_FULL, V_FULL = np.array(BASE + HOME), np.array([0.0] * 6 + QD)

ARM_CASES = {
    "f64-h32": dict(K=64, H=32, f64=True),
    "f32-h20-k50": dict(K=50, H=20, f64=False),                                     # pad lanes, a ragged K
    "h96": dict(K=32, H=96, f64=True, r_move=0.13, end_gap=-0.15, gap=0.045),                                            # two chunks
    "looped": dict(K=64, H=32, f64=True, blocks_per_vehicle=8, block_threads=128),  # iters = 2
    "track": dict(K=64, H=32, f64=True, track=True),                                # a moving target as well
    "terms": dict(K=64, H=32, f64=True, cost_terms=("center", "joint_limit"), enabled=("center", "limit"), w_center=0.05),
    "indicator": dict(K=64, H=32, f64=True, penalty=OO.PENALTY, sigma=1.0, gap=0.03, end_gap=-0.002),
}


def _arm_case(monkeypatch, name):
    c = dict(ARM_CASES[name])
    K, H, f64 = c.pop("K"), c.pop("H"), c.pop("f64")
    spec = OO.SceneSpec(ARM_BODY, penalty=c.pop("penalty", 0.0))
    terms = O.CostTerms(enabled=c.pop("enabled", ()))
    extra, track, sig, gap = tuple(c.pop("cost_terms", ())), c.pop("track", False), c.pop("sigma", 0.1), c.pop("gap", None)
    end_gap, r_move, w_cen = c.pop("end_gap", -0.12), c.pop("r_move", 0.10), c.pop("w_center", None)
    if w_cen is not None:   # (a light centering term: S stays small enough for the obstacle term to show)
        terms.centering_weight = w_cen
        c["cost_weights"] = {"w_center": w_cen}
    chain = TT._chain()
    torch.manual_seed(len(name) + H)
    u = torch.randn(H, 7) * 0.05
    noise = O.draw_noise(K, H, torch.eye(7) * sig)
    pos, quat = np.asarray(ARM_TPOS, np.float32), np.asarray(TO.TQUAT, np.float32)
    if track:
        pos, quat = TT._arm_tables(TT._arm_ee0(chain, Q_FULL, f64), H, 0)
    qs = O.integrate((u.unsqueeze(0) + noise).double(), torch.as_tensor(Q_FULL[7:]), torch.as_tensor(V_FULL[6:]), 0.01)
    frames = OO.arm_frames(chain, qs, BASE)
    if not track:   # (the target on the EE's path: a small pose cost, so the term is not lost in TOL_S |S|)
        pos = _centre(frames, (len(chain) - 1, (0.0, 0.0, 0.0), 0.0), H // 2).astype(np.float32)
    obs = _place(frames, spec, H, gap=gap, end_gap=end_gap, r_move=r_move)
    step = lambda variant=None, o=obs: OO.arm_step(monkeypatch, chain, Q_FULL, V_FULL, u, noise, pos, quat, spec, o,  # noqa: E731
                                                    f64=f64, terms=terms, variant=variant)
    eng = dict(model="arm", n_samples=K, n_horizon=H, noise="injected", state_f64=f64,
               cost_terms=(("target_track",) if track else ()) + extra, **c)
    return dict(K=K, H=H, spec=spec, u=u, noise=noise, pos=pos, quat=quat, track=track, obs=obs, step=step, eng=eng)


def _arm_target(c, e, vehicle=0):
    if c["track"]:
        e.set_target(ARM_TPOS, TO.TQUAT, vehicle=vehicle)
        e.set_target_trajectory(c["pos"], c["quat"], vehicle=vehicle)
    else:
        e.set_target(c["pos"], c["quat"], vehicle=vehicle)


def _run_arm(c, e, obs=None):
    obs = c["obs"] if obs is None else obs
    _arm_target(c, e)
    e.set_obstacles(obs.centers, obs.radii, obs.velocities)
    e.set_u_prev(c["u"].numpy())
    return e.step(ARM_STATE, c["noise"].numpy()[None])


@pytest.mark.parametrize("name", [n for n in ARM_CASES if n != "indicator"])
def test_arm_scene_matches_oracle(monkeypatch, name):
    c = _arm_case(monkeypatch, name)
    what = f"arm {name}"
    ref = c["step"]()
    OO.assert_case_can_fail(c["step"], ref, what=what)
    e = _engine(c["spec"], **c["eng"])
    out, u0, st = _run_arm(c, e)
    _check_clr(e, 0, ref, OO.tol_c_max(c["spec"], TO.TOL_EE), what)
    u0_tol = _check_softmin(e, 0, ref, c["noise"].numpy(), 9, what)
    TT._close(u0[0], ref["u_prev_out"].numpy()[0], atol=u0_tol, what=what + " u0")
    err = float(np.abs(u0[0] - ref["u_prev_out"].numpy()[0]).max()) + 1e-7
    TT._close(out[0, 7:], ref["vdes"], atol=err * 0.01 + 1e-7, what=what + " vdes")
    TT._close(out[0, :7], ref["qdes"], atol=err * 1e-4 + 1e-7, what=what + " qdes")
    assert not st[0].nonfinite


def test_arm_indicator(monkeypatch):
    """penalty 1e4: S on the samples whose float64 min |g| over all (t, b, o) is >= 1e-4 m (closer,
    the flag may legitimately flip): at least 95% of K, at least 10% of K on each side of the flag."""
    c = _arm_case(monkeypatch, "indicator")
    K = c["K"]
    ref = c["step"]()
    ob = ref["obs"]
    kept = ob["gabs"] >= 1e-4
    hit = ob["clr"] < 0.0
    print(f"indicator: kept {kept.sum()} of {K}; hit {np.sum(kept & hit)}, clear {np.sum(kept & ~hit)}")
    assert kept.sum() >= 0.95 * K and np.sum(kept & hit) >= 0.1 * K and np.sum(kept & ~hit) >= 0.1 * K
    e = _engine(c["spec"], **c["eng"])
    _, _, st = _run_arm(c, e)
    _close_S(e.get_costs()[0], ref, "indicator", kept)
    clr = e.get_clearances()[0]
    assert np.array_equal(clr[kept] < 0.0, hit[kept])
    _check_clr(e, 0, ref, OO.tol_c_max(c["spec"], TO.TOL_EE), "indicator")
    assert not st[0].nonfinite


def _generic_case(monkeypatch):
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
    obs = _place(OO.arm_frames(chain, qs, BASE), spec, H)
    step = lambda variant=None: OO.arm_step(monkeypatch, chain, q_full, v_full, u, noise, TO.TPOS, TO.TQUAT, spec, obs,  # noqa: E731
                                            variant=variant)
    return dict(step=step, spec=spec, obs=obs, u=u, noise=noise, K=K, H=H, chain_d=chain_d, q0=q0, qd0=qd0)


def test_generic_chain_scene_matches_oracle(monkeypatch):
    """The ten-joint generic chain (tests/pose_envelope.py): the loop form of the FK, leading, mid-chain
    and no trailing fixed joints, a prismatic joint; spheres on the fixed joint's and the prismatic
    joint's frames."""
    c = _generic_case(monkeypatch)
    step, spec, obs, u, noise, q0, qd0 = (c[k] for k in ("step", "spec", "obs", "u", "noise", "q0", "qd0"))
    ref = step()
    OO.assert_case_can_fail(step, ref, what="generic chain")
    e = _engine(spec, model="arm", n_samples=c["K"], n_horizon=c["H"], noise="injected", chain=c["chain_d"])
    e.set_target(TO.TPOS, TO.TQUAT)
    e.set_obstacles(obs.centers, obs.radii, obs.velocities)
    e.set_u_prev(u.numpy())
    _, _, st = e.step(np.concatenate([BASE, q0, qd0]), noise.numpy()[None])
    _check_clr(e, 0, ref, OO.tol_c_max(spec, TO.TOL_EE), "generic chain")
    _check_softmin(e, 0, ref, noise.numpy(), 9, "generic chain")
    assert not st[0].nonfinite


# ============================================================================ whole-body, drone, fleet
WB_VX = [0.1, -0.05, 0.05]   # (a slow base: the links do not sweep through the static obstacle for the whole horizon)


def _wb_case(monkeypatch):
    K, H = 64, 40
    chain = TT._chain()
    rpy = O.base_rpy_from_quat(TT.WB_QUAT)
    spec = OO.SceneSpec(((-1, (0.0, 0.0, 0.15), 0.20),) + ARM_BODY[1:], penalty=0.0)
    torch.manual_seed(40)
    u = torch.randn(H, 10) * 0.05
    noise = O.draw_noise(K, H, torch.from_numpy(TT.WB_SIGMA))
    s0 = torch.as_tensor(np.asarray(TT.WB_X + HOME, np.float64))
    d0 = torch.as_tensor(np.asarray(WB_VX + QD, np.float64))
    qs = O.integrate((u.unsqueeze(0) + noise).double(), s0, d0, 0.01)
    frames = OO.wholebody_frames(chain, qs, rpy.double().numpy())
    tpos = _centre(frames, (len(chain) - 1, (0.0, 0.0, 0.0), 0.0), H // 2).astype(np.float32)
    obs = _place(frames, spec, H)
    step = lambda variant=None: OO.wholebody_step(monkeypatch, chain, TT.WB_X, WB_VX, HOME, QD, rpy, u, noise,  # noqa: E731
                                                  tpos, TO.TQUAT, spec, obs, variant=variant)
    return dict(step=step, spec=spec, obs=obs, u=u, noise=noise, K=K, H=H, tpos=tpos)


def test_wholebody_scene_matches_oracle(monkeypatch):
    """H = 40: one 64-lane segment with pad lanes; the base sphere rides on p_drone(k, t)."""
    c = _wb_case(monkeypatch)
    step, spec, obs, u, noise = (c[k] for k in ("step", "spec", "obs", "u", "noise"))
    ref = step()
    OO.assert_case_can_fail(step, ref, what="wholebody")
    e = _engine(spec, model="wholebody", n_samples=c["K"], n_horizon=c["H"], noise="injected", sigma=TT.WB_SIGMA)
    e.set_target(c["tpos"], TO.TQUAT)
    e.set_obstacles(obs.centers, obs.radii, obs.velocities)
    e.set_u_prev(u.numpy())
    _, _, st = e.step(np.array(TT.WB_X + TT.WB_QUAT + HOME + WB_VX + QD, np.float64), noise.numpy()[None])
    _check_clr(e, 0, ref, OO.tol_c_max(spec, TO.TOL_EE_WB), "wholebody")
    _check_softmin(e, 0, ref, noise.numpy(), 9, "wholebody")
    assert not st[0].nonfinite


DRONE_TGT = [0.3, 0.3, 0.9]   # (near the path: a small pose cost, so the term is not lost in TOL_S |S|)


def _drone_case(monkeypatch):
    K, H = 64, 32
    spec = OO.SceneSpec(DRONE_BODY, penalty=0.0)
    torch.manual_seed(32)
    u = torch.randn(H, 3)
    noise = O.draw_noise(K, H, torch.from_numpy(TT.DRONE_SIG))
    traj = O.integrate((noise + u).double(), torch.as_tensor(np.asarray(TT.DRONE_X, np.float64)),
                       torch.as_tensor(np.asarray(TT.DRONE_V, np.float64)), 0.01)
    obs = _place(OO.drone_frames(traj), spec, H)
    step = lambda variant=None: OO.drone_step(monkeypatch, TT.DRONE_X, TT.DRONE_V, u, noise, DRONE_TGT, spec, obs, variant=variant)  # noqa: E731
    return dict(step=step, spec=spec, obs=obs, u=u, noise=noise, K=K, H=H)


def test_drone_scene_matches_oracle(monkeypatch):
    c = _drone_case(monkeypatch)
    step, spec, obs, u, noise = (c[k] for k in ("step", "spec", "obs", "u", "noise"))
    ref = step()
    # (no chain: the frame shift is not a mistake a drone kernel can make)
    OO.assert_case_can_fail(step, ref, what="drone", variants=("row_time", "no_margin", "no_offsets"))
    e = _engine(spec, model="drone", n_samples=c["K"], n_horizon=c["H"], noise="injected", sigma=TT.DRONE_SIG)
    e.set_target(DRONE_TGT)
    e.set_obstacles(obs.centers, obs.radii, obs.velocities)
    e.set_u_prev(u.numpy())
    _, _, st = e.step(np.array(TT.DRONE_X + TT.DRONE_V, np.float64), noise.numpy()[None])
    _check_clr(e, 0, ref, TO.TOL_POS * 1.3, "drone")
    _check_softmin(e, 0, ref, noise.numpy(), 5, "drone")
    assert not st[0].nonfinite


def test_fleet_an_obstacle_set_per_vehicle(monkeypatch):
    """V = 2: different sets per vehicle -- the (V, block) indexing of the staging and the kernel."""
    c = _arm_case(monkeypatch, "f64-h32")
    V = 2
    sets = [c["obs"], c["obs"].only([1, 2])]
    refs = [c["step"](None, o) for o in sets]
    assert float(np.max(np.abs(refs[0]["obs"]["S"] - refs[1]["obs"]["S"]))) > 1.0   # the two sets differ in S
    e = _engine(c["spec"], n_vehicles=V, **c["eng"])
    for v in range(V):
        _arm_target(c, e, v)
        e.set_obstacles(sets[v].centers, sets[v].radii, sets[v].velocities, vehicle=v)
    e.set_u_prev(np.tile(c["u"].numpy(), (V, 1, 1)))
    e.step(np.tile(ARM_STATE, (V, 1)), np.tile(c["noise"].numpy()[None], (V, 1, 1, 1)))
    for v in range(V):
        _close_S(e.get_costs()[v], refs[v], f"fleet vehicle {v}")
        _check_clr(e, v, refs[v], OO.tol_c_max(c["spec"], TO.TOL_EE), f"fleet vehicle {v}")


# ================================================================================== C. identities
def test_no_obstacles_far_obstacle_and_the_tracking_engine(monkeypatch):
    c = _arm_case(monkeypatch, "track")
    far = c["obs"].only([2])
    e = _engine(c["spec"], **c["eng"])
    _run_arm(c, e, OO.Obstacles.of([]))
    S_none, clr_none = e.get_costs()[0], e.get_clearances()[0]
    assert np.all(np.isposinf(clr_none)), "no obstacles: +inf clearances"
    _run_arm(c, e, far)
    S_far, clr_far = e.get_costs()[0], e.get_clearances()[0]
    assert np.array_equal(S_none.view(np.uint32), S_far.view(np.uint32)), "the 10 m obstacle adds exactly nothing"
    assert np.all(np.isfinite(clr_far)) and np.all(clr_far > 5.0)
    plain = _engine(None, **c["eng"])
    _arm_target(c, plain)
    plain.set_u_prev(c["u"].numpy())
    plain.step(ARM_STATE, c["noise"].numpy()[None])
    TT._close(S_none, plain.get_costs()[0], rtol=1e-6, what="scene engine, no obstacles vs the tracking engine")
    with pytest.raises(Exception):
        plain.set_obstacles(far.centers, far.radii)
    with pytest.raises(Exception):
        plain.get_clearances()


def test_a_new_set_between_two_calls(monkeypatch):
    c = _arm_case(monkeypatch, "f64-h32")
    e = _engine(c["spec"], **c["eng"])
    _run_arm(c, e, c["obs"].only([2]))
    S_far = e.get_costs()[0].copy()
    _run_arm(c, e)
    ref = c["step"]()
    _close_S(e.get_costs()[0], ref, "after set_obstacles")
    assert np.max(np.abs(e.get_costs()[0] - S_far)) > 1.0


@pytest.mark.parametrize("model", ["arm", "drone"])
def test_dispatch_paths_and_batches(monkeypatch, model):
    """Native and HIP dispatch give bit-equal S and clearances; after run_steps(3) both are the last
    step's (three single steps of a twin engine end on the same bits)."""
    spec = OO.SceneSpec(ARM_BODY if model == "arm" else DRONE_BODY)
    state = ARM_STATE if model == "arm" else np.array(TT.DRONE_X + TT.DRONE_V, np.float64)
    obs = OO.Obstacles.of([((-0.40, 0.30, 1.05) if model == "arm" else (0.5, 0.45, 0.9), 0.05, (0.0, 0.0, 0.0)),
                           ((-0.5, 0.0, 1.0) if model == "arm" else (0.0, 0.6, 1.2), 0.06, (0.6, 0.5, 0.0)), FAR])
    got = {}
    for mode, batch in (("hip", True), ("aql", True), ("hip", False)):
        monkeypatch.setenv("MPPI_DISPATCH", mode)
        e = _engine(spec, model=model, n_samples=256, n_horizon=32, seed=11)
        if model == "arm":
            e.set_target(TO.TPOS, TO.TQUAT)
        else:
            e.set_target([1.0, 2.0, 3.4])
        e.set_obstacles(obs.centers, obs.radii, obs.velocities)
        e.set_state(state)
        for _ in range(1 if batch else 3):
            e.run_steps(3 if batch else 1)
            e.synchronize()
        got[(mode, batch)] = (e.get_costs()[0], e.get_clearances()[0], e.dispatch_info() if hasattr(e, "dispatch_info") else "")
        e.close()
    ref = got[("hip", False)]
    assert np.isfinite(ref[1]).all() and ref[1].min() < 0.5
    for key in (("hip", True), ("aql", True)):
        assert np.array_equal(got[key][0].view(np.uint32), ref[0].view(np.uint32)), key
        assert np.array_equal(got[key][1].view(np.uint32), ref[1].view(np.uint32)), key
    print("native batch:", got[("aql", True)][2])


@pytest.mark.parametrize("name", ["f64-h32", "track"])
def test_plan_carries_the_term(monkeypatch, name):
    """get_plan of a scene engine: S, the obstacle share of cost_t, Plan.clearance against the oracle's
    zero-noise rollout; sum(cost_t) == S."""
    c = _arm_case(monkeypatch, name)
    H = c["H"]
    chain = TT._chain()
    zero = torch.zeros(1, H, 7)
    ref = OO.arm_step(monkeypatch, chain, Q_FULL, V_FULL, c["u"], zero, c["pos"], c["quat"], c["spec"], c["obs"])
    ob = ref["obs"]
    assert np.sum(ob["x"][0] > 0.0) >= H // 4, "the plan must meet the obstacles"
    e = _engine(c["spec"], **c["eng"])
    _arm_target(c, e)
    e.set_u_prev(c["u"].numpy())
    e.set_state(ARM_STATE)
    base = e.get_plan()
    assert np.all(np.isposinf(base.clearance))
    e.set_obstacles(c["obs"].centers, c["obs"].radii, c["obs"].velocities)
    plan = e.get_plan()
    S_ref = float(ref["S"][0])
    tol_S = TO.TOL_S * abs(S_ref) + ob["bound"][0]
    print(f"plan {name}: S {plan.S[0]:.4f} vs {S_ref:.4f} (tol {tol_S:.2e})")
    assert abs(float(plan.S[0]) - S_ref) <= tol_S
    TT._close(plan.cost_t[0] - base.cost_t[0], ob["x"][0], atol=tol_S, what=f"plan {name} obstacle share of cost_t")
    TT._close(plan.clearance[0], ob["clr_t"][0], atol=OO.tol_c_max(c["spec"], TO.TOL_EE), what=f"plan {name} clearance")
    assert abs(float(plan.cost_t[0].astype(np.float64).sum()) - float(plan.S[0])) <= 1e-5 * abs(float(plan.S[0]))


# ================================================================================== D. behaviour
def test_the_arm_keeps_clear_of_an_obstacle_on_its_path():
    """60 control calls (K = 1024, H = 32, device noise), each fed its own output as the next state: a
    static obstacle sits on the straight line from the hand to the target.  With the scene the executed
    path's min clearance stays >= 0; without it (the engine as it was) the arm goes through.  On the
    CPU oracle (three seeds of its own noise) the two outcomes were +0.048 .. +0.060 m and
    -0.076 .. -0.137 m: the geometry leaves several centimetres either side."""
    chain = TT._chain()
    K, H, N, sig, r_o = 1024, 32, 60, 2.0, 0.10
    spec = OO.SceneSpec(ARM_BODY, w_obs=1000.0, margin=0.10)
    hand = spec.body[-1]
    fk = lambda q: OO.arm_frames(chain, torch.as_tensor(np.asarray(q, np.float64)).view(1, 1, 7), BASE)  # noqa: E731
    fr0 = fk(HOME)
    d = np.array([-0.6, -0.3, -0.74]) / np.linalg.norm([-0.6, -0.3, -0.74])
    tpos = (fr0[7][0, 0, :3, 3].numpy() + 0.35 * d).astype(np.float32)
    tquat = TO.quat_of(fr0[7][0, 0, :3, :3].numpy()).astype(np.float32)
    obs = OO.Obstacles.of([(_centre(fr0, hand, 0) + d * (hand[2] + r_o + 0.06), r_o, (0.0, 0.0, 0.0))])
    got = {}
    for with_scene in (True, False):
        e = _engine(spec if with_scene else None, model="arm", n_samples=K, n_horizon=H, sigma=np.eye(7, dtype=np.float32) * sig,
                    seed=7)
        e.set_target(tpos, tquat)
        if with_scene:
            e.set_obstacles(obs.centers, obs.radii, obs.velocities)
        state = np.concatenate([BASE, HOME, np.zeros(7)])
        clr = []
        for _ in range(N):
            out, _, st = e.step(state)
            assert not st[0].nonfinite
            state = np.concatenate([BASE, out[0, :7], out[0, 7:14]])
            clr.append(float(OO.term(fk(out[0, :7]), spec, obs, 0.01, TO.TOL_EE)["clr"][0]))
        got[with_scene] = min(clr)
        e.close()
    print(f"executed path's min clearance: with the scene {got[True]:+.4f} m, without {got[False]:+.4f} m")
    assert got[True] >= 0.0, got
    assert got[False] < 0.0, got
