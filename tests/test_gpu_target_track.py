"""GPU tests of target tracking (MPPI_COST_TARGET_TRACK, mppi_set_target_trajectory): one pose target
per horizon step in the rollout kernels (k_rollout_tt, k_rollout_quad_tt), the plan kernel, the
C-ABI, the engine, the shards and the drop-in classes.

A. against the CPU oracle (tests/tracking_oracle.py: ``oracle/mppi_oracle.py`` as it stands with the
   row for its constant target), on injected noise, two consecutive steps with two tables.
B. semantics with no oracle: the clear table, NULL orientation, the dispatch paths, plan, shards,
   elites, drop-ins.

Tolerances are the project's own for the same quantities (tracking_oracle.py lists them once).  The
top-2 cost gap of every step is printed; below 10 lambda the weights, w_eps and u_prev are compared
as tests/test_gpu_parity.py:104-124 does: the reduction given the GPU's own S, and end to end within
the softmin's conditioning bound.

A case must be able to fail: before it looks at the GPU, every oracle case asserts on the oracle's
own numbers that the table differs from H copies of row 0 and from itself rolled by one row by more
than 100 x the S tolerance (tracking_oracle.assert_case_can_fail), the plan cases that cost_t tells
the table from the rolled one on H/2 steps (assert_plan_can_fail).
"""
import numpy as np
import pytest
import torch

import tracking_oracle as TO
from oracle import mppi_oracle as O

pytestmark = pytest.mark.gpu

BASE = [0.1, -0.2, 1.1, 0.0, 0.0, 0.2588190, 0.9659258]
HOME = [1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0]
# joint rates (test_arm_horizons_match_oracle's): the EE moves along the horizon, so which row meets
# which step matters to the sum (with an EE at rest, S is the same under any permutation of the rows)
QD = [0.8, -0.5, 0.3, -1.2, 0.4, 0.9, -0.7]
# each step's table runs along the EE's (the vehicle's) own direction of motion plus this deviation
DEV = [(0.1, 0.05, -0.03), (-0.2, 0.3, 0.2)]
SPEEDS = [0.5, 0.45]


def _dir(motion, s):
    d = np.asarray(motion, np.float64)
    return d / np.linalg.norm(d) + np.asarray(DEV[s])


def _engine(**kw):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    return Engine(make_config(**kw))


def _chain():
    from quadrotor_manipulator_mppi_amd.robot.urdf_chain import load_chain
    return [O.Joint(j["name"], j["type"], j["xyz"], j["rpy"], j["axis"], j["q_index"]) for j in load_chain()]


def _close(got, want, rtol=0.0, atol=0.0, what=""):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    lim = atol + rtol * np.abs(want)
    print(f"{what}: max err {err.max():.3e}, max rel {np.max(err / (np.abs(want) + 1e-30)):.3e}")
    bad = err > lim
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} off, max err {err.max():.3e}, " \
                          f"max rel {np.max(err / (np.abs(want) + 1e-30)):.3e}"


def _amplified_bound(dS_max, w, noise, lam, floor=2e-6):
    """|d w_eps| <= (2/lam) max|dS| sum_k w_k |eps_k| (first order) + rounding (test_gpu_parity.py)."""
    return (2.0 / lam) * dS_max * np.einsum("k,kha->ha", w, np.abs(noise)) * 1.5 + floor


def _check_softmin(e, v, ref, noise, window, S_rtol, what, own=(1e-5, 1e-7), floor=2e-6):
    """S, w, w_eps raw and smoothed, u_prev of vehicle v against one oracle step.  Returns the bound
    on u0 for the outputs' tolerances."""
    noise = np.asarray(noise)
    S, S_ref = e.get_costs()[v], ref["S"].numpy()
    _close(S, S_ref, rtol=S_rtol, what=what + " S")
    srt = np.sort(S_ref.astype(np.float64))
    gap = float(srt[1] - srt[0])
    print(f"{what}: top-2 cost gap {gap:.3f} ({'plain' if gap >= 10 * TO.LAM else 'near tie'}, 10 lambda = {10 * TO.LAM})")
    raw, sm = e.get_weighted_noise()
    raw, sm, u_new = raw[v], sm[v], e.get_u_prev()[v]
    if gap >= 10 * TO.LAM:
        _close(e.get_weights()[v], ref["w"].numpy(), rtol=1e-4, atol=1e-12, what=what + " w")
        _close(raw, ref["w_eps_raw"].numpy(), what=what + " w_eps raw", **TO.TOL_W)
        _close(sm, ref["w_eps"].numpy(), what=what + " w_eps savgol", **TO.TOL_W)
        _close(u_new, ref["u_prev_out"].numpy(), what=what + " u_prev", **TO.TOL_W)
        u0_ref = ref["u_prev_out"].numpy()[0]
        return float(np.max(1e-4 * np.abs(u0_ref) + 1e-5))
    # near tie: (a) the reduction given the GPU's own costs
    w_own = O.softmin(torch.from_numpy(S), TO.LAM).numpy()
    _close(e.get_weights()[v], w_own, rtol=1e-5, atol=1e-9, what=what + " w | S_gpu")
    _close(raw, np.einsum("k,kha->ha", w_own.astype(np.float64), noise), rtol=own[0], atol=own[1],
           what=what + " w_eps | S_gpu")
    # (b) end to end within the softmin's conditioning
    dS = float(np.max(np.abs(S.astype(np.float64) - S_ref)))
    bound = _amplified_bound(dS, ref["w"].numpy().astype(np.float64), noise, TO.LAM, floor)
    assert np.all(np.abs(raw - ref["w_eps_raw"].numpy()) <= bound), what + ": w_eps beyond the conditioning bound"
    sm_bound = np.abs(O.savgol(torch.from_numpy(bound.astype(np.float32)), window, 2).numpy()) + 4 * bound.max()
    assert np.all(np.abs(sm - ref["w_eps"].numpy()) <= sm_bound), what + ": SavGol(w_eps) beyond the bound"
    _close(u_new, ref["u_prev_out"].numpy(), atol=float(sm_bound.max()) + 1e-6, what=what + " u_prev")
    return float(sm_bound.max()) + 1e-6


# ================================================================================ A. oracle
def _arm_ee0(chain, q_full, f64, ahead=0.0):
    """The EE at the state (ahead = 0) or at the joint rates' straight-line state `ahead` seconds on."""
    q = O._as_state(np.asarray(q_full)[7:] + ahead * np.asarray(QD), f64)
    base = O._as_state(np.asarray(q_full)[:7], f64)
    return O.ee_world(chain, q.view(1, 1, 7), base)[0, 0].double().numpy()


def _arm_tables(ee0, H, s, ee1=None, fracs=(1.0, 0.6)):
    """Position rows from the initial EE along its direction of motion (ee1: the EE a horizon on), the
    orientation rows slerped from its orientation toward the reference target quaternion (fracs: how
    far along the arc the last row lies; the whole-body cases stop short -- at the full arc the
    orientation term's gain cancels the position term's loss against H copies of row 0)."""
    if ee1 is None:
        ee1 = _arm_ee0(_chain(), np.array(BASE + HOME), True, ahead=0.01 * H)
    pos = TO.line_rows(ee0[:3, 3], H, _dir(ee1[:3, 3] - ee0[:3, 3], s), SPEEDS[s])
    quat = TO.slerp_rows(TO.quat_of(ee0[:3, :3]), TO.TQUAT, H, frac=fracs[s])
    return pos, quat


ARM_CASES = {
    "f64-h32": dict(K=64, H=32, f64=True),                                          # L = 32, t = lane & 31
    "f32-h20-k100": dict(K=100, H=20, f64=False),                                   # ragged H and K
    "terms": dict(K=64, H=32, f64=True, cost_terms=("center", "joint_limit"), enabled=("center", "limit")),
    "h128": dict(K=32, H=128, f64=True),                                            # NCH 2
    "h200": dict(K=32, H=200, f64=False),                                           # ragged NCH 4
    "looped": dict(K=64, H=32, f64=True, blocks_per_vehicle=1, block_threads=128),  # iters >= 2
}


@pytest.mark.parametrize("name", list(ARM_CASES))
def test_arm_tracking_matches_oracle(monkeypatch, name):
    c = dict(ARM_CASES[name])
    K, H, f64 = c.pop("K"), c.pop("H"), c.pop("f64")
    terms = O.CostTerms(enabled=c.pop("enabled", ()))
    extra = tuple(c.pop("cost_terms", ()))
    chain = _chain()
    q_full, v_full = np.array(BASE + HOME), np.array([0.0] * 6 + QD)
    state = np.concatenate([q_full[:7], q_full[7:], v_full[6:]])
    ee0 = _arm_ee0(chain, q_full, f64)
    e = _engine(model="arm", n_samples=K, n_horizon=H, noise="injected", state_f64=f64,
                cost_terms=("target_track",) + extra, **c)
    e.set_target(TO.TPOS, TO.TQUAT)
    torch.manual_seed(len(name) + H)
    u = torch.randn(H, 7) * 0.05
    for s in range(2):
        what = f"arm {name} step {s}"
        pos, quat = _arm_tables(ee0, H, s)
        noise = O.draw_noise(K, H, torch.eye(7) * 0.1)
        step = lambda p, q: TO.arm_step(monkeypatch, chain, q_full, v_full, u, noise, p, q, f64=f64, terms=terms)  # noqa: E731
        TO.assert_case_can_fail(lambda p, q: step(p, q)["S"], pos, quat, what=what)
        ref = step(pos, quat)
        e.set_target_trajectory(pos, quat)
        e.set_u_prev(u.numpy())
        out, u0, st = e.step(state, noise.numpy()[None])
        tr = e.get_trajectory()[0]
        _close(tr[..., :7], ref["q_samples"].numpy(), atol=TO.TOL_Q, what=what + " q_samples")
        _close(tr[..., 7:], ref["ee"].numpy().reshape(K, H, 16), atol=TO.TOL_EE, what=what + " EE")
        u0_tol = _check_softmin(e, 0, ref, noise.numpy(), 9, TO.TOL_S, what)
        u0_ref = ref["u_prev_out"].numpy()[0]
        _close(u0[0], u0_ref, atol=u0_tol, what=what + " u0")
        err = float(np.abs(u0[0] - u0_ref).max()) + 1e-7
        _close(out[0, 7:], ref["vdes"], atol=err * 0.01 + 1e-7, what=what + " vdes")
        _close(out[0, :7], ref["qdes"], atol=err * 1e-4 + 1e-7, what=what + " qdes")
        print(f"{what}: reach {bool(st[0].reach)} (oracle, against row 0: {ref['reach']})")
        assert bool(st[0].reach) == ref["reach"], what + ": check_reach measures against row 0"
        assert not st[0].nonfinite
        u = ref["u_prev_out"]


def test_arm_reach_is_measured_against_row_zero(monkeypatch):
    """Row 0 on the EE one step ahead and the fixed target far away: reach, as the oracle's; the same
    rows pushed one step down the table: no reach."""
    chain = _chain()
    K, H = 64, 32
    q_full, v_full = np.array(BASE + HOME), np.array([0.0] * 6 + QD)
    state = np.concatenate([q_full[:7], q_full[7:], v_full[6:]])
    ee0 = _arm_ee0(chain, q_full, True)
    torch.manual_seed(3)
    noise = O.draw_noise(K, H, torch.eye(7) * 0.1)
    u = torch.zeros(H, 7)
    quat = np.tile(np.asarray(TO.TQUAT, np.float32), (H, 1))
    pos = TO.line_rows(ee0[:3, 3], H, (1.0, 0.5, -0.3), 0.5)
    pos[0] = ee0[:3, 3] + np.array([2e-4, -1e-4, 1e-4])
    e = _engine(model="arm", n_samples=K, n_horizon=H, noise="injected", cost_terms=("target_track",))
    e.set_target(TO.TPOS, TO.TQUAT)
    for rows, want in ((pos, True), (np.roll(pos, 1, 0), False)):
        ref = TO.arm_step(monkeypatch, chain, q_full, v_full, u, noise, rows, quat)
        assert ref["reach"] == want
        e.set_target_trajectory(rows, quat)
        e.set_u_prev(u.numpy())
        _, _, st = e.step(state, noise.numpy()[None])
        assert bool(st[0].reach) == want


WB_X, WB_VX, WB_QUAT = [0.3, -0.1, 1.2], [0.5, -0.4, 0.2], [0.0, 0.0, 0.1305262, 0.9914449]
WB_SIGMA = np.diag([1.0] * 3 + [0.1] * 7).astype(np.float32)   # (at 30 on the base some sample meets condition 1 by chance)


def _wb_ee0(chain, rpy, ahead=0.0):
    x = torch.tensor(WB_X) + ahead * torch.tensor(WB_VX)
    q = torch.tensor(HOME) + ahead * torch.tensor(QD)
    qfull = torch.cat([x, rpy, q]).view(1, 1, 13)
    return O.chain_fk(chain, qfull, mobile_dof=6)[0, 0].double().numpy()


def test_wholebody_tracking_matches_oracle(monkeypatch):
    """L = 64."""
    K, H = 64, 64
    chain = _chain()
    rpy = O.base_rpy_from_quat(WB_QUAT)
    ee0, ee1 = _wb_ee0(chain, rpy), _wb_ee0(chain, rpy, ahead=0.01 * H)
    state = np.array(WB_X + WB_QUAT + HOME + WB_VX + QD, np.float64)
    e = _engine(model="wholebody", n_samples=K, n_horizon=H, noise="injected", sigma=WB_SIGMA,
                cost_terms=("target_track",))
    e.set_target(TO.TPOS, TO.TQUAT)
    torch.manual_seed(64)
    u = torch.randn(H, 10) * 0.05
    for s in range(2):
        what = f"wholebody step {s}"
        pos, quat = _arm_tables(ee0, H, s, ee1, fracs=(0.5, 0.3))
        noise = O.draw_noise(K, H, torch.from_numpy(WB_SIGMA))
        step = lambda p, q: TO.wholebody_step(monkeypatch, chain, WB_X, WB_VX, HOME, QD, rpy, u, noise, p, q)  # noqa: E731
        TO.assert_case_can_fail(lambda p, q: step(p, q)["S"], pos, quat, what=what)
        ref = step(pos, quat)
        e.set_target_trajectory(pos, quat)
        e.set_u_prev(u.numpy())
        out, u0, st = e.step(state, noise.numpy()[None])
        tr = e.get_trajectory()[0]
        _close(tr[..., :10], ref["q_samples"].numpy(), atol=TO.TOL_POS, what=what + " positions")
        _close(tr[..., 10:], ref["ee"].numpy().reshape(K, H, 16), atol=TO.TOL_EE_WB, what=what + " EE")
        u0_tol = _check_softmin(e, 0, ref, noise.numpy(), 9, TO.TOL_S, what)
        u0_ref = ref["u_prev_out"].numpy()[0]
        _close(u0[0], u0_ref, atol=u0_tol, what=what + " u0")
        err = float(np.abs(u0[0] - u0_ref).max()) + 1e-7
        _close(out[0, :3], ref["x_out"].numpy(), atol=err * 1e-4 + 1e-6, what=what + " x")
        _close(out[0, 3:6], ref["v_out"].numpy(), atol=err * 0.01 + 1e-6, what=what + " v")
        _close(out[0, 6:13], ref["qdes"].numpy(), atol=err * 1e-4 + 1e-6, what=what + " qdes")
        _close(out[0, 13:20], ref["vdes"].numpy(), atol=err * 0.01 + 1e-6, what=what + " vdes")
        assert not st[0].nonfinite
        u = ref["u_prev_out"]


DRONE_X, DRONE_V = [0.1, 0.2, 1.0], [0.5, 0.3, -0.2]
# (at the class's 30 I the samples scatter so far that fewer than 90% of them tell a rolled table)
DRONE_SIG = (np.eye(3) * 3.0).astype(np.float32)


@pytest.mark.parametrize("H", [32, 20])
def test_drone_tracking_matches_oracle(monkeypatch, H):
    """The drone branch: positions only."""
    K = 128
    e = _engine(model="drone", n_samples=K, n_horizon=H, noise="injected", sigma=DRONE_SIG, cost_terms=("target_track",))
    e.set_target([1.0, 2.0, 3.4])
    torch.manual_seed(H)
    u = torch.randn(H, 3)
    for s in range(2):
        what = f"drone H={H} step {s}"
        pos = TO.line_rows(DRONE_X, H, _dir(DRONE_V, s), SPEEDS[s])
        noise = O.draw_noise(K, H, torch.from_numpy(DRONE_SIG))
        step = lambda p, q=None: TO.drone_step(monkeypatch, DRONE_X, DRONE_V, u, noise, p)  # noqa: E731
        TO.assert_case_can_fail(lambda p, q: step(p)["S"], pos, what=what)
        ref = step(pos)
        e.set_target_trajectory(pos)
        e.set_u_prev(u.numpy())
        out, u0, st = e.step(np.array(DRONE_X + DRONE_V, np.float64), noise.numpy()[None])
        _close(e.get_trajectory()[0], ref["traj"].numpy(), atol=TO.TOL_POS, what=what + " traj")
        u0_tol = _check_softmin(e, 0, ref, noise.numpy(), 5, TO.TOL_S, what)
        u0_ref = ref["u_prev_out"].numpy()[0]
        _close(u0[0], u0_ref, atol=u0_tol, what=what + " u0")
        err = float(np.abs(u0[0] - u0_ref).max()) + 1e-7
        _close(out[0, :3], ref["x_out"].numpy(), atol=err * 1e-4 + 1e-6, what=what + " x")
        _close(out[0, 3:], ref["v_out"].numpy(), atol=err * 0.01 + 1e-6, what=what + " v")
        assert not st[0].nonfinite
        u = ref["u_prev_out"]


QUAD_X, QUAD_V = [0.2, -0.1, 2.5, 0.05, -0.08, 0.7], [0.5, -0.3, 0.2, 0.2, -0.1, 0.05]
QUAD_SIG = np.diag([30.0, 1.0, 1.0, 1.0]).astype(np.float32)
# the rows run at the vehicle's own speed: the cost is then small in sum, and a row off by one shows
# at the quadrotor's 100 x 1e-4 (at 0.45 m/s the roll by -1 moved fewer than 90% of the samples)
QUAD_SPEEDS = [0.6, 0.62]


@pytest.mark.parametrize("H,literal", [(32, False), (32, True), (64, False), (64, True)])
def test_quadrotor_tracking_matches_oracle(monkeypatch, H, literal):
    """k_rollout_quad_tt: three 16-rollout blocks, both integrations of the Euler angles."""
    K = 48
    e = _engine(model="quadrotor", n_samples=K, n_horizon=H, noise="injected", sigma=QUAD_SIG,
                quad={"quad_literal_jinv": literal}, cost_terms=("target_track",))
    e.set_target(np.asarray([0.5, 0.4, 3.0], np.float32))
    rng = np.random.default_rng(H + literal)
    u = np.zeros((H, 4), np.float32)
    u[:, 0] = 14.7 * 9.81
    u += rng.normal(0, 0.5, (H, 4)).astype(np.float32)
    torch.manual_seed(H + 2 * literal)
    for s in range(2):
        what = f"quadrotor H={H} literal={literal} step {s}"
        pos = TO.line_rows(QUAD_X[:3], H, _dir(QUAD_V[:3], s), QUAD_SPEEDS[s])
        noise = O.draw_noise(K, H, torch.from_numpy(QUAD_SIG))
        ut = torch.from_numpy(u)
        step = lambda p, q=None: TO.quad_step(monkeypatch, QUAD_X, QUAD_V, ut, noise, p, literal_jinv=literal)  # noqa: E731
        TO.assert_case_can_fail(lambda p, q: step(p)["S"], pos, S_rtol=TO.TOL_S_QUAD, what=what)
        ref = step(pos)
        e.set_target_trajectory(pos)
        e.set_u_prev(u)
        out, u0, st = e.step(np.asarray(QUAD_X + QUAD_V, np.float64), noise.numpy()[None])
        _close(e.get_trajectory()[0], ref["traj"].numpy(), atol=TO.TOL_QUAD, what=what + " traj")
        _check_softmin(e, 0, ref, noise.numpy(), 5, TO.TOL_S_QUAD, what, own=(1e-5, 1e-6), floor=2e-5)
        # outputs: the first model step under the device's own u[0] (test_gpu_quadrotor.py)
        one = O.quad_rollout(torch.from_numpy(u0[0]).view(1, 1, 4), QUAD_X, QUAD_V)[0, 0].numpy()
        _close(out[0, :6], one, atol=1e-5, what=what + " x_des")
        Iinv = np.array([1 / 1.57, 1 / 3.93, 1 / 2.59])
        _close(out[0, 9:12], np.asarray(QUAD_V[3:]) + 0.01 * Iinv * u0[0, 1:], atol=1e-5, what=what + " omega_des")
        assert not st[0].nonfinite
        u = ref["u_prev_out"].numpy()


def test_arm_fleet_a_table_per_vehicle(monkeypatch):
    """V = 3: a different table per vehicle, vehicle 2 left clear (its fixed target): the
    (V, H, row) indexing and the clear state."""
    V, K, H = 3, 64, 32
    chain = _chain()
    q_full, v_full = np.array(BASE + HOME), np.array([0.0] * 6 + QD)
    state = np.tile(np.concatenate([q_full[:7], q_full[7:], v_full[6:]]), (V, 1))
    ee0 = _arm_ee0(chain, q_full, True)
    e = _engine(model="arm", n_samples=K, n_horizon=H, n_vehicles=V, noise="injected", cost_terms=("target_track",))
    tgts = [([0.3, 0.1, 1.2], TO.TQUAT), ([0.0, 0.5, 1.5], TO.TQUAT), (TO.TPOS, TO.TQUAT)]
    for v, t in enumerate(tgts):
        e.set_target(t[0], t[1], vehicle=v)
    torch.manual_seed(33)
    u = torch.randn(V, H, 7) * 0.05
    noise = torch.stack([O.draw_noise(K, H, torch.eye(7) * 0.1) for _ in range(V)])
    tables = [_arm_tables(ee0, H, 0), _arm_tables(ee0, H, 1)]
    refs = []
    for v in range(2):
        pos, quat = tables[v]
        TO.assert_case_can_fail(lambda p, q: TO.arm_step(monkeypatch, chain, q_full, v_full, u[v], noise[v], p, q)["S"],
                                pos, quat, what=f"fleet vehicle {v}")
        refs.append(TO.arm_step(monkeypatch, chain, q_full, v_full, u[v], noise[v], pos, quat))
        e.set_target_trajectory(pos, quat, vehicle=v)
    refs.append(O.arm_step(chain, q_full, v_full, u[2], noise[2], *tgts[2]))
    e.set_u_prev(u.numpy())
    out, u0, st = e.step(state, noise.numpy())
    for v in range(V):
        what = f"fleet vehicle {v}"
        tr = e.get_trajectory()[v]
        _close(tr[..., 7:], refs[v]["ee"].numpy().reshape(K, H, 16), atol=TO.TOL_EE, what=what + " EE")
        _check_softmin(e, v, refs[v], noise[v].numpy(), 9, TO.TOL_S, what)
        assert bool(st[v].reach) == refs[v]["reach"]


# ============================================================================= B. semantics
ARM_STATE = np.array([0, 0, 1, 0, 0, 0, 1] + HOME + [0.0] * 7, np.float64)


def _fixed_rows(H):
    return (np.tile(np.asarray(TO.TPOS, np.float32), (H, 1)), np.tile(np.asarray(TO.TQUAT, np.float32), (H, 1)))


def test_clear_table_is_the_fixed_target():
    """The bit set and no table == a table of H copies of the fixed target, bit for bit; both match
    an engine created without the bit at the tolerance between two of the project's own kernels
    (test_gpu_parity.py:289-290); a moving table changes S, clearing it restores the state; a NULL
    orientation is the fixed orientation on every row; mppi_set_target refills a clear table."""
    K, H = 256, 32
    torch.manual_seed(5)
    noise = O.draw_noise(K, H, torch.eye(7) * 0.1).numpy()[None]

    def run(e, u=None):
        e.set_u_prev(np.zeros((H, 7), np.float32) if u is None else u)
        out, u0, _ = e.step(ARM_STATE, noise)
        return e.get_costs()[0].copy(), e.get_u_prev()[0].copy(), out.copy(), e.get_trajectory()[0].copy()

    kw = dict(model="arm", n_samples=K, n_horizon=H, noise="injected")
    plain, a, b = _engine(**kw), _engine(cost_terms=("target_track",), **kw), _engine(cost_terms=("target_track",), **kw)
    for e in (plain, a, b):
        e.set_target(TO.TPOS, TO.TQUAT)
    b.set_target_trajectory(*_fixed_rows(H))
    rp, ra, rb = run(plain), run(a), run(b)
    for x, y, what in zip(ra, rb, ("S", "u_prev", "outputs", "trajectory")):
        assert np.array_equal(x, y), f"no table vs H copies of the fixed target: {what}"
    _close(ra[0], rp[0], rtol=1e-6, what="tracking vs fixed-target engine: S")
    _close(ra[3][..., 7:], rp[3][..., 7:], atol=1e-6, what="tracking vs fixed-target engine: EE")
    # a moving table, then cleared
    pos = TO.line_rows(TO.TPOS, H, (1.0, 0.5, -0.3), 0.5)
    b.set_target_trajectory(pos, _fixed_rows(H)[1])
    moved = run(b)
    assert not np.array_equal(moved[0], ra[0])
    # NULL orientation rows == the fixed orientation on every row
    b.set_target_trajectory(pos, None)
    assert np.array_equal(run(b)[0], moved[0]), "quat_h4 = NULL uses the fixed orientation"
    b.set_target_trajectory(None)
    for x, y, what in zip(ra, run(b), ("S", "u_prev", "outputs", "trajectory")):
        assert np.array_equal(x, y), f"cleared table: {what}"
    # a clear table follows mppi_set_target
    for e in (plain, a):
        e.set_target([0.3, 0.2, 1.4], TO.TQUAT)
    rp2, ra2 = run(plain), run(a)
    assert not np.array_equal(ra2[0], ra[0])
    _close(ra2[0], rp2[0], rtol=1e-6, what="clear table after set_target: S")
    # without the bit the call is refused
    from quadrotor_manipulator_mppi_amd._capi import ERR_STATE, ERR_INVALID_ARG, MPPIError
    with pytest.raises(MPPIError) as ei:
        plain.set_target_trajectory(pos)
    assert ei.value.status == ERR_STATE
    with pytest.raises(MPPIError) as ei:
        a.set_target_trajectory(pos, vehicle=1)
    assert ei.value.status == ERR_INVALID_ARG


def test_dispatch_paths_agree(monkeypatch):
    """mppi_run_steps(3) natively and with MPPI_DISPATCH=hip: bit-identical u_prev on a tracking engine,
    natively dispatched where an extended-kernel (XC) engine is."""
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    K, H = 1024, 32
    pos = TO.line_rows(TO.TPOS, H, (1.0, 0.5, -0.3), 0.5)
    quat = TO.slerp_rows([0.0, 0.0, 0.0, 1.0], TO.TQUAT, H)
    engines = []
    for mode, terms in (("hip", ("target_track",)), ("aql", ("target_track",)), ("auto", ("target_track",)),
                        ("auto", ("center",))):
        if mode == "auto":
            monkeypatch.delenv("MPPI_DISPATCH", raising=False)
        else:
            monkeypatch.setenv("MPPI_DISPATCH", mode)
        e = Engine(make_config("arm", n_samples=K, n_horizon=H, seed=11, cost_terms=terms, cost_weights={"w_center": 0.0}))
        e.set_target(TO.TPOS, TO.TQUAT)
        e.set_state(ARM_STATE)
        if "target_track" in terms:
            e.set_target_trajectory(pos, quat)
        e.run_steps(3)
        e.synchronize()
        engines.append(e)
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    h, a, auto, xc = engines
    assert h.dispatch_info().startswith("hip") and a.dispatch_info().startswith("aql;"), (h.dispatch_info(), a.dispatch_info())
    assert auto.dispatch_info().split(";")[0] == xc.dispatch_info().split(";")[0], (auto.dispatch_info(), xc.dispatch_info())
    assert "k_rollout_tt" in a.kernel_info() and "k_rollout_tt" in h.kernel_info(), a.kernel_info()
    np.testing.assert_array_equal(a.get_u_prev(), h.get_u_prev())
    np.testing.assert_array_equal(auto.get_u_prev(), h.get_u_prev())
    # a second table between two batches is seen by the next one on both paths
    pos2 = TO.line_rows(TO.TPOS, H, (-0.4, 1.0, 0.6), 0.45)
    for e in (h, a):
        e.set_target_trajectory(pos2, quat)
        e.run_steps(3)
        e.synchronize()
    np.testing.assert_array_equal(a.get_u_prev(), h.get_u_prev())
    for e in engines:
        e.close()


def test_control_call_sees_the_new_table(monkeypatch):
    """One-vehicle control calls (native where the engine dispatches natively): two calls with two
    tables give two different S sets, each the oracle's under that call's table and stored noise."""
    chain = _chain()
    K, H = 64, 32
    q_full, v_full = np.array(BASE + HOME), np.array([0.0] * 6 + QD)
    state = np.concatenate([q_full[:7], q_full[7:], v_full[6:]])
    ee0 = _arm_ee0(chain, q_full, True)
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    e = _engine(model="arm", n_samples=K, n_horizon=H, seed=21, store_noise=True, cost_terms=("target_track",))
    xc = _engine(model="arm", n_samples=K, n_horizon=H, seed=21, store_noise=True, cost_terms=("center",))
    e.set_target(TO.TPOS, TO.TQUAT)
    xc.set_target(TO.TPOS, TO.TQUAT)
    xc.step(state)
    Ss = []
    for s in range(2):
        pos, quat = _arm_tables(ee0, H, s)
        e.set_target_trajectory(pos, quat)
        u = torch.from_numpy(e.get_u_prev()[0].copy())
        e.step(state)
        noise = torch.from_numpy(e.get_noise()[0].copy())
        ref = TO.arm_step(monkeypatch, chain, q_full, v_full, u, noise, pos, quat)
        _close(e.get_costs()[0], ref["S"].numpy(), rtol=TO.TOL_S, what=f"control call {s} S")
        Ss.append(e.get_costs()[0].copy())
    assert not np.allclose(Ss[0], Ss[1], rtol=1e-3)
    assert e.dispatch_info().split("calls:")[1] == xc.dispatch_info().split("calls:")[1], (e.dispatch_info(), xc.dispatch_info())


def _plan_costs_pose(ee, pos, quat):
    W = O.PoseWeights()
    tp, tq = torch.as_tensor(pos, dtype=torch.float32), torch.as_tensor(quat, dtype=torch.float32)
    cp, co = O._pose_terms(ee, tp, tq)
    c = (W.stage_pos * cp + W.stage_ori * co).double()
    c[-1] = float(W.term_pos * cp[-1] + W.term_ori * co[-1])
    return c.numpy(), torch.sum(torch.abs(ee[:, 0:3, 3] - tp), dim=-1).double().numpy()


def _plan_costs_square(p, pos):
    e = p - torch.as_tensor(pos, dtype=torch.float32)
    e2 = torch.pow(e, 2).sum(dim=-1)
    c = (e2 * 100.0).double()
    c[-1] = float(e2[-1] * 20.0)
    return c.numpy(), torch.sum(torch.abs(e), dim=-1).double().numpy()


def _check_plan(p, ref_S, cost_t, perr, S_rtol, perr_atol, what):
    _close(p.S[0], ref_S, rtol=S_rtol, what=what + " S")
    _close(p.cost_t[0], cost_t, atol=S_rtol * abs(ref_S), what=what + " cost_t")
    _close(p.pos_err[0], perr, atol=perr_atol, what=what + " pos_err")


def _first_reach_moves(e, path, far):
    """A table on the plan's own path at one step only: first_reach is that step, and moves with it."""
    for t1 in (5, 9):
        rows = np.array(far, np.float32) + np.float32(0.1)   # 0.3 m (L1) off the line the plan follows
        rows[t1] = path[t1]
        e.set_target_trajectory(rows)
        assert e.get_plan().vehicle(0).first_reach(0.005) == t1


@pytest.mark.parametrize("model", ["arm", "wholebody", "drone", "quadrotor"])
def test_plan_measures_against_row_t(monkeypatch, model):
    """cost_t, pos_err and S of the plan against the oracle's zero-noise sample under the table."""
    chain = _chain()
    H = 64 if model == "wholebody" else 32
    A = dict(arm=7, wholebody=10, drone=3, quadrotor=4)[model]
    torch.manual_seed(7 + A)
    z = torch.zeros(1, H, A)
    S_rtol, perr_atol = TO.TOL_S, TO.TOL_PERR
    if model == "arm":
        q_full, v_full = np.array(BASE + HOME), np.array([0.0] * 6 + QD)
        u = torch.randn(H, A) * 0.3
        ee0 = _arm_ee0(chain, q_full, True)
        pos, quat = _arm_tables(ee0, H, 0)
        run = lambda p, q: TO.arm_step(monkeypatch, chain, q_full, v_full, u, z, p, q)  # noqa: E731
        costs = lambda r, p, q: _plan_costs_pose(r["ee"][0], p, q)  # noqa: E731
        state = np.concatenate([q_full[:7], q_full[7:], v_full[6:]])
    elif model == "wholebody":
        u = torch.randn(H, A) * 0.3
        rpy = O.base_rpy_from_quat(WB_QUAT)
        run = lambda p, q: TO.wholebody_step(monkeypatch, chain, WB_X, WB_VX, HOME, QD, rpy, u, z, p, q)  # noqa: E731
        # The cost_t bound is a fraction of the sum (2e-4 S per step at 10 x), so the table stays close
        # to the plan's own path (tests/test_gpu_plan.py docstring): the line at the EE's own speed, each
        # orientation row a twentieth of the arc from the plan's own orientation toward the target's.
        ee0, ee1 = _wb_ee0(chain, rpy), _wb_ee0(chain, rpy, ahead=0.01 * H)
        pos = TO.line_rows(ee0[:3, 3], H, _dir(ee1[:3, 3] - ee0[:3, 3], 0), float(np.linalg.norm(ee1[:3, 3] - ee0[:3, 3]) / (0.01 * H)))
        path = run(pos, np.tile(np.asarray(TO.TQUAT, np.float32), (H, 1)))["ee"][0].double().numpy()
        quat = np.stack([TO.slerp_rows(TO.quat_of(path[t, :3, :3]), TO.TQUAT, 20, scaled=())[0] for t in range(H)])
        quat[3] *= 0.5
        quat[7] *= 2.0
        costs = lambda r, p, q: _plan_costs_pose(r["ee"][0], p, q)  # noqa: E731
        state = np.array(WB_X + WB_QUAT + HOME + WB_VX + QD, np.float64)
        perr_atol = TO.TOL_PERR_WB
    elif model == "drone":
        u = torch.randn(H, A) * 0.3
        pos, quat = TO.line_rows(DRONE_X, H, _dir(DRONE_V, 0), 0.5), None
        run = lambda p, q: TO.drone_step(monkeypatch, DRONE_X, DRONE_V, u, z, p)  # noqa: E731
        costs = lambda r, p, q: _plan_costs_square(r["traj"][0], p)  # noqa: E731
        state = np.array(DRONE_X + DRONE_V, np.float64)
    else:
        un = np.zeros((H, 4), np.float32)
        un[:, 0] = 14.7 * 9.81
        u = torch.from_numpy(un)
        pos, quat = TO.line_rows(QUAD_X[:3], H, _dir(QUAD_V[:3], 0), QUAD_SPEEDS[0]), None
        run = lambda p, q: TO.quad_step(monkeypatch, QUAD_X, QUAD_V, u, z, p)  # noqa: E731
        costs = lambda r, p, q: _plan_costs_square(r["traj"][0][:, :3], p)  # noqa: E731
        state = np.asarray(QUAD_X + QUAD_V, np.float64)
        S_rtol, perr_atol = TO.TOL_S_QUAD, TO.TOL_PERR_WB
    ref = run(pos, quat)
    cost_t, perr = costs(ref, pos, quat)
    rolled = (np.roll(pos, 1, 0), None if quat is None else np.roll(quat, 1, 0))
    TO.assert_plan_can_fail(cost_t, costs(ref, *rolled)[0], float(ref["S"][0]), S_rtol, what=f"{model} plan")
    kw = dict(sigma=WB_SIGMA) if model == "wholebody" else {}
    e = _engine(model=model, n_samples=64, n_horizon=H, cost_terms=("target_track",), **kw)
    e.set_target(TO.TPOS, TO.TQUAT)
    e.set_u_prev(u.numpy())
    e.set_state(state)
    e.set_target_trajectory(pos, quat)
    p = e.get_plan()
    _check_plan(p, float(ref["S"][0]), cost_t, perr, S_rtol, perr_atol, f"{model} plan")
    _first_reach_moves(e, p.ee_path[0], pos)


def test_shards_given_the_same_table():
    """Two in-process shards of K = 32, given the same table, reproduce the K = 64 engine's u_prev
    (the existing shard test's tolerance)."""
    K, H = 32, 32
    pos = TO.line_rows(TO.TPOS, H, (1.0, 0.5, -0.3), 0.5)
    quat = TO.slerp_rows([0.0, 0.0, 0.0, 1.0], TO.TQUAT, H)
    kw = dict(model="arm", n_horizon=H, seed=5, cost_terms=("target_track",))
    full = _engine(n_samples=2 * K, **kw)
    full.set_target(TO.TPOS, TO.TQUAT)
    full.set_target_trajectory(pos, quat)
    _, u0_full, _ = full.step(ARM_STATE)
    shards = [_engine(n_samples=K, shard_rank=r, shard_count=2, **kw) for r in range(2)]
    slot = shards[0].exchange_slot_floats()
    bufs = [torch.zeros(2 * slot, device="cuda") for _ in range(2)]
    for sh, b in zip(shards, bufs):
        sh.set_target(TO.TPOS, TO.TQUAT)
        sh.set_target_trajectory(pos, quat)
        sh.set_state(ARM_STATE)
        sh.bind_exchange(b.data_ptr())
        sh.rollout()
        sh.synchronize()
    total = bufs[0] + bufs[1]
    for sh, b in zip(shards, bufs):
        b.copy_(total)
        torch.cuda.synchronize()
        sh.finalize()
    outs = [sh.read_outputs() for sh in shards]
    assert np.array_equal(outs[0][0], outs[1][0])
    _close(outs[0][1], u0_full, rtol=1e-4, atol=1e-6, what="u0 sharded vs single")
    _close(shards[0].get_u_prev(), full.get_u_prev(), rtol=1e-4, atol=1e-6, what="u_prev sharded vs single")
    # and the table changed the result
    fixed = _engine(n_samples=2 * K, **kw)
    fixed.set_target(TO.TPOS, TO.TQUAT)
    fixed.step(ARM_STATE)
    assert not np.allclose(fixed.get_u_prev(), full.get_u_prev(), rtol=1e-4, atol=1e-6)


def test_elites_compose_with_tracking():
    K, H, n = 256, 32, 12
    e = _engine(model="arm", n_samples=K, n_horizon=H, seed=9, cost_terms=("target_track",))
    e.set_target(TO.TPOS, TO.TQUAT)
    e.set_target_trajectory(TO.line_rows(TO.TPOS, H, (1.0, 0.5, -0.3), 0.5), TO.slerp_rows([0.0, 0.0, 0.0, 1.0], TO.TQUAT, H))
    e.step(ARM_STATE)
    S = e.get_costs()[0]
    el = e.get_elites(n).vehicle(0)
    want = np.argsort(S, kind="stable")[:n]
    assert np.array_equal(el.idx, want)
    assert np.array_equal(el.S, S[want])


def test_dropin_arm_tracks_a_table(monkeypatch):
    """MPPI(track_target=True) with set_target_trajectory returns the oracle's qdes and vdes for one
    tick; with track_target=False the class has the methods and they raise RuntimeError."""
    from quadrotor_manipulator_mppi_amd.mppi_solver.mppi import MPPI
    chain = _chain()
    K, H = 64, 32
    q_full, v_full = np.array(BASE + HOME), np.array([0.0] * 6 + QD)
    ee0 = _arm_ee0(chain, q_full, True)
    pos, quat = _arm_tables(ee0, H, 0)
    torch.manual_seed(77)
    noise = O.draw_noise(K, H, torch.eye(7) * 0.1)
    ref = TO.arm_step(monkeypatch, chain, q_full, v_full, torch.zeros(H, 7), noise, pos, quat)
    m = MPPI(n_samples=K, n_horizon=H, noise="injected", verbose=False, track_target=True)
    m.update_joint(q_full, v_full)
    m.set_target_trajectory(np.concatenate([pos, quat], 1))
    qdes, vdes = m.compute_control_input(noise.numpy())
    S = m.get_costs()
    _close(S, ref["S"].numpy(), rtol=TO.TOL_S, what="drop-in S")
    dS = float(np.max(np.abs(S.astype(np.float64) - ref["S"].numpy())))
    bound = _amplified_bound(dS, ref["w"].numpy().astype(np.float64), noise.numpy(), TO.LAM)
    u0_tol = float((np.abs(O.savgol(torch.from_numpy(bound.astype(np.float32)), 9, 2).numpy()) + 4 * bound.max()).max()) + 1e-6
    _close(qdes, ref["qdes"], atol=u0_tol * 1e-4 + 1e-7, what="drop-in qdes")
    _close(vdes, ref["vdes"], atol=u0_tol * 0.01 + 1e-7, what="drop-in vdes")
    assert m.check_reach() == ref["reach"]
    # cleared: the fixed target_pose again
    m.clear_target_trajectory()
    m.u_prev = torch.zeros(H, 7)
    m.compute_control_input(noise.numpy())
    fixed = O.arm_step(chain, q_full, v_full, torch.zeros(H, 7), noise, TO.TPOS, TO.TQUAT)
    _close(m.get_costs(), fixed["S"].numpy(), rtol=TO.TOL_S, what="drop-in cleared S")
    off = MPPI(n_samples=K, n_horizon=H, noise="injected", verbose=False)
    with pytest.raises(RuntimeError):
        off.set_target_trajectory(np.concatenate([pos, quat], 1))
    with pytest.raises(RuntimeError):
        off.clear_target_trajectory()


def test_dropin_drone_classes_take_positions(monkeypatch):
    from quadrotor_manipulator_mppi_amd.mppi_solver.drone_mppi import MPPI as Drone
    from quadrotor_manipulator_mppi_amd.mppi_solver.quadrotor_mppi import MPPI as Quad
    K, H = 128, 32
    torch.manual_seed(8)
    noise = O.draw_noise(K, H, torch.eye(3) * 30.0)
    pos = TO.line_rows(DRONE_X, H, _dir(DRONE_V, 0), 0.5)
    d = Drone(n_samples=K, n_timestep=H, noise="injected", track_target=True)
    d.set_state(DRONE_X, DRONE_V)
    d.set_target_trajectory(pos)
    d.compute_control_input(noise.numpy())
    ref = TO.drone_step(monkeypatch, DRONE_X, DRONE_V, torch.zeros(H, 3), noise, pos)
    _close(d.get_costs(), ref["S"].numpy(), rtol=TO.TOL_S, what="drone drop-in S")
    with pytest.raises(ValueError):
        d.set_target_trajectory(pos[:-1])
    for cls in (Drone, Quad):
        with pytest.raises(RuntimeError):
            cls(n_samples=K, n_timestep=H).set_target_trajectory(pos)
    q = Quad(n_samples=64, n_timestep=H, track_target=True)
    q.set_state(QUAD_X, QUAD_V)
    q.set_target_trajectory(TO.line_rows(QUAD_X[:3], H, _dir(QUAD_V[:3], 0), QUAD_SPEEDS[0]))
    x, v = q.compute_control_input()
    assert torch.isfinite(x).all() and torch.isfinite(v).all()
