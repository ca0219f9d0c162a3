"""GPU tests of the nominal plan (mppi_get_plan, csrc/mppi_plan.hip k_plan): the zero-noise rollout
of the warm start u_prev from the engine's current state.

A. against the CPU oracle: ``oracle.mppi_oracle``'s own steps with ``noise = zeros(1, H, A)``; sample
   0's states, EE and S, and per step the pose terms (``O._pose_terms`` / the squared error of
   ``O.drone_cost``) and the lines of ``O.extra_costs`` with the same weights.
B. against the engine's own rollout of injected zero noise (no oracle).
C. semantics: the plan reads the current state and u_prev, disturbs nothing, first_reach, drop-ins.

Tolerances are the project's (test_gpu_parity.py, test_gpu_quadrotor.py):
  joint angles 2e-6, drone / whole-body positions 2e-5, EE 2e-5 (whole-body 5e-5), S 2e-5 relative,
  pos_err 6e-5 (whole-body 1.5e-4): three coordinates, each within the EE tolerance,
  cost_t 2e-5 * |S_oracle| absolute: a kernel inside the tolerance on the sum may spend it in one step.
  Quadrotor (sequential fp32 dynamics on the hardware sin/cos; test_gpu_quadrotor.py): states 5e-5,
  S 1e-4 relative, hence pos_err 1.5e-4 and cost_t 1e-4 * |S_oracle|.

A shifted step index must be visible to the cost_t check: every oracle case asserts, on the oracle's
own values, that |cost_t[t+1] - cost_t[t]| exceeds ten times the cost_t bound for at least H/2 steps
(``_assert_discriminates``; the rates below are chosen for it).  The bound is a fraction of the sum, 2e-4 * S per step,
so the longer horizons need a cost that is small in sum and steep in t: from H = 64 on the arm and
whole-body cases aim at a pose of the plan's own path (a V in t), the drone and the quadrotor fly
through their target in mid-horizon.  At H = 256 no input can meet it: the steepest shapes are the V
a |t - t0| of the pose cost, whose step a stays below 2e-4 * a * 256^2 / 4 = 3.3 a, and the drone's
quadratic a (t - t0)^2, whose largest step 256 a stays below 2e-4 * a * 256^3 / 12 = 280 a (the
fp32 scans bound the rates, too: an increment of tens of radians is off by more than the 2e-6 of
the joint angles).  There the same property is asserted for pos_err (bound 6e-5), which the kernel
stores under the same index, and cost_t has to discriminate at the terminal step alone.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import mppi_oracle as O

pytestmark = pytest.mark.gpu

TPOS, TQUAT = [0.1029, 0.4055, 1.6498], [-0.5, -0.5, 0.5, -0.5]
BASE = [0.1, -0.2, 1.1, 0.0, 0.0, 0.2588190, 0.9659258]
HOME = [1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0]
# joint rates: test_arm_horizons_match_oracle's, times a factor the longer horizons raise (the cost
# of a step must move by more than the cost_t bound, which grows with S ~ H)
RATES = np.array([0.8, -0.5, 0.3, -1.2, 0.4, 0.9, -0.7])
W = O.PoseWeights()
ALL_TERMS = O.CostTerms(enabled=("covar", "center", "jtraj", "action", "limit"))


def _engine(**kw):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    kw.setdefault("n_samples", 64)
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
    print(f"{what}: max err {err.max():.3e} (limit {np.min(lim):.3e})")
    bad = err > lim
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} off, max err {err.max():.3e} at {np.argmax(err)}"


# ------------------------------------------------------------------------------- oracle plans
def _pose_cost_t(ee, tpos, tquat, extra=None):
    """(cost_t, pos_err, the terminal step's cost, the same step under the stage weights) of one EE
    path (H,4,4): O.pose_cost's terms step by step."""
    tp, tq = torch.as_tensor(tpos, dtype=torch.float32), torch.as_tensor(tquat, dtype=torch.float32)
    cp, co = O._pose_terms(ee, tp, tq)
    c = (W.stage_pos * cp + W.stage_ori * co).double()
    last = float(extra[-1]) if extra is not None else 0.0
    term, as_stage = float(W.term_pos * cp[-1] + W.term_ori * co[-1]) + last, float(c[-1]) + last
    if extra is not None:
        c = c + extra
    c[-1] = term
    perr = torch.sum(torch.abs(ee[:, 0:3, 3] - tp), dim=-1)
    return c.numpy(), perr.double().numpy(), (term, as_stage)


def _extra_cost_t(terms, u, q, sigma, lam=0.1):
    """The enabled lines of O.extra_costs before their sum over t, for one sample with v = u."""
    H = u.shape[0]
    g = O._discount(terms.gamma, H)
    v = u
    c = torch.zeros(H, dtype=torch.float64)
    if "covar" in terms.enabled:
        sinv = torch.linalg.inv(sigma)
        quad = torch.matmul(u.unsqueeze(-2), sinv @ v.unsqueeze(-1)).squeeze(-1).squeeze(-1)
        c += terms.covar_weight * (lam * (1.0 - terms.alpha)) * quad
    if "center" in terms.enabled:
        c += torch.sum(torch.pow(q - torch.tensor(terms.q_center), 2), dim=1) * terms.centering_weight * g
    if "jtraj" in terms.enabled:
        c += torch.sum(torch.pow(q - torch.zeros_like(v), 2), dim=1) * terms.joint_traj_weight * g
    if "action" in terms.enabled:
        c += torch.sum(torch.pow(v, 2), dim=1) * terms.action_weight * g
    if "limit" in terms.enabled:
        lo, hi = torch.tensor(terms.q_lower), torch.tensor(terms.q_upper)
        c += ((q < lo) | (q > hi)).any(dim=1).float() * terms.limit_penalty * g
    return c


def oracle_arm(H, f64, u_prev, q_full, v_full, tpos=TPOS, tquat=TQUAT, terms=O.CostTerms(), sigma=None):
    r = O.arm_step(_chain(), q_full, v_full, u_prev, torch.zeros(1, H, 7), tpos, tquat, f64=f64, terms=terms,
                   sigma=sigma)
    q, ee = r["q_samples"][0], r["ee"][0]
    extra = None
    if terms.enabled:
        extra = _extra_cost_t(terms, u_prev, q, sigma if sigma is not None else 0.1 * torch.eye(7))
    c, perr, term = _pose_cost_t(ee, tpos, tquat, extra)
    return dict(state=q.double().numpy(), ee=ee.numpy().reshape(H, 16), S=float(r["S"][0]), cost_t=c, pos_err=perr,
                term=term)


def oracle_wholebody(H, u_prev, x, vx, q, qd, quat, tpos=TPOS, tquat=TQUAT):
    r = O.wholebody_step(_chain(), x, vx, q, qd, O.base_rpy_from_quat(quat), u_prev, torch.zeros(1, H, 10),
                         tpos, tquat)
    ee = r["ee"][0]
    c, perr, term = _pose_cost_t(ee, tpos, tquat)
    return dict(state=r["q_samples"][0].double().numpy(), ee=ee.numpy().reshape(H, 16), S=float(r["S"][0]),
                cost_t=c, pos_err=perr, term=term)


def _square_cost_t(pos, target, w_stage=100.0, w_term=20.0):
    e = pos - torch.as_tensor(target, dtype=torch.float32)
    e2 = torch.pow(e, 2).sum(dim=-1)
    c = e2 * w_stage
    c[-1] = e2[-1] * w_term
    return (c.double().numpy(), torch.sum(torch.abs(e), dim=-1).double().numpy(),
            (float(e2[-1] * w_term), float(e2[-1] * w_stage)))


def oracle_drone(H, u_prev, x, v, target):
    r = O.drone_step(x, v, u_prev, torch.zeros(1, H, 3), target)
    tr = r["traj"][0]
    c, perr, term = _square_cost_t(tr, target)
    return dict(state=tr.double().numpy(), ee=None, S=float(r["S"][0]), cost_t=c, pos_err=perr, term=term)


def oracle_quad(H, u_prev, x, v, target, literal):
    r = O.quad_step(x, v, u_prev, torch.zeros(1, H, 4), target, literal_jinv=literal)
    tr = r["traj"][0]
    c, perr, term = _square_cost_t(tr[:, :3], target)
    return dict(state=tr.double().numpy(), ee=None, S=float(r["S"][0]), cost_t=c, pos_err=perr, term=term)


def _assert_discriminates(ref, cost_rtol=2e-5, min_steps=None, what=""):
    """On the oracle's own values: adjacent steps' costs differ by more than ten times the cost_t
    bound for at least H/2 steps (else a shifted index would pass the cost_t check)."""
    c = ref["cost_t"]
    H = len(c)
    n = int(np.sum(np.abs(np.diff(c)) > 10 * cost_rtol * abs(ref["S"])))
    print(f"{what}: {n} of {H - 1} steps discriminate (need {H // 2 if min_steps is None else min_steps})")
    assert n >= (H // 2 if min_steps is None else min_steps), (what, n, H)
    return n


def _check_plan(p, v, ref, A, q_atol, ee_atol, perr_atol, S_rtol=2e-5, what=""):
    """Vehicle v of the engine's plan against one oracle plan."""
    H = len(ref["cost_t"])
    tr = p.traj[v]
    ns = ref["state"].shape[1]
    if isinstance(q_atol, tuple):   # whole-body: base positions, then joints
        _close(tr[:, :3], ref["state"][:, :3], atol=q_atol[0], what=what + " positions")
        _close(tr[:, 3:ns], ref["state"][:, 3:], atol=q_atol[1], what=what + " joints")
    else:
        _close(tr[:, :ns], ref["state"], atol=q_atol, what=what + " state")
    if ref["ee"] is not None:
        _close(tr[:, ns:], ref["ee"], atol=ee_atol, what=what + " EE")
        _close(p.ee_path[v], ref["ee"].reshape(H, 4, 4)[:, :3, 3], atol=ee_atol, what=what + " ee_path")
    else:
        assert tr.shape[1] == ns
        _close(p.ee_path[v], ref["state"][:, :3], atol=ee_atol, what=what + " ee_path")
    _close(p.S[v], ref["S"], rtol=S_rtol, what=what + " S")
    _close(p.pos_err[v], ref["pos_err"], atol=perr_atol, what=what + " pos_err")
    _close(p.cost_t[v], ref["cost_t"], atol=S_rtol * abs(ref["S"]), what=what + " cost_t")
    _close(np.sum(p.cost_t[v].astype(np.float64)), p.S[v], rtol=1e-5, what=what + " sum_t cost_t == S")
    # the terminal step carries the terminal weights (ref["term"]: that step under the terminal and
    # under the stage weights)
    _close(p.cost_t[v][H - 1], ref["term"][0], atol=S_rtol * abs(ref["S"]), what=what + " terminal cost")


def _arm_inputs(H, rate_scale, seed):
    torch.manual_seed(seed)
    u_prev = torch.randn(H, 7) * 0.3
    q_full = np.array(BASE + HOME)
    v_full = np.array([0.0] * 6 + list(RATES * rate_scale))
    return u_prev, q_full, v_full


def _arm_state(q_full, v_full):
    return np.concatenate([q_full[:7], q_full[7:], v_full[6:]])


def _pose_on_path(ee16):
    """(position, quaternion xyzw) of one EE matrix of a path: a target the plan passes through, so
    that the pose cost is V-shaped in t and small in sum (see the module docstring)."""
    T = np.asarray(ee16, np.float64).reshape(4, 4)
    R = T[:3, :3]
    w = 0.5 * np.sqrt(max(1e-12, 1.0 + R[0, 0] + R[1, 1] + R[2, 2]))
    q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (4.0 * w)
    return [float(x) for x in T[:3, 3]], [float(q[0]), float(q[1]), float(q[2]), float(w)]


# (H, fp64 state, rate factor): the longer horizons raise the rates of test_arm_horizons_match_oracle
# and, from H = 64 on, aim at the path's own mid-horizon pose (the cost_t bound grows with S)
ARM_CASES = [(16, False, 1.0), (16, True, 1.0), (32, False, 1.0), (32, True, 1.0), (64, False, 2.0), (64, True, 2.0),
             (96, True, 2.0), (256, True, 1.0)]


def arm_case(H, f64, scale, **kw):
    u_prev, q_full, v_full = _arm_inputs(H, scale, 100 + H)
    if 64 <= H < 256:
        ee = oracle_arm(H, f64, u_prev, q_full, v_full, **kw)["ee"]
        kw["tpos"], kw["tquat"] = _pose_on_path(ee[H // 2])
    ref = oracle_arm(H, f64, u_prev, q_full, v_full, **kw)
    ref["target"] = (kw.get("tpos", TPOS), kw.get("tquat", TQUAT))
    return u_prev, q_full, v_full, ref


# ------------------------------------------------------------------------- A. against the oracle
@pytest.mark.parametrize("H,f64,scale", ARM_CASES)
def test_arm_plan_matches_oracle(H, f64, scale):
    """Arm, fp32 and fp64 state, one wave (H <= 64), two (96) and four (256: the cross-chunk carry)."""
    u_prev, q_full, v_full, ref = arm_case(H, f64, scale)
    if H < 256:
        _assert_discriminates(ref, what=f"arm H={H}")
    else:   # (module docstring: no smooth cost meets H/2 at H = 256; pos_err takes the index check)
        _assert_discriminates(ref, min_steps=1, what="arm H=256 (terminal step)")
        assert np.sum(np.abs(np.diff(ref["pos_err"])) > 10 * 6e-5) >= H // 2
    e = _engine(model="arm", n_horizon=H, state_f64=f64)
    e.set_target(*ref["target"])
    e.set_u_prev(u_prev.numpy())
    e.set_state(_arm_state(q_full, v_full))
    _check_plan(e.get_plan(), 0, ref, 7, 2e-6, 2e-5, 6e-5, what=f"arm H={H} f64={f64}")


DRONE_X, DRONE_TARGET = [0.1, 0.2, 1.0], [1.0, 2.0, 3.4]


def drone_case(H):
    """The vehicle flies through the target in mid-horizon: the cost's quadratic has its vertex there,
    the shape with the largest steps relative to its sum."""
    torch.manual_seed(300 + H)
    u_prev = torch.randn(H, 3) * 0.3
    d = np.array(DRONE_TARGET) - np.array(DRONE_X)
    v = list(d / (0.01 * (H / 2)))
    return u_prev, v, oracle_drone(H, u_prev, DRONE_X, v, DRONE_TARGET)


@pytest.mark.parametrize("H", [20, 128, 256])
def test_drone_plan_matches_oracle(H):
    u_prev, v, ref = drone_case(H)
    if H < 256:
        _assert_discriminates(ref, what=f"drone H={H}")
    else:   # (module docstring: a quadratic cannot meet H/2 at H = 256; pos_err takes the index check)
        _assert_discriminates(ref, min_steps=1, what="drone H=256 (terminal step)")
        assert np.sum(np.abs(np.diff(ref["pos_err"])) > 10 * 6e-5) >= H // 2
    e = _engine(model="drone", n_horizon=H)
    e.set_target(DRONE_TARGET)
    e.set_u_prev(u_prev.numpy())
    e.set_state(np.array(DRONE_X + v, np.float64))
    _check_plan(e.get_plan(), 0, ref, 3, 2e-5, 2e-5, 6e-5, what=f"drone H={H}")


WB_Q = [0.0, 0.0, 0.1305262, 0.9914449]


def wb_inputs(H, scale, seed, x=(0.3, -0.1, 1.2), vx=(0.5, -0.4, 0.2), quat=WB_Q):
    torch.manual_seed(seed)
    u_prev = torch.randn(H, 10) * 0.3
    return u_prev, list(x), list(np.array(vx) * scale), list(HOME), list(RATES * scale), list(quat)


def wb_state(x, vx, q, qd, quat):
    return np.array(list(x) + list(quat) + list(q) + list(vx) + list(qd), np.float64)


@pytest.mark.parametrize("H,scale", [(64, 2.0), (100, 2.0)])
def test_wholebody_plan_matches_oracle(H, scale):
    u_prev, x, vx, q, qd, quat = wb_inputs(H, scale, 200 + H)
    tgt = _pose_on_path(oracle_wholebody(H, u_prev, x, vx, q, qd, quat)["ee"][H // 2])
    ref = oracle_wholebody(H, u_prev, x, vx, q, qd, quat, tpos=tgt[0], tquat=tgt[1])
    _assert_discriminates(ref, what=f"wholebody H={H}")
    e = _engine(model="wholebody", n_horizon=H)
    e.set_target(*tgt)
    e.set_u_prev(u_prev.numpy())
    e.set_state(wb_state(x, vx, q, qd, quat))
    _check_plan(e.get_plan(), 0, ref, 10, (2e-5, 2e-6), 5e-5, 1.5e-4, what=f"wholebody H={H}")


def test_wholebody_fleet_every_vehicle_its_own_plan():
    """V = 3 with three states, targets and warm starts: every vehicle matches its own oracle."""
    H, V = 64, 3
    ins = [wb_inputs(H, 2.0, 400, x=(0.3, -0.1, 1.2)), wb_inputs(H, 2.5, 401, x=(-0.4, 0.6, 0.9), vx=(-0.3, 0.2, 0.4),
                                                                  quat=[0.0, 0.0, 0.2588190, 0.9659258]),
           wb_inputs(H, 3.0, 402, x=(1.0, 0.2, 1.5), vx=(0.1, 0.6, -0.3), quat=[0.0, 0.0, 0.0, 1.0])]
    # each vehicle aims at a pose of its own path (mid-horizon, a third, two thirds of the way)
    tgts = [_pose_on_path(oracle_wholebody(H, i[0], *i[1:])["ee"][ts]) for i, ts in zip(ins, (32, 21, 42))]
    refs = [oracle_wholebody(H, i[0], *i[1:], tpos=t[0], tquat=t[1]) for i, t in zip(ins, tgts)]
    e = _engine(model="wholebody", n_horizon=H, n_vehicles=V)
    for v, t in enumerate(tgts):
        e.set_target(t[0], t[1], vehicle=v)
    e.set_u_prev(np.stack([i[0].numpy() for i in ins]))
    e.set_state(np.stack([wb_state(*i[1:]) for i in ins]))
    p = e.get_plan()
    assert p.traj.shape == (V, H, 26) and p.cost_t.shape == (V, H) and p.S.shape == (V,)
    for v in range(V):
        _assert_discriminates(refs[v], what=f"fleet vehicle {v}")
        _check_plan(p, v, refs[v], 10, (2e-5, 2e-6), 5e-5, 1.5e-4, what=f"fleet vehicle {v}")


QUAD_X, QUAD_TARGET = [0.2, -0.1, 2.5, 0.05, -0.08, 0.7], [0.5, 0.4, 3.0]


def quad_case(H, literal):
    rng = np.random.default_rng(500 + H)
    u = np.zeros((H, 4), np.float32)
    u[:, 0] = 14.7 * 9.81
    u += (rng.standard_normal((H, 4)) * 0.3).astype(np.float32)
    # through the target in mid-horizon, as the drone
    d = np.array(QUAD_TARGET) - np.array(QUAD_X[:3])
    v = list(d / (0.01 * (H / 2))) + [0.2, -0.1, 0.05]
    return u, v, oracle_quad(H, torch.from_numpy(u), QUAD_X, v, QUAD_TARGET, literal)


@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("literal", [False, True])
def test_quadrotor_plan_matches_oracle(H, literal):
    u, v, ref = quad_case(H, literal)
    _assert_discriminates(ref, cost_rtol=1e-4, what=f"quadrotor H={H}")
    e = _engine(model="quadrotor", n_horizon=H, quad={"quad_literal_jinv": literal})
    e.set_target(np.asarray(QUAD_TARGET, np.float32))
    e.set_u_prev(u)
    e.set_state(np.asarray(QUAD_X + v, np.float64))
    _check_plan(e.get_plan(), 0, ref, 4, 5e-5, 5e-5, 1.5e-4, S_rtol=1e-4, what=f"quadrotor H={H} literal={literal}")


def allcosts_case(step=0):
    g = load_golden("arm_k64_h32_allcosts.npz")
    u_prev = torch.from_numpy(g[f"s{step}_u_prev_in"])
    ref = oracle_arm(32, True, u_prev, g["q_full"], g["v_full"], g["target_pos"], g["target_quat"], terms=ALL_TERMS,
                     sigma=torch.from_numpy(g["sigma"]))
    return g, u_prev, ref


@pytest.mark.parametrize("step", [0, 1])
def test_arm_plan_every_cost_term(step):
    """cost_terms = 31 on the inputs of the all-costs fixture (state near joint 6's limit): its first
    step's warm start (zeros: the joint terms), and its second step's (nonzero: covar and action too)."""
    g, u_prev, ref = allcosts_case(step)
    _assert_discriminates(ref, what="arm allcosts")
    e = _engine(model="arm", n_horizon=32, state_f64=True, cost_terms=31, sigma=g["sigma"])
    e.set_target(g["target_pos"], g["target_quat"])
    e.set_u_prev(u_prev.numpy())
    e.set_state(np.concatenate([g["q_full"][:7], g["q_full"][7:], g["v_full"][6:]]))
    _check_plan(e.get_plan(), 0, ref, 7, 2e-6, 2e-5, 6e-5, what="arm allcosts")


def test_arm_plan_generic_chain(monkeypatch):
    """MPPI_NO_KINOVA_PATH=1: the chain product joint by joint instead of the Kinova origin table."""
    monkeypatch.setenv("MPPI_NO_KINOVA_PATH", "1")
    u_prev, q_full, v_full, ref = arm_case(32, True, 1.0)
    _assert_discriminates(ref, what="arm generic chain")
    e = _engine(model="arm", n_horizon=32, state_f64=True)
    e.set_target(TPOS, TQUAT)
    e.set_u_prev(u_prev.numpy())
    e.set_state(_arm_state(q_full, v_full))
    _check_plan(e.get_plan(), 0, ref, 7, 2e-6, 2e-5, 6e-5, what="arm generic chain")


# --------------------------------------------------------- B. against the engine's own rollout
def _rollout_vs_plan(e, state, u_prev, ns, q_atol, ee_atol, S_rtol=2e-5):
    e.set_u_prev(u_prev)
    e.set_state(state)
    p = e.get_plan()   # (before the step moves u_prev)
    e.step(state, np.zeros((e.V, e.K, e.H, e.A), np.float32))
    tr, S = e.get_trajectory(), e.get_costs()
    for v in range(e.V):
        _close(p.traj[v][:, :ns], tr[v, 0][:, :ns], atol=q_atol, what="state vs rollout")
        if tr.shape[-1] > ns:
            _close(p.traj[v][:, ns:], tr[v, 0][:, ns:], atol=ee_atol, what="EE vs rollout")
        _close(p.S[v], S[v, 0], rtol=S_rtol, what="S vs rollout")


def test_plan_is_the_samplers_zero_noise_rollout_arm():
    u_prev, q_full, v_full = _arm_inputs(32, 1.0, 132)
    e = _engine(model="arm", n_horizon=32, state_f64=True, noise="injected")
    e.set_target(TPOS, TQUAT)
    _rollout_vs_plan(e, _arm_state(q_full, v_full), u_prev.numpy(), 7, 2e-6, 2e-5)


def test_plan_is_the_samplers_zero_noise_rollout_wholebody():
    u_prev, x, vx, q, qd, quat = wb_inputs(64, 2.0, 264)
    e = _engine(model="wholebody", n_horizon=64, noise="injected")
    e.set_target(TPOS, TQUAT)
    _rollout_vs_plan(e, wb_state(x, vx, q, qd, quat), u_prev.numpy(), 10, 2e-5, 5e-5)


def test_plan_is_the_samplers_zero_noise_rollout_drone():
    u_prev, v, _ = drone_case(20)
    e = _engine(model="drone", n_horizon=20, noise="injected")
    e.set_target(DRONE_TARGET)
    _rollout_vs_plan(e, np.array(DRONE_X + v, np.float64), u_prev.numpy(), 3, 2e-5, 2e-5)


def test_plan_is_the_samplers_zero_noise_rollout_quadrotor():
    u, v, _ = quad_case(32, False)
    e = _engine(model="quadrotor", n_horizon=32, noise="injected")
    e.set_target(np.asarray(QUAD_TARGET, np.float32))
    _rollout_vs_plan(e, np.asarray(QUAD_X + v, np.float64), u, 6, 5e-5, 5e-5, S_rtol=1e-4)


# ------------------------------------------------------------------------------- C. semantics
def test_plan_reads_the_current_state_and_warm_start():
    """After a device-noise step the plan is the oracle plan of get_u_prev(); after set_state alone
    (no step) it is the plan from the new state."""
    H = 32
    _, q_full, v_full = _arm_inputs(H, 1.0, 600)
    e = _engine(model="arm", n_horizon=H, state_f64=True, seed=11)
    e.set_target(TPOS, TQUAT)
    e.step(_arm_state(q_full, v_full))
    u = torch.from_numpy(e.get_u_prev()[0].copy())
    assert float(u.abs().max()) > 0.0
    ref = oracle_arm(H, True, u, q_full, v_full)
    _check_plan(e.get_plan(), 0, ref, 7, 2e-6, 2e-5, 6e-5, what="after a step")
    q2 = q_full.copy()
    q2[7:] += np.array([0.3, -0.2, 0.1, 0.25, -0.15, 0.2, 0.05])
    v2 = v_full.copy()
    v2[6:] *= -1.5
    e.set_state(_arm_state(q2, v2))
    ref2 = oracle_arm(H, True, u, q2, v2)
    assert np.abs(ref2["state"] - ref["state"]).max() > 0.1
    _check_plan(e.get_plan(), 0, ref2, 7, 2e-6, 2e-5, 6e-5, what="after set_state")


def test_plan_leaves_the_engine_undisturbed():
    """get_plan after a native batch and after a native control call returns, and the next step's
    outputs are bit-identical to those of a twin engine that never asked for a plan."""
    H = 32
    _, q_full, v_full = _arm_inputs(H, 1.0, 700)
    state = _arm_state(q_full, v_full)
    outs = []
    for ask in (False, True):
        e = _engine(model="arm", n_samples=256, n_horizon=H, state_f64=True, seed=21)
        e.set_target(TPOS, TQUAT)
        e.set_state(state)
        e.run_steps(5)
        e.synchronize()
        if ask:
            p = e.get_plan()
            assert np.isfinite(p.traj).all() and np.isfinite(p.S).all()
        e.step(state)   # (a control call: native where the engine dispatches natively)
        if ask:
            p = e.get_plan()
            assert np.isfinite(p.traj).all() and np.isfinite(p.cost_t).all()
        out, u0, st = e.step(state)
        outs.append((out, u0, e.get_u_prev(), st[0].rho, st[0].eta))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert a.tobytes() == b.tobytes()
    assert outs[0][3:] == outs[1][3:]


def test_fresh_engine_plans_the_ballistic_path():
    """A zero warm start: q_t = q0 + (t + 1) dt qd0, before any step."""
    H = 32
    _, q_full, v_full = _arm_inputs(H, 1.0, 800)
    e = _engine(model="arm", n_horizon=H, state_f64=True)
    e.set_target(TPOS, TQUAT)
    e.set_state(_arm_state(q_full, v_full))
    p = e.get_plan()
    t = np.arange(1, H + 1)[:, None]
    _close(p.traj[0][:, :7], q_full[7:][None] + 0.01 * t * v_full[6:][None], atol=2e-6, what="ballistic q")
    ref = oracle_arm(H, True, torch.zeros(H, 7), q_full, v_full)
    _check_plan(p, 0, ref, 7, 2e-6, 2e-5, 6e-5, what="ballistic")


def test_first_reach():
    """The target moved onto the plan's own EE position at t*: reached by t*, not before the path
    comes within the tolerance, and -1 for a target off the path."""
    H, ts = 32, 20
    u_prev, q_full, v_full = _arm_inputs(H, 1.0, 900)
    e = _engine(model="arm", n_horizon=H, state_f64=True)
    e.set_target(TPOS, TQUAT)
    e.set_u_prev(u_prev.numpy())
    e.set_state(_arm_state(q_full, v_full))
    p = e.get_plan()
    assert p.first_reach(0.005)[0] == -1   # the home pose is nowhere near the default target
    e.set_target(p.ee_path[0, ts], TQUAT)
    p2 = e.get_plan()
    assert p2.pos_err[0, ts] < 6e-5
    fr = int(p2.first_reach(0.005)[0])
    assert 0 <= fr <= ts
    assert p2.pos_err[0, fr] < 0.005 and (p2.pos_err[0, :fr] >= 0.005).all()
    assert p2.vehicle(0).first_reach(0.005) == fr


def test_dropin_get_plan():
    """The drop-in classes return vehicle 0's plan: (H, C), (H,), (H,), scalar, (H, 3)."""
    from quadrotor_manipulator_mppi_amd.mppi_solver.mppi import MPPI
    g = load_golden("arm_k100_h32_f64.npz")
    m = MPPI()
    m.update_joint(g["q_full"], g["v_full"])
    m.compute_control_input()
    p = m.get_plan()
    H = 32
    assert p.traj.shape == (H, 23) and p.cost_t.shape == (H,) and p.pos_err.shape == (H,)
    assert np.ndim(p.S) == 0 and p.ee_path.shape == (H, 3)
    assert isinstance(p.first_reach(0.005), int)
    full = m._engine.get_plan()
    assert p.traj.tobytes() == full.traj[0].tobytes() and float(p.S) == float(full.S[0])
    _close(np.sum(p.cost_t.astype(np.float64)), p.S, rtol=1e-5, what="sum_t cost_t == S")
