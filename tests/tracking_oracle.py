"""The CPU oracle of target tracking (MPPI_COST_TARGET_TRACK): ``oracle/mppi_oracle.py`` used as it
stands, its constant target swapped for one pose per horizon step.

A target trajectory is H rows: row t the position p*_t (3) and the quaternion q*_t (xyzw, 4) wanted
at horizon index t, the state after t + 1 integration steps.  ``O._pose_terms`` broadcasts a
(H-1, 3) position and a (H-1, 4) quaternion against (K, H-1, 4, 4) poses, so the tracking costs
are ``O.pose_cost`` / ``O.drone_cost`` with the rows for the constant, summed in their order.  The
step functions call ``O.arm_step``, ``O.wholebody_step``, ``O.drone_step`` and ``O.quad_step`` with
the cost function swapped (pytest's ``monkeypatch``) and row 0 as the fixed target, so the oracle's
``reach`` is the row-0 measure.

Also here, shared by tests/test_gpu_target_track.py: the tolerances (the project's own for the same
quantities, tests/test_gpu_parity.py and the tests/test_gpu_plan.py docstring), the rows the cases
use, and the three conditions every oracle case asserts on the oracle's own numbers before it looks
at the GPU (``assert_case_can_fail``, ``assert_plan_can_fail``).
"""
import numpy as np
import torch

from oracle import mppi_oracle as O

F32 = torch.float32

# tolerances, listed once
TOL_Q = 2e-6            # joint angles
TOL_EE = 2e-5           # EE (TOL_EE_WB whole-body)
TOL_EE_WB = 5e-5
TOL_POS = 2e-5          # drone / whole-body base positions (test_gpu_parity.py)
TOL_QUAD = 5e-5         # quadrotor states (test_gpu_quadrotor.py)
TOL_S = 2e-5            # S, relative (TOL_S_QUAD quadrotor)
TOL_S_QUAD = 1e-4
TOL_W = dict(rtol=1e-4, atol=1e-5)   # w_eps, u_prev
TOL_PERR = 6e-5         # plan pos_err (TOL_PERR_WB whole-body and quadrotor)
TOL_PERR_WB = 1.5e-4
LAM = 0.1
TPOS, TQUAT = [0.1029, 0.4055, 1.6498], [-0.5, -0.5, 0.5, -0.5]


# ------------------------------------------------------------------------------------- costs
def pose_cost_tracking(ee, tpos_h3, tquat_h4, w=O.PoseWeights()):
    """O.pose_cost with row t for the constant target: the stage terms from rows [:-1], the
    terminal from row [-1], summed in O.pose_cost's order."""
    tp, tq = torch.as_tensor(tpos_h3, dtype=F32), torch.as_tensor(tquat_h4, dtype=F32)
    cp, co = O._pose_terms(ee[:, :-1], tp[:-1], tq[:-1])
    stage = torch.sum(w.stage_pos * cp + w.stage_ori * co, dim=1)
    cp, co = O._pose_terms(ee[:, -1], tp[-1], tq[-1])
    term = w.term_pos * cp + w.term_ori * co
    S = torch.zeros(ee.shape[0])
    S += stage
    S += term
    return S


def drone_cost_tracking(traj, tpos_h3, w_stage=100.0, w_term=20.0):
    """O.drone_cost with row t for the constant target."""
    tp = torch.as_tensor(tpos_h3, dtype=F32)
    e = traj[:, :-1, :].clone()[:, :, :3] - tp[:-1]
    stage = torch.pow(e, 2).sum(dim=-1).sum(dim=-1) * w_stage
    e = traj[:, -1, :].clone()[:, :3] - tp[-1]
    term = torch.pow(e, 2).sum(dim=-1) * w_term
    S = torch.zeros(traj.shape[0])
    S += stage
    S += term
    return S


# ------------------------------------------------------------------------------------- steps
def _swap_pose(mp, pos, quat):
    mp.setattr(O, "pose_cost", lambda ee, tpos, tquat, w=O.PoseWeights(): pose_cost_tracking(ee, pos, quat, w))


def _swap_drone(mp, pos):
    mp.setattr(O, "drone_cost", lambda traj, target, w_stage=100.0, w_term=20.0:
               drone_cost_tracking(traj, pos, w_stage, w_term))


def arm_step(mp, chain, q_full, v_full, u_prev, noise, pos, quat, **kw):
    with mp.context() as m:
        _swap_pose(m, pos, quat)
        return O.arm_step(chain, q_full, v_full, u_prev, noise, pos[0], quat[0], **kw)


def wholebody_step(mp, chain, x, vx, q, qd, base_rpy, u_prev, noise, pos, quat, **kw):
    with mp.context() as m:
        _swap_pose(m, pos, quat)
        return O.wholebody_step(chain, x, vx, q, qd, base_rpy, u_prev, noise, pos[0], quat[0], **kw)


def drone_step(mp, x, v, u_prev, noise, pos, **kw):
    with mp.context() as m:
        _swap_drone(m, pos)
        return O.drone_step(x, v, u_prev, noise, pos[0], **kw)


def quad_step(mp, x, v, u_prev, noise, pos, **kw):
    with mp.context() as m:
        _swap_drone(m, pos)
        return O.quad_step(x, v, u_prev, noise, pos[0], **kw)


# -------------------------------------------------------------------------------------- rows
def quat_of(R):
    """xyzw of a rotation matrix (trace > -1)."""
    R = np.asarray(R, np.float64)
    w = 0.5 * np.sqrt(max(1e-12, 1.0 + R[0, 0] + R[1, 1] + R[2, 2]))
    q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (4.0 * w)
    return np.array([q[0], q[1], q[2], w])


def line_rows(p0, H, direction, speed=0.5, dt=0.01):
    """Position rows along a line from p0: row t = p0 + speed (t + 1) dt direction/|direction|."""
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    t = (np.arange(H) + 1.0)[:, None] * dt
    return (np.asarray(p0, np.float64)[None] + speed * t * d[None]).astype(np.float32)


def slerp_rows(q0, q1, H, frac=1.0, scaled=((3, 0.5), (7, 2.0), (-1, 0.5))):
    """Orientation rows from q0 toward q1 (xyzw; row t at frac (t + 1)/H of the arc), a few rows
    left un-normalised (scaled: rotation_conversions.py:45-75 divides by |q|^2)."""
    q0, q1 = np.asarray(q0, np.float64), np.asarray(q1, np.float64)
    q0, q1 = q0 / np.linalg.norm(q0), q1 / np.linalg.norm(q1)
    if np.dot(q0, q1) < 0.0:
        q1 = -q1
    th = np.arccos(np.clip(np.dot(q0, q1), -1.0, 1.0))
    rows = np.zeros((H, 4))
    for t in range(H):
        s = frac * (t + 1.0) / H
        rows[t] = q1 if th < 1e-9 else (np.sin((1 - s) * th) * q0 + np.sin(s * th) * q1) / np.sin(th)
    for i, f in scaled:
        rows[i] *= f
    return rows.astype(np.float32)


# --------------------------------------------------------------------- a case must be able to fail
def assert_case_can_fail(S_of, pos, quat=None, S_rtol=TOL_S, what=""):
    """On the oracle's own numbers (S_of(pos, quat) -> S (K) of the case under a table):
    1. S under the table differs from S under H copies of row 0 by more than 100 x the S tolerance
       for every sample;
    2. S under the table rolled by one row (either way) differs from S by more than 100 x the S
       tolerance for at least 90% of the samples: an off-by-one row index is visible in the sum."""
    S = S_of(pos, quat).double().numpy()
    lim = 100.0 * S_rtol * np.abs(S)
    rep = lambda a: None if a is None else np.repeat(np.asarray(a)[:1], len(a), 0)   # noqa: E731
    d0 = np.abs(S_of(rep(pos), rep(quat)).double().numpy() - S)
    print(f"{what}: table vs H copies of row 0: min |dS|/S {np.min(d0 / np.abs(S)):.3e} (need > {100 * S_rtol:.1e})")
    assert np.all(d0 > lim), (what, "constant-target engine would pass", float(np.min(d0 / np.abs(S))))
    for sh in (1, -1):
        roll = lambda a: None if a is None else np.roll(np.asarray(a), sh, 0)   # noqa: E731
        d = np.abs(S_of(roll(pos), roll(quat)).double().numpy() - S)
        frac = float(np.mean(d > lim))
        print(f"{what}: rows rolled by {sh}: {100 * frac:.0f}% of the samples move by > {100 * S_rtol:.1e} S")
        assert frac >= 0.9, (what, "an off-by-one row would pass", sh, frac)
    return S


def assert_plan_can_fail(cost_t, cost_t_rolled, S, S_rtol=TOL_S, what=""):
    """3. |cost_t(table) - cost_t(rolled table)| exceeds 10 x the cost_t bound on at least H/2 steps."""
    H = len(cost_t)
    n = int(np.sum(np.abs(np.asarray(cost_t) - np.asarray(cost_t_rolled)) > 10.0 * S_rtol * abs(S)))
    print(f"{what}: {n} of {H} steps tell the table from the rolled one (need {H // 2})")
    assert n >= H // 2, (what, n, H)
