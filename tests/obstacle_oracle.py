"""The CPU oracle of the obstacle term (mppi_create_scene, mppi_set_obstacles), in float64, built on
``oracle/mppi_oracle.py`` as it stands.

The term is the project's own (include/mppi_hip.h): body sphere b rides on frame f_b of the chain --
the world transform after joints 0..f_b, f = -1 the base transform alone -- at offset o_b, radius
r_b; obstacle o is a sphere (c, r, vel) standing at c + vel (t + 1) dt at horizon row t.  With
g_bo = |centre_b - centre_o| - r_b - r_o,

    x_obs(k,t) = w_obs sum_{b,o} max(0, margin - g_bo) + P [min_{b,o} g_bo < 0]
    S_k += sum_t x_obs(k,t),      clr_k = min_{t,b,o} g_bo.

The frames are prefixes of the oracle's own chain product (``O.xyzquat_matrix`` / ``O.xyzrpy_matrix``,
then ``O.origin_matrix``, ``O.revolute_local``, ``O.prismatic_local`` joint by joint) evaluated under
``O.float64_everywhere()``.  The step functions hand the term to ``O.arm_step`` / ``O.wholebody_step``
/ ``O.drone_step`` by swapping their cost function for (the tracking cost + the term), as
tests/tracking_oracle.py swaps the pose cost, so the softmin, SavGol and outputs downstream are the
oracle's.

Tolerances (the project's own, tests/tracking_oracle.py): a body-sphere centre is an EE-like point, so
TOL_C_b = TOL_EE (1 + |o_b|_1) for the arm, TOL_EE_WB likewise for the whole-body model, TOL_POS for
the drone.  The hinge is 1-Lipschitz in the centre:
    |S_gpu - S_ref| <= TOL_S |S_ref| + w_obs sum_{(t,b,o) active} TOL_C_b,
active = g_bo < margin + TOL_C_b (``bound``), and |clr_gpu - clr_ref| <= max_b TOL_C_b.

Variants (``variant=``), the mistakes a case must be able to show (``assert_case_can_fail``):
"row_time" (the obstacles at t dt instead of (t + 1) dt), "frame_shift" (every body sphere one frame
further down the chain), "no_margin", "no_offsets".
"""
from dataclasses import dataclass

import numpy as np
import torch

import tracking_oracle as TO
from oracle import mppi_oracle as O

F64 = torch.float64
W_OBS, MARGIN, PENALTY = 100.0, 0.05, 1e4   # the project's defaults (mppi_scene_default)
VARIANTS = ("row_time", "frame_shift", "no_margin", "no_offsets")


@dataclass
class SceneSpec:
    """body: [(frame, (ox, oy, oz), radius)]; the weights."""
    body: tuple
    w_obs: float = W_OBS
    margin: float = MARGIN
    penalty: float = PENALTY


@dataclass
class Obstacles:
    """centers (n, 3), radii (n,), velocities (n, 3) (zeros: static), all as the engine is given them
    (float32 values)."""
    centers: np.ndarray
    radii: np.ndarray
    velocities: np.ndarray

    @staticmethod
    def of(rows):
        """rows: [(centre, radius, velocity)]"""
        c = np.asarray([r[0] for r in rows], np.float32).reshape(-1, 3)
        rad = np.asarray([r[1] for r in rows], np.float32).reshape(-1)
        v = np.asarray([r[2] for r in rows], np.float32).reshape(-1, 3)
        return Obstacles(c, rad, v)

    def only(self, idx):
        idx = list(idx)
        return Obstacles(self.centers[idx], self.radii[idx], self.velocities[idx])


# ------------------------------------------------------------------------------------ frames
def _chain_frames(chain, q, T):
    """{-1: T, f: T after chain joints 0..f} for q (K, H, nq) float64 (inside float64_everywhere)."""
    frames = {-1: T}
    for f, j in enumerate(chain):
        qv = q[:, :, j.q_index] if j.q_index >= 0 else torch.zeros([1, 1])
        if j.type in ("revolute", "continuous"):
            T = T @ O.revolute_local(j, qv)
        elif j.type == "prismatic":
            T = T @ O.prismatic_local(j, qv)
        else:
            T = T @ O.origin_matrix(j.xyz, j.rpy)
        frames[f] = T
    return frames


def arm_frames(chain, qs, base):
    """qs (K, H, nq), base (7,) xyz + quaternion xyzw."""
    with O.float64_everywhere():
        K, H, _ = qs.shape
        T = O.xyzquat_matrix(torch.as_tensor(np.asarray(base, np.float64))).expand(K, H, 4, 4)
        return _chain_frames(chain, qs.double(), T)


def wholebody_frames(chain, qs, rpy):
    """qs (K, H, 3 + nq): the base position then the joints; rpy (3,) the fixed base attitude."""
    with O.float64_everywhere():
        K, H, _ = qs.shape
        qs = qs.double()
        q6 = torch.cat([qs[..., :3], torch.as_tensor(np.asarray(rpy, np.float64)).expand(K, H, 3)], -1)
        return _chain_frames(chain, qs[..., 3:], O.xyzrpy_matrix(q6))


def drone_frames(traj):
    """traj (K, H, 3): the spheres ride on p(k, t) in world axes."""
    with O.float64_everywhere():
        K, H, _ = traj.shape
        T = torch.eye(4).expand(K, H, 4, 4).clone()
        T[..., :3, 3] = traj.double()[..., :3]
        return {-1: T}


# -------------------------------------------------------------------------------------- term
def term(frames, scene, obs, dt, tol_ee, variant=None):
    """x (K, H), S (K), clr (K), clr_t (K, H), bound (K): w_obs sum over active (t, b, o) of TOL_C_b,
    n_act (K), gabs (K): min |g| over all (t, b, o) -- everything float64 numpy."""
    assert variant in (None,) + VARIANTS
    any_T = frames[-1]
    K, H = any_T.shape[0], any_T.shape[1]
    fmax = max(frames)
    margin = 0.0 if variant == "no_margin" else scene.margin
    tt = np.arange(H, dtype=np.float64) + (0.0 if variant == "row_time" else 1.0)
    tau = torch.as_tensor(tt * float(np.float32(dt)))   # (the kernel's fp32 dt)
    hinge = torch.zeros(K, H, dtype=F64)
    gmin = torch.full((K, H), float("inf"), dtype=F64)
    gabs = torch.full((K,), float("inf"), dtype=F64)
    bound = torch.zeros(K, dtype=F64)
    n_act = torch.zeros(K, dtype=F64)
    for f, o, rb in scene.body:
        if variant == "frame_shift":
            f = min(f + 1, fmax)
        off = np.zeros(3) if variant == "no_offsets" else np.asarray(np.float32(o), np.float64)
        tol_c = tol_ee * (1.0 + float(np.abs(np.asarray(o, np.float64)).sum()))
        T = frames[f].double()
        ctr = T[..., :3, :3] @ torch.as_tensor(off) + T[..., :3, 3]          # (K, H, 3)
        for i in range(len(obs.radii)):
            c = torch.as_tensor(obs.centers[i].astype(np.float64))
            v = torch.as_tensor(obs.velocities[i].astype(np.float64))
            oc = c.view(1, 3) + tau.view(H, 1) * v.view(1, 3)                 # (H, 3)
            g = torch.linalg.norm(ctr - oc.view(1, H, 3), dim=-1) - float(np.float32(rb)) - float(obs.radii[i])
            hinge += torch.clamp(margin - g, min=0.0)
            gmin = torch.minimum(gmin, g)
            gabs = torch.minimum(gabs, g.abs().min(dim=1).values)
            act = (g < margin + tol_c).double()
            bound += scene.w_obs * tol_c * act.sum(dim=1)
            n_act += act.sum(dim=1)
    x = scene.w_obs * hinge + scene.penalty * (gmin < 0.0).double()
    return dict(x=x.numpy(), S=x.sum(dim=1).numpy(), clr=gmin.min(dim=1).values.numpy(), clr_t=gmin.numpy(),
                bound=bound.numpy(), n_act=n_act.numpy(), gabs=gabs.numpy())


def tol_c_max(scene, tol_ee):
    return max([tol_ee * (1.0 + float(np.abs(np.asarray(o, np.float64)).sum())) for _, o, _ in scene.body] or [tol_ee])


# ------------------------------------------------------------------------------------- steps
def _rows(pos, quat, H):
    """H copies of a fixed target, or the table as it is."""
    pos, quat = np.asarray(pos, np.float32), np.asarray(quat, np.float32)
    if pos.ndim == 1:
        pos, quat = np.tile(pos, (H, 1)), np.tile(quat, (H, 1))
    return pos, quat


def arm_step(mp, chain, q_full, v_full, u_prev, noise, pos, quat, scene, obs, f64=True, dt=0.01, variant=None, **kw):
    """O.arm_step with (tracking pose cost + obstacle term); pos / quat a fixed target or (H, .) rows.
    Returns the oracle's dict plus "obs" (``term``'s)."""
    H = noise.shape[1]
    pos, quat = _rows(pos, quat, H)
    q = torch.as_tensor(np.asarray(q_full, np.float64)[7:])
    qd = torch.as_tensor(np.asarray(v_full, np.float64)[6:])
    qs = O.integrate((u_prev.unsqueeze(0) + noise).double(), q, qd, dt)
    ob = term(arm_frames(chain, qs, np.asarray(q_full)[:7]), scene, obs, dt, TO.TOL_EE, variant)
    add = torch.as_tensor(ob["S"]).float()
    with mp.context() as m:
        m.setattr(O, "pose_cost", lambda ee, tp, tq, w=O.PoseWeights(): TO.pose_cost_tracking(ee, pos, quat, w) + add)
        ref = O.arm_step(chain, q_full, v_full, u_prev, noise, pos[0], quat[0], dt=dt, f64=f64, **kw)
    ref["obs"] = ob
    return ref


def wholebody_step(mp, chain, x, vx, q, qd, rpy, u_prev, noise, pos, quat, scene, obs, dt=0.01, variant=None, **kw):
    H = noise.shape[1]
    pos, quat = _rows(pos, quat, H)
    s0 = torch.as_tensor(np.asarray(list(x) + list(q), np.float64))
    d0 = torch.as_tensor(np.asarray(list(vx) + list(qd), np.float64))
    qs = O.integrate((u_prev.unsqueeze(0) + noise).double(), s0, d0, dt)
    ob = term(wholebody_frames(chain, qs, np.asarray(rpy, np.float64)), scene, obs, dt, TO.TOL_EE_WB, variant)
    add = torch.as_tensor(ob["S"]).float()
    with mp.context() as m:
        m.setattr(O, "pose_cost", lambda ee, tp, tq, w=O.PoseWeights(): TO.pose_cost_tracking(ee, pos, quat, w) + add)
        ref = O.wholebody_step(chain, x, vx, q, qd, rpy, u_prev, noise, pos[0], quat[0], dt=dt, **kw)
    ref["obs"] = ob
    return ref


def drone_step(mp, x, v, u_prev, noise, target, scene, obs, dt=0.01, variant=None, **kw):
    H = noise.shape[1]
    pos = np.asarray(target, np.float32)
    pos = np.tile(pos, (H, 1)) if pos.ndim == 1 else pos
    traj = O.integrate((noise + u_prev).double(), torch.as_tensor(np.asarray(x, np.float64)),
                       torch.as_tensor(np.asarray(v, np.float64)), dt)
    ob = term(drone_frames(traj), scene, obs, dt, TO.TOL_POS, variant)
    add = torch.as_tensor(ob["S"]).float()
    with mp.context() as m:
        m.setattr(O, "drone_cost", lambda tr, tg, w_stage=100.0, w_term=20.0:
                  TO.drone_cost_tracking(tr, pos, w_stage, w_term) + add)
        ref = O.drone_step(x, v, u_prev, noise, pos[0], dt=dt, **kw)
    ref["obs"] = ob
    return ref


# --------------------------------------------------------------------- a case must be able to fail
def assert_case_can_fail(step_of, ref, S_rtol=TO.TOL_S, what="", min_active=1.0 / 3.0, variants=VARIANTS):
    """On the oracle's own numbers (step_of(variant) -> a step's dict): at least ``min_active`` of the
    samples carry a nonzero term, and each of the mistakes (``variants``) moves S on some sample by more than
    100 x that sample's tolerance."""
    S, ob = ref["S"].double().numpy(), ref["obs"]
    tol = S_rtol * np.abs(S) + ob["bound"]
    frac = float(np.mean(ob["S"] > 0.0))
    print(f"{what}: {100 * frac:.0f}% of the samples carry a nonzero obstacle term (need {100 * min_active:.0f}%)")
    assert frac >= min_active, (what, frac)
    for variant in variants:
        Sv = step_of(variant)["S"].double().numpy()
        ratio = float(np.max(np.abs(Sv - S) / tol))
        print(f"{what}: variant {variant}: max |dS| / tol = {ratio:.1f} (need > 100)")
        assert ratio > 100.0, (what, variant, "the mistake would pass", ratio)
