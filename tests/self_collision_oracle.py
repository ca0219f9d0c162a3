"""The CPU oracle of the self-collision term (mppi_create_scene_self), in float64, built on
tests/obstacle_oracle.py's frames (``arm_frames``, ``wholebody_frames``) as they stand.

The term is the project's own (include/mppi_hip.h): a pair list P of unordered pairs (a, b) of the scene's
body spheres, indexed as in the scene's body; with c_b(k,t) the sphere's world centre exactly as the
obstacle term defines it and g_ab = |c_a - c_b| - r_a - r_b,

    x_self(k,t) = w_self sum_{(a,b) in P} max(0, margin_self - g_ab) + P_self [min_{(a,b)} g_ab < 0]
    S_k += sum_t x_self(k,t)   (after the obstacle term),      sclr_k = min_{t,(a,b)} g_ab.

The step functions hand (the tracking cost + the obstacle term + this term) to ``O.arm_step`` /
``O.wholebody_step`` by the cost-function swap of tests/obstacle_oracle.py, so the softmin, SavGol and
outputs downstream are the oracle's.

Tolerances (the project's own): a centre moves by at most TOL_C_b = TOL_EE (1 + |o_b|_1) (arm; TOL_EE_WB
for the whole-body model), so a pair distance by at most TOL_P_ab = TOL_C_a + TOL_C_b.  The hinge is
1-Lipschitz in the distance:
    |S_gpu - S_ref| <= TOL_S |S_ref| + w_self sum_{(t,a,b) active} TOL_P_ab   (+ the obstacle bound),
active = g_ab < margin_self + TOL_P_ab, and |sclr_gpu - sclr_ref| <= max_{(a,b)} TOL_P_ab.

Variants (``variant=``), the mistakes a case must be able to show (``assert_case_can_fail``):
"member_shift" (the second member of each pair replaced by the next sphere), "one_radius" (only r_a
subtracted), "no_margin", "no_offsets".
"""
from dataclasses import dataclass

import numpy as np
import torch

import field_oracle as FO
import obstacle_oracle as OO
import tracking_oracle as TO
from oracle import mppi_oracle as O

F64 = torch.float64
W_SELF, MARGIN_SELF, PENALTY_SELF = 100.0, 0.02, 1e4   # the project's defaults (mppi_self_collision_default)
VARIANTS = ("member_shift", "one_radius", "no_margin", "no_offsets")


@dataclass
class SelfSpec:
    """pairs: [(a, b)] indices into the scene's body; the term's own weights."""
    pairs: tuple
    w_self: float = W_SELF
    margin: float = MARGIN_SELF
    penalty: float = PENALTY_SELF


def tol_c(sphere, tol_ee):
    return tol_ee * (1.0 + float(np.abs(np.asarray(sphere[1], np.float64)).sum()))


def tol_p(scene, a, b, tol_ee):
    return tol_c(scene.body[a], tol_ee) + tol_c(scene.body[b], tol_ee)


def tol_p_max(scene, sc, tol_ee):
    return max([tol_p(scene, a, b, tol_ee) for a, b in sc.pairs] or [2.0 * tol_ee])


def centre(frames, sphere, no_offsets=False):
    """(K, H, 3) float64: the world centre of a body sphere (frame, offset, radius)."""
    f, o, _ = sphere
    off = np.zeros(3) if no_offsets else np.asarray(np.float32(o), np.float64)
    T = frames[f].double()
    return T[..., :3, :3] @ torch.as_tensor(off) + T[..., :3, 3]


def pair_distance(frames, scene, a, b):
    """(K, H) float64: |c_a - c_b|."""
    return torch.linalg.norm(centre(frames, scene.body[a]) - centre(frames, scene.body[b]), dim=-1)


def term(frames, scene, sc, tol_ee, variant=None):
    """x (K, H), S (K), sclr (K), sclr_t (K, H), bound (K): w_self sum over active (t, a, b) of TOL_P_ab,
    n_act (K), gabs (K): min |g| over all (t, a, b) -- everything float64 numpy."""
    assert variant in (None,) + VARIANTS
    any_T = frames[-1]
    K, H = any_T.shape[0], any_T.shape[1]
    n = len(scene.body)
    margin = 0.0 if variant == "no_margin" else sc.margin
    hinge = torch.zeros(K, H, dtype=F64)
    gmin = torch.full((K, H), float("inf"), dtype=F64)
    gabs = torch.full((K,), float("inf"), dtype=F64)
    bound = torch.zeros(K, dtype=F64)
    n_act = torch.zeros(K, dtype=F64)
    for a, b in sc.pairs:
        tp = tol_p(scene, a, b, tol_ee)
        if variant == "member_shift":
            b = (b + 1) % n
            if b == a:
                b = (b + 1) % n
        ca = centre(frames, scene.body[a], variant == "no_offsets")
        cb = centre(frames, scene.body[b], variant == "no_offsets")
        ra, rb = float(np.float32(scene.body[a][2])), float(np.float32(scene.body[b][2]))
        g = torch.linalg.norm(ca - cb, dim=-1) - ra - (0.0 if variant == "one_radius" else rb)
        hinge += torch.clamp(margin - g, min=0.0)
        gmin = torch.minimum(gmin, g)
        gabs = torch.minimum(gabs, g.abs().min(dim=1).values)
        act = (g < margin + tp).double()
        bound += sc.w_self * tp * act.sum(dim=1)
        n_act += act.sum(dim=1)
    x = sc.w_self * hinge + sc.penalty * (gmin < 0.0).double()
    sclr = gmin.min(dim=1).values if sc.pairs else torch.full((K,), float("inf"), dtype=F64)
    return dict(x=x.numpy(), S=x.sum(dim=1).numpy(), sclr=sclr.numpy(), sclr_t=gmin.numpy(),
                bound=bound.numpy(), n_act=n_act.numpy(), gabs=gabs.numpy())


def size_second_members(frames, scene, pairs, margin, row, frac=0.5):
    """The scene with the second member of each pair resized so that the pair's sample-mean clearance at
    ``row`` is ``frac`` of the margin (the margin is then crossed inside the horizon).  The pairs must not
    share second members."""
    body = list(scene.body)
    assert len({b for _, b in pairs}) == len(pairs)
    for a, b in pairs:
        d = float(pair_distance(frames, scene, a, b)[:, row].mean())
        r = d - float(np.float32(body[a][2])) - frac * margin
        assert r > 0.01, (a, b, d, r)
        body[b] = (body[b][0], body[b][1], float(np.float32(r)))
    return OO.SceneSpec(tuple(body), scene.w_obs, scene.margin, scene.penalty)


def _combined(ob, sf):
    """The obstacle term's dict with both terms' sums and bounds: what the S comparison of
    tests/test_gpu_obstacles.py (``_close_S``, ``_check_softmin``) takes as ref["obs"]."""
    out = dict(ob)
    for k in ("x", "S", "bound", "n_act"):
        out[k] = ob[k] + sf[k]
    out["gabs"] = np.minimum(ob["gabs"], sf["gabs"])
    return out


def arm_step(mp, chain, q_full, v_full, u_prev, noise, pos, quat, scene, obs, sc, f64=True, dt=0.01, variant=None, field=None, **kw):
    """O.arm_step with (tracking pose cost + obstacle term + self term); field: a field_oracle.Field as one
    more obstacle of the obstacle term (field_oracle.term).  Returns the oracle's dict plus "self"
    (``term``'s), "obs_only" (the obstacle term's) and "obs" (both terms' sums and bounds)."""
    H = noise.shape[1]
    pos, quat = OO._rows(pos, quat, H)
    q = torch.as_tensor(np.asarray(q_full, np.float64)[7:])
    qd = torch.as_tensor(np.asarray(v_full, np.float64)[6:])
    qs = O.integrate((u_prev.unsqueeze(0) + noise).double(), q, qd, dt)
    frames = OO.arm_frames(chain, qs, np.asarray(q_full)[:7])
    ob = OO.term(frames, scene, obs, dt, TO.TOL_EE) if field is None else FO.term(frames, scene, obs, field, dt, TO.TOL_EE)
    sf = term(frames, scene, sc, TO.TOL_EE, variant)
    add = torch.as_tensor(ob["S"] + sf["S"]).float()
    with mp.context() as m:
        m.setattr(O, "pose_cost", lambda ee, tp, tq, w=O.PoseWeights(): TO.pose_cost_tracking(ee, pos, quat, w) + add)
        ref = O.arm_step(chain, q_full, v_full, u_prev, noise, pos[0], quat[0], dt=dt, f64=f64, **kw)
    ref["self"], ref["obs_only"], ref["obs"] = sf, ob, _combined(ob, sf)
    return ref


def wholebody_step(mp, chain, x, vx, q, qd, rpy, u_prev, noise, pos, quat, scene, obs, sc, dt=0.01, variant=None, **kw):
    H = noise.shape[1]
    pos, quat = OO._rows(pos, quat, H)
    s0 = torch.as_tensor(np.asarray(list(x) + list(q), np.float64))
    d0 = torch.as_tensor(np.asarray(list(vx) + list(qd), np.float64))
    qs = O.integrate((u_prev.unsqueeze(0) + noise).double(), s0, d0, dt)
    frames = OO.wholebody_frames(chain, qs, np.asarray(rpy, np.float64))
    ob = OO.term(frames, scene, obs, dt, TO.TOL_EE_WB)
    sf = term(frames, scene, sc, TO.TOL_EE_WB, variant)
    add = torch.as_tensor(ob["S"] + sf["S"]).float()
    with mp.context() as m:
        m.setattr(O, "pose_cost", lambda ee, tp, tq, w=O.PoseWeights(): TO.pose_cost_tracking(ee, pos, quat, w) + add)
        ref = O.wholebody_step(chain, x, vx, q, qd, rpy, u_prev, noise, pos[0], quat[0], dt=dt, **kw)
    ref["self"], ref["obs_only"], ref["obs"] = sf, ob, _combined(ob, sf)
    return ref


# --------------------------------------------------------------------- a case must be able to fail
def assert_case_can_fail(step_of, ref, S_rtol=TO.TOL_S, what="", min_active=1.0 / 3.0, variants=VARIANTS):
    """On the oracle's own numbers (step_of(variant) -> a step's dict): at least ``min_active`` of the
    samples carry a nonzero self term, and each of the mistakes moves S on some sample by more than
    100 x that sample's tolerance.  Returns {variant: ratio}."""
    S = ref["S"].double().numpy()
    tol = S_rtol * np.abs(S) + ref["obs"]["bound"]
    frac = float(np.mean(ref["self"]["S"] > 0.0))
    print(f"{what}: {100 * frac:.0f}% of the samples carry a nonzero self term (need {100 * min_active:.0f}%)")
    assert frac >= min_active, (what, frac)
    out = {}
    for variant in variants:
        Sv = step_of(variant)["S"].double().numpy()
        out[variant] = ratio = float(np.max(np.abs(Sv - S) / tol))
        print(f"{what}: variant {variant}: max |dS| / tol = {ratio:.1f} (need > 100)")
        assert ratio > 100.0, (what, variant, "the mistake would pass", ratio)
    return out
