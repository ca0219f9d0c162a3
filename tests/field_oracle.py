"""The CPU oracle of the distance-field term (mppi_create_scene_field, mppi_set_distance_field), in
float64, built on tests/obstacle_oracle.py's frames and step wrappers.

The field (include/mppi_hip.h) is a nodal grid d[iz][iy][ix] of signed distances, node (ix, iy, iz) at
origin + voxel (ix, iy, iz).  Sampling at c: u = (c - origin) / voxel clamped per axis to [0, n - 1],
i = min(floor(u), n - 2), f = u - i, trilinear over the 8 nodes.  For body sphere b at row t,
g_b,field = d(c_b(k,t)) - r_b joins the sphere obstacles' accumulators as one more obstacle:

    x_obs(k,t) = w_obs sum_{b, o in obstacles U {field}} max(0, margin - g_bo) + P [min g < 0]
    S_k += sum_t x_obs(k,t),      clr_k = min over the same set.

Tolerance, derived (not fitted to GPU output).  The trilinear interpolant's partial derivative along an
axis is a convex combination of that axis' node differences over voxel, so with
    G = sum_axis max |Delta_axis d| / voxel          (over the whole grid)
it is G-Lipschitz in |.|_inf, and so is its composition with the clamp (a projection, 1-Lipschitz in
|.|_inf).  A centre known to TOL_C_b (obstacle_oracle: TOL_EE (1 + |o_b|_1) ...) therefore gives
    |g_gpu - g_ref| <= G TOL_C_b + TOL_D.
TOL_D is the fp32 rounding of the documented operation order on the same centre.  u = (c - o) * inv:
the subtraction rounds to 2^-24 (|c| + |o|), inv = fl(1 / voxel) and the product add 2 * 2^-24 |u|,
|u| voxel <= extent after the clamp; in metres that is at most 2^-24 (|c| + |o| + 2 extent), the
fraction f = u - i is exact (Sterbenz-like: u and i share their exponent range, u < 512), so the
interpolant moves by at most G 2^-24 (|c| + |o| + 2 extent).  The seven lerps fmaf(f, b - a, a): each
rounds b - a (2^-24 * 2 max|d|) and the fma (2^-24 max|d|), three levels deep: 3 * 3 * 2^-24 max|d|.
Doubled for slack and rounded up:
    TOL_D = 2^-23 (4 G (|c|_inf + |origin|_inf + extent) + 8 max|d|),   extent = voxel (max n - 1).
An fp32 restatement in numpy of the documented order stayed at 0.033 of TOL_D and the measured
Lipschitz ratio at 0.93 of G (24 x 20 x 16, voxel 0.05, wall U sphere, 2e5 points, a quarter outside);
tests/test_capi_field_cpu.py repeats both against the library's own sampler.

S bound (obstacle_oracle's with the field's rows):
    |S_gpu - S_ref| <= TOL_S |S_ref| + w_obs sum_{active} tol,   tol = TOL_C_b (spheres), G TOL_C_b + TOL_D (field),
active = g < margin + tol; |clr_gpu - clr_ref| <= the largest tol.

Variants (``variant=``), the mistakes a case must be able to show (``assert_case_can_fail``):
"axis_order" (the grid read as (nx, ny, nz): dims are pairwise distinct and the field not symmetric),
"cell_centred" (nodes at (i + 1/2) voxel), "nearest" (no interpolation), "no_radius", "no_origin".
"""
from dataclasses import dataclass, replace

import numpy as np
import torch

import obstacle_oracle as OO
import tracking_oracle as TO
from oracle import mppi_oracle as O

VARIANTS = ("axis_order", "cell_centred", "nearest", "no_radius", "no_origin")
DIMS, VOXEL = (24, 20, 16), 0.05   # the tests' grid (nx, ny, nz)


@dataclass
class Field:
    """dims (nx, ny, nz), voxel, origin (3,), d (nz, ny, nx) -- all as the engine is given them (float32 values)."""
    dims: tuple
    voxel: float
    origin: np.ndarray
    d: np.ndarray

    def __post_init__(self):
        self.origin = np.asarray(self.origin, np.float32)
        self.d = np.ascontiguousarray(self.d, np.float32)
        assert self.d.shape == tuple(self.dims[::-1]), (self.d.shape, self.dims)

    @property
    def G(self):
        d = self.d.astype(np.float64)
        return float(sum(np.abs(np.diff(d, axis=a)).max() for a in range(3)) / float(np.float32(self.voxel)))

    @property
    def extent(self):
        return float(np.float32(self.voxel)) * (max(self.dims) - 1)

    def tol_d(self, c):
        """TOL_D at centres c (..., 3) (module docstring)."""
        cinf = np.abs(np.nan_to_num(np.asarray(c, np.float64), nan=0.0, posinf=0.0, neginf=0.0)).max(axis=-1)
        return 2.0 ** -23 * (4.0 * self.G * (cinf + float(np.abs(self.origin).max()) + self.extent)
                             + 8.0 * float(np.abs(self.d).max()))

    def nodes(self):
        ax = [float(self.origin[a]) + float(np.float32(self.voxel)) * np.arange(self.dims[a], dtype=np.float64) for a in range(3)]
        Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        return X, Y, Z


def rasterise(fn, dims, voxel, origin):
    """Field of fn(X, Y, Z) -> d on the nodes (float64 in, float32 stored)."""
    f = Field(dims, voxel, origin, np.zeros(tuple(dims[::-1]), np.float32))
    f.d = np.ascontiguousarray(fn(*f.nodes()), np.float32)
    return f


def sample(field, c, variant=None):
    """d(c) for c (..., 3) float64, float64 arithmetic on the float32-valued field."""
    assert variant in (None,) + VARIANTS
    nx, ny, nz = field.dims
    d = field.d.astype(np.float64)
    if variant == "axis_order":   # the same memory read as [ix][iy][iz]
        d = d.reshape(-1).reshape(nx, ny, nz).transpose(2, 1, 0)
    o = np.zeros(3) if variant == "no_origin" else field.origin.astype(np.float64)
    u = (np.asarray(c, np.float64) - o) / float(np.float32(field.voxel))
    if variant == "cell_centred":
        u = u - 0.5
    n = np.array([nx, ny, nz], np.float64)
    u = np.where(np.isnan(u), 0.0, u)
    u = np.minimum(np.maximum(u, 0.0), n - 1.0)
    if variant == "nearest":
        i = np.floor(u + 0.5).astype(np.int64)
        return d[i[..., 2], i[..., 1], i[..., 0]]
    i = np.minimum(np.floor(u), n - 2.0).astype(np.int64)
    f = u - i
    ix, iy, iz = i[..., 0], i[..., 1], i[..., 2]
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    lerp = lambda a, b, t: a + t * (b - a)  # noqa: E731
    x00 = lerp(d[iz, iy, ix], d[iz, iy, ix + 1], fx)
    x10 = lerp(d[iz, iy + 1, ix], d[iz, iy + 1, ix + 1], fx)
    x01 = lerp(d[iz + 1, iy, ix], d[iz + 1, iy, ix + 1], fx)
    x11 = lerp(d[iz + 1, iy + 1, ix], d[iz + 1, iy + 1, ix + 1], fx)
    return lerp(lerp(x00, x10, fy), lerp(x01, x11, fy), fz)


def centres(frames, body):
    """Body sphere (frame, offset, radius)'s centres (K, H, 3), float64 numpy, as obstacle_oracle.term forms them."""
    f, o, _ = body
    T = frames[f].double()
    off = torch.as_tensor(np.asarray(np.float32(o), np.float64))
    return (T[..., :3, :3] @ off + T[..., :3, 3]).numpy()


# -------------------------------------------------------------------------------------- term
def term(frames, scene, obs, field, dt, tol_ee, variant=None):
    """obstacle_oracle.term's dict for the sphere obstacles and the field together (field None: the
    spheres alone), plus "S_field" (K): the field's own hinge share of S, and "tol_clr": the clearance tolerance."""
    unit = replace(scene, w_obs=1.0, penalty=0.0)
    ob = OO.term(frames, unit, obs, dt, tol_ee)   # x: the spheres' hinge sum; bound: sum of active TOL_C_b
    hinge, gmin = ob["x"].copy(), ob["clr_t"].copy()
    bound, n_act, gabs = scene.w_obs * ob["bound"], ob["n_act"].copy(), ob["gabs"].copy()
    hf = np.zeros_like(hinge)
    tol_clr = OO.tol_c_max(scene, tol_ee)
    if field is not None:
        G = field.G
        for b in scene.body:
            c = centres(frames, b)
            rb = 0.0 if variant == "no_radius" else float(np.float32(b[2]))
            g = sample(field, c, variant) - rb
            tol = G * tol_ee * (1.0 + float(np.abs(np.asarray(b[1], np.float64)).sum())) + field.tol_d(c)
            hf += np.maximum(scene.margin - g, 0.0)
            gmin = np.minimum(gmin, g)
            gabs = np.minimum(gabs, np.abs(g).min(axis=1))
            act = g < scene.margin + tol
            bound += scene.w_obs * (tol * act).sum(axis=1)
            n_act += act.sum(axis=1)
            tol_clr = max(tol_clr, float(tol.max()))
    x = scene.w_obs * (hinge + hf) + scene.penalty * (gmin < 0.0)
    return dict(x=x, S=x.sum(axis=1), clr=gmin.min(axis=1), clr_t=gmin, bound=bound, n_act=n_act, gabs=gabs,
                S_field=scene.w_obs * hf.sum(axis=1), tol_clr=tol_clr)


def outside_fraction(frames, scene, field):
    """The fraction of (k, t) rows on which some body sphere's centre lies outside the grid."""
    lo = field.origin.astype(np.float64)
    hi = lo + float(np.float32(field.voxel)) * (np.asarray(field.dims, np.float64) - 1.0)
    out = None
    for b in scene.body:
        c = centres(frames, b)
        o = np.any((c < lo) | (c > hi), axis=-1)
        out = o if out is None else out | o
    return float(out.mean())


# ------------------------------------------------------------------------------------- steps
def arm_step(mp, chain, q_full, v_full, u_prev, noise, pos, quat, scene, obs, field, f64=True, dt=0.01, variant=None, **kw):
    """obstacle_oracle.arm_step with the joint term."""
    H = noise.shape[1]
    pos, quat = OO._rows(pos, quat, H)
    q = torch.as_tensor(np.asarray(q_full, np.float64)[7:])
    qd = torch.as_tensor(np.asarray(v_full, np.float64)[6:])
    qs = O.integrate((u_prev.unsqueeze(0) + noise).double(), q, qd, dt)
    ob = term(OO.arm_frames(chain, qs, np.asarray(q_full)[:7]), scene, obs, field, dt, TO.TOL_EE, variant)
    add = torch.as_tensor(ob["S"]).float()
    with mp.context() as m:
        m.setattr(O, "pose_cost", lambda ee, tp, tq, w=O.PoseWeights(): TO.pose_cost_tracking(ee, pos, quat, w) + add)
        ref = O.arm_step(chain, q_full, v_full, u_prev, noise, pos[0], quat[0], dt=dt, f64=f64, **kw)
    ref["obs"] = ob
    return ref


def wholebody_step(mp, chain, x, vx, q, qd, rpy, u_prev, noise, pos, quat, scene, obs, field, dt=0.01, variant=None, **kw):
    H = noise.shape[1]
    pos, quat = OO._rows(pos, quat, H)
    s0 = torch.as_tensor(np.asarray(list(x) + list(q), np.float64))
    d0 = torch.as_tensor(np.asarray(list(vx) + list(qd), np.float64))
    qs = O.integrate((u_prev.unsqueeze(0) + noise).double(), s0, d0, dt)
    ob = term(OO.wholebody_frames(chain, qs, np.asarray(rpy, np.float64)), scene, obs, field, dt, TO.TOL_EE_WB, variant)
    add = torch.as_tensor(ob["S"]).float()
    with mp.context() as m:
        m.setattr(O, "pose_cost", lambda ee, tp, tq, w=O.PoseWeights(): TO.pose_cost_tracking(ee, pos, quat, w) + add)
        ref = O.wholebody_step(chain, x, vx, q, qd, rpy, u_prev, noise, pos[0], quat[0], dt=dt, **kw)
    ref["obs"] = ob
    return ref


def drone_step(mp, x, v, u_prev, noise, target, scene, obs, field, dt=0.01, variant=None, **kw):
    H = noise.shape[1]
    pos = np.asarray(target, np.float32)
    pos = np.tile(pos, (H, 1)) if pos.ndim == 1 else pos
    traj = O.integrate((noise + u_prev).double(), torch.as_tensor(np.asarray(x, np.float64)),
                       torch.as_tensor(np.asarray(v, np.float64)), dt)
    ob = term(OO.drone_frames(traj), scene, obs, field, dt, TO.TOL_POS, variant)
    add = torch.as_tensor(ob["S"]).float()
    with mp.context() as m:
        m.setattr(O, "drone_cost", lambda tr, tg, w_stage=100.0, w_term=20.0:
                  TO.drone_cost_tracking(tr, pos, w_stage, w_term) + add)
        ref = O.drone_step(x, v, u_prev, noise, pos[0], dt=dt, **kw)
    ref["obs"] = ob
    return ref


# ------------------------------------------------------------------------------- placing a field
def _mean_centre(frames, b, t):
    return centres(frames, b)[:, t].mean(axis=0)


def place(frames, scene, H, dims=DIMS, voxel=VOXEL, gap=None, blob_gap=0.02, r_blob=0.10, thick=0.2, half_w=0.2,
          shift=(0.0, 0.0, 0.0), clip_last=None, tol_ee=TO.TOL_EE, s_hint=0.0):
    """The case's field on the oracle's own frames, as test_gpu_obstacles._place places spheres: a wall
    slab ahead of the last body sphere's path, its face ``gap`` (default: half the margin) beyond that
    sphere's mean surface at the horizon's end -- met near the end only -- united with a sphere blob
    standing ``blob_gap`` off the mid-chain sphere's mean end position.  The grid is centred between
    the two (``shift`` moves it; ``clip_last``: along the axis on which the last sphere's end position is
    farthest from the centre, the grid ends that far short of it, so the rows that meet the wall read clamped
    positions: the clamp case).  Where the nodes fall relative to that geometry is free:
    of the 27 sub-voxel alignments (thirds of a voxel per axis) the one is taken at which the least
    visible of the five mistakes shows best in the term alone (on the oracle; ``s_hint``: the size of S
    the term rides on, for TOL_S's share of the tolerance)."""
    gap = 0.5 * scene.margin if gap is None else gap
    last, mid = scene.body[-1], scene.body[len(scene.body) // 2]
    c_end = _mean_centre(frames, last, H - 1)
    n1 = c_end - _mean_centre(frames, last, 0)
    n1 = n1 / np.linalg.norm(n1) if np.linalg.norm(n1) > 1e-6 else np.array([0.48, 0.6, 0.64])
    p_mid = c_end + n1 * (last[2] + gap + 0.5 * thick)        # the slab's mid-plane
    c_mid = _mean_centre(frames, mid, H - 1)
    n2 = c_mid - _mean_centre(frames, mid, 0)     # ahead of the mid sphere's own path as well
    n2 = n2 / np.linalg.norm(n2) if np.linalg.norm(n2) > 1e-6 else np.array([0.0, -0.6, 0.8])
    c_blob = c_mid + n2 * (mid[2] + r_blob + blob_gap)
    span = float(np.float32(voxel)) * (np.asarray(dims, np.float64) - 1.0)
    centre = 0.5 * (c_end + c_mid) + np.asarray(shift, np.float64)
    if clip_last is not None:
        a = int(np.argmax(np.abs(c_end - centre)))
        sgn = 1.0 if c_end[a] >= centre[a] else -1.0
        centre[a] = c_end[a] - sgn * (clip_last + 0.5 * span[a])
    origin = np.float32(centre - 0.5 * span)

    # the slab is a box in the frame (e1, e2, n1), half_w wide either way: only what moves near the last
    # sphere's end position meets it, not the links that an unbounded wall would cut through
    e1 = np.cross(n1, [0.0, 0.0, 1.0] if abs(n1[2]) < 0.9 else [1.0, 0.0, 0.0])
    e1 = e1 / np.linalg.norm(e1)
    e2 = np.cross(n1, e1)
    half = np.array([half_w, half_w, 0.5 * thick])

    def sdf(X, Y, Z):
        P = np.stack([X, Y, Z], -1)
        L = P - p_mid
        q = np.abs(np.stack([L @ e1, L @ e2, L @ n1], -1)) - half
        slab = np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)
        blob = np.linalg.norm(P - c_blob, axis=-1) - r_blob
        return np.minimum(slab, blob)
    best = None
    for sub in np.ndindex(3, 3, 3):
        f = rasterise(sdf, dims, voxel, np.float32(origin + float(np.float32(voxel)) * np.asarray(sub) / 3.0))
        ref = term(frames, scene, OO.Obstacles.of([]), f, 0.01, tol_ee)
        tol = TO.TOL_S * (s_hint + ref["S"]) + ref["bound"] + 1e-12
        score = min(float(np.max(np.abs(term(frames, scene, OO.Obstacles.of([]), f, 0.01, tol_ee, v)["S"] - ref["S"]) / tol))
                    for v in VARIANTS)
        if best is None or score > best[0]:
            best = (score, f)
    return best[1]


# --------------------------------------------------------------------- a case must be able to fail
def assert_case_can_fail(step_of, ref, S_rtol=TO.TOL_S, what="", min_active=1.0 / 3.0, variants=VARIANTS):
    """On the oracle's own numbers (step_of(variant) -> a step's dict): at least ``min_active`` of the
    samples carry a nonzero field term, and each of the mistakes moves S on some sample by more than
    100 x that sample's tolerance."""
    S, ob = ref["S"].double().numpy(), ref["obs"]
    tol = S_rtol * np.abs(S) + ob["bound"]
    frac = float(np.mean(ob["S_field"] > 0.0))
    print(f"{what}: {100 * frac:.0f}% of the samples carry a nonzero field term (need {100 * min_active:.0f}%)")
    assert frac >= min_active, (what, frac)
    for variant in variants:
        Sv = step_of(variant)["S"].double().numpy()
        ratio = float(np.max(np.abs(Sv - S) / tol))
        print(f"{what}: variant {variant}: max |dS| / tol = {ratio:.1f} (need > 100)")
        assert ratio > 100.0, (what, variant, "the mistake would pass", ratio)
