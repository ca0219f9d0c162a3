"""Float64 oracle of depth-image integration (mppi_integrate_depth, mppi_depth_integrate_host): a numpy
restatement of the definition in include/mppi_hip.h, written from that text and not from the inline
(csrc/mppi_depth.h).

The definition, restated.  A used pixel (column i, row j, value z; rows and columns 0, stride, ...) is
skipped (NaN, -inf, z < z_min), a return (z_min <= z <= z_max) or a miss (z > z_max: the ray ends at z_max
and marks nothing).  With R the rotation of the normalised quaternion,
    p_cam = ((i - cx) / fx z, (j - cy) / fy z, z),  w = R p_cam + pos,
    ue = (w - origin) / voxel,  uo = (pos - origin) / voxel,  du = ue - uo,
    n = clamp(ceil(2 max_d |du_d|), 1, 16384),  u(m) = uo + (m / n) du for 0 <= m < n;
a point is in the grid iff -0.5 <= u_d < n_d - 0.5 on all axes and its node is floor(u + 0.5).  F: the
nodes of all in-grid samples, except a return's samples in that return's own end node (carve = 0: empty);
O: the in-grid end nodes of the returns; the map becomes (map \\ F) U O.

Tolerance.  fp32 cannot be matched bit for bit where a point sits on a node boundary, so the oracle
carries a tolerance tol_u on index coordinates, derived here by counting the roundings of the fp32 chain
(eps = 2^-24, the unit roundoff; P = max |pos_d|, O = max |origin_d|, rho = z_max sqrt(1 + xn^2 + yn^2) at
the image's corner, the longest |p_cam|; all in metres):
  * xn = ((float)i - cx) inv_fx: the difference, the reciprocal and the product round once each, and
    p0 = xn z once more: each component of p_cam carries at most 4 eps of itself.
  * R's entries come from mppi_target_rotation: the squared norm (4 roundings), 2 / s, the two-product sums
    (3), the product with 2 / s and the subtraction from 1: at most 8 eps in absolute terms (|R| <= 1).
  * w_d = fmaf(R0, p0, fmaf(R1, p1, fmaf(R2, p2, pos_d))): three roundings of partial sums that are at
    most P + rho in magnitude, plus the inputs' errors sqrt(3) rho (4 + 8) eps < 21 rho eps:
        |dw| <= eps (3 (P + rho) + 21 rho)
  * (w_d - origin_d) inv_voxel: the difference, the reciprocal and the product, 3 eps of |w - origin|
    <= P + rho + O.  So, in voxels,
        tol_end = eps (3 (P + rho) + 21 rho + 3 (P + rho + O)) / voxel
    (uo's own error, 3 eps (P + O) / voxel, is inside that).
  * sample m: t = (float)m inv_n carries 2 eps of itself (t <= 1), and the fmaf rounds once:
        |du(m)| <= tol_end + 2 eps |du| + eps |u| + (the end points' errors, already counted, weighted
        by t and 1 - t)  <=  tol_end + 3 eps U,  U = 2 (P + rho + O) / voxel bounding |du| and |u|.
  tol_u = tol_end + 3 eps U.  For coordinates up to 4 m and voxel 0.05 this is 1.2e-4 voxels; nothing in
it is fitted to any implementation's output.

The sets.  integrate() returns F_certain <= F_possible and O_certain <= O_possible (boolean (nz, ny, nx)).
A sample (or an end point) is *decided* when it is further than tol_u from every node boundary and grid
face on every axis (both are the half-integers: floor(u + 0.5 - tol) == floor(u + 0.5 + tol)); otherwise
every node its perturbations reach is a candidate.  A decided in-grid sample counts towards F_certain when
it is no candidate of its ray's end node; every candidate of every sample counts towards F_possible unless
the end node is decided and equal to it.  A ray whose 2 L is within 2 tol_u of an integer has an undecided n:
the samples of both counts go to F_possible only.  End points likewise for O.
check(before, after, sets): every node of O_certain is 1, every node of F_certain \\ O_possible is 0, and no
node outside F_possible U O_possible differs from `before`.  undecided(sets) is 1 - |certain| / |possible|
for F and for O: the cap 0.02 on both is what keeps the tolerance from hiding a failure, and
tests/test_capi_depth_cpu.py asserts it for every case of CASES.

Planted mistakes: model(case, before, variant=...) is a plain float64 implementation (no tolerance) that the
rule passes with variant=None and must fail, on at least one case, with each of VARIANTS:
  x_forward         p_cam in the body convention (x forward, y left, z up) instead of the optical one
  cell_corner       floor(u) instead of the nearest node
  free_wins         all marks, then all carves (with the exclusion): other rays clear a return's end node
  quat_wxyz         the quaternion read as (w, x, y, z)
  principal_swap    cx and cy exchanged
  endpoint_cleared  one pass per ray, the end point marked and then the ray's samples carved with no
                    exclusion: a ray clears its own end node
  miss_marks        a miss marks its end point at z_max
  stride_ignored    every pixel used
"""
import itertools
from types import SimpleNamespace

import numpy as np

EPS = 2.0 ** -24
MAX_SAMPLES = 16384
CAP = 0.02
VARIANTS = ("x_forward", "cell_corner", "free_wins", "quat_wxyz", "principal_swap", "endpoint_cleared",
            "miss_marks", "stride_ignored")


# ------------------------------------------------------------------------------------------- the cases
def look_at(forward, up=(0.0, 0.0, 1.0)):
    """quat_xyzw of an optical frame (z forward, x right, y down) looking along `forward`."""
    z = np.asarray(forward, np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=1)
    w = 0.5 * np.sqrt(max(1e-12, 1.0 + R[0, 0] + R[1, 1] + R[2, 2]))
    q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    assert np.allclose(quat_R(q), R, atol=1e-9)
    return q


def quat_R(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene_image(width, height, z_wall, z_disc, z_max, kind="scene"):
    """(height, width) float32: a disc in front of a (slightly slanted) wall with a band of misses, a few
    NaN, below-gate and negative pixels; or a constant image."""
    if kind == "nan":
        return np.full((height, width), np.nan, np.float32)
    if kind == "inf":
        return np.full((height, width), np.inf, np.float32)
    if kind == "zmax":
        return np.full((height, width), np.float32(z_max), np.float32)
    if kind == "wall":
        return np.full((height, width), np.float32(z_wall), np.float32)
    jj, ii = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    d = z_wall * (1.0 + 0.08 * ii / max(1, width - 1) - 0.05 * jj / max(1, height - 1))
    r2 = ((ii - 0.45 * width) / (0.22 * width + 1e-9)) ** 2 + ((jj - 0.4 * height) / (0.3 * height + 1e-9)) ** 2
    d = np.where(r2 < 1.0, z_disc * (1.0 + 0.03 * r2), d)
    band = (jj >= int(0.7 * height)) & (jj < int(0.7 * height) + max(1, height // 8))
    d = np.where(band, np.where(ii % 2 == 0, np.inf, 1.5 * z_max), d)
    d = d.astype(np.float32)
    if width * height >= 35:
        d[0, 0] = np.nan
        d[-1, 2] = -1.0
        d[1, -1] = 1e-3     # below the gate
        d[2, 1] = -np.inf
    return d


def _case(name, dims, voxel, image, stride, pos_idx, forward, kind="scene", z_wall=1.6, z_disc=0.9, z_min=0.2, z_max=2.0,
          carve=True, fx=None, origin=(0.25, -0.5, 1.0)):
    w, h = image
    fx = float(fx if fx is not None else 0.87 * w)
    origin = np.asarray(origin, np.float64)
    pos = origin + voxel * np.asarray(pos_idx, np.float64)
    view = SimpleNamespace(width=w, height=h, fx=fx, fy=1.07 * fx, cx=0.5 * w - 0.3, cy=0.5 * h - 0.1,
                           pos=tuple(pos), quat_xyzw=tuple(1.25 * look_at(forward)), z_min=z_min, z_max=z_max,
                           stride=stride, carve=carve)
    field = SimpleNamespace(dims=tuple(dims), voxel=float(voxel), origin=tuple(origin))
    return SimpleNamespace(name=name, field=field, view=view, depth=scene_image(w, h, z_wall, z_disc, z_max, kind))


INSIDE = (6.37, 5.21, 9.43)
TOWARDS = (1.0, 0.8, 0.35)
CASES = [
    _case("48x40x32-64x48-inside", (48, 40, 32), 0.05, (64, 48), 1, INSIDE, TOWARDS),
    _case("48x40x32-64x48-inside-stride3", (48, 40, 32), 0.05, (64, 48), 3, INSIDE, TOWARDS),
    _case("48x40x32-64x48-outside", (48, 40, 32), 0.05, (64, 48), 3, (-9.4, 12.3, 14.6), (1.0, 0.3, 0.1), z_wall=2.2, z_disc=1.3, z_max=3.0),
    _case("48x40x32-7x5-inside", (48, 40, 32), 0.05, (7, 5), 1, INSIDE, TOWARDS),
    _case("33x17x9-64x48-inside", (33, 17, 9), 0.05, (64, 48), 1, (3.37, 8.21, 4.43), (1.0, -0.2, 0.1), z_wall=1.2, z_disc=0.6),
    _case("33x17x9-7x5-inside", (33, 17, 9), 0.05, (7, 5), 1, (3.37, 8.21, 4.43), (1.0, -0.2, 0.1), z_wall=1.2, z_disc=0.6),
    _case("33x17x9-7x5-away", (33, 17, 9), 0.05, (7, 5), 1, (-3.37, 8.21, 4.43), (-1.0, 0.1, 0.2)),
    _case("33x17x9-7x5-nan", (33, 17, 9), 0.05, (7, 5), 1, (3.37, 8.21, 4.43), (1.0, -0.2, 0.1), kind="nan"),
    _case("33x17x9-7x5-zmax", (33, 17, 9), 0.05, (7, 5), 1, (3.37, 8.21, 4.43), (1.0, -0.2, 0.1), kind="zmax", z_max=0.93),
    _case("16x12x10-64x48-inside", (16, 12, 10), 0.1, (64, 48), 1, (2.37, 3.21, 4.43), (1.0, 0.5, 0.1), z_wall=1.1, z_disc=0.6),
    _case("16x12x10-64x48-inf", (16, 12, 10), 0.1, (64, 48), 3, (2.37, 3.21, 4.43), (1.0, 0.5, 0.1), kind="inf", z_max=0.9),
    _case("16x12x10-1x1", (16, 12, 10), 0.1, (1, 1), 1, (2.37, 3.21, 4.43), (1.0, 0.5, 0.1), kind="wall", z_wall=0.8, fx=1.0),
    _case("16x12x10-7x5-markonly", (16, 12, 10), 0.1, (7, 5), 1, (2.37, 3.21, 4.43), (1.0, 0.5, 0.1), z_wall=0.8, z_disc=0.5, carve=False),
    _case("512x2x2-64x48-along-x", (512, 2, 2), 0.05, (64, 48), 1, (3.37, 0.41, 0.33), (1.0, 0.004, 0.002), z_wall=5.0, z_disc=2.5,
          z_max=6.0, fx=900.0),
]


def before_map(case, seed=3, share=0.06):
    """A map to integrate into: a random `share` of the nodes occupied, so that carving shows."""
    rng = np.random.default_rng(seed)
    return (rng.random(case.field.dims[::-1]) < share).astype(np.uint8)


# ------------------------------------------------------------------------------------------ the geometry
def _f32(x):
    return np.asarray(np.asarray(x, np.float32), np.float64)


def tol_u(case):
    v, f = case.view, case.field
    voxel = float(_f32(f.voxel))
    P, O = float(np.max(np.abs(_f32(v.pos)))), float(np.max(np.abs(_f32(f.origin))))
    xn = max(abs(0.0 - v.cx), abs(v.width - 1.0 - v.cx)) / v.fx
    yn = max(abs(0.0 - v.cy), abs(v.height - 1.0 - v.cy)) / v.fy
    rho = float(v.z_max) * np.sqrt(1.0 + xn * xn + yn * yn)
    tol_end = EPS * (3.0 * (P + rho) + 21.0 * rho + 3.0 * (P + rho + O)) / voxel
    return tol_end + 3.0 * EPS * 2.0 * (P + rho + O) / voxel


def _rays(case, variant=None):
    """kind (N,) 0 skipped / 1 return / 2 miss, ue (N, 3), uo (3,) of the used pixels, in float64 from the
    float32 values the structs hold."""
    v, f = case.view, case.field
    depth = np.asarray(case.depth, np.float32)
    stride = 1 if variant == "stride_ignored" else int(v.stride)
    jj, ii = np.meshgrid(np.arange(0, v.height, stride), np.arange(0, v.width, stride), indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()
    z32 = depth[jj, ii]
    z_min, z_max = np.float32(v.z_min), np.float32(v.z_max)
    with np.errstate(invalid="ignore"):
        skip = ~(z32 >= z_min)
        hit = ~skip & (z32 <= z_max)
    kind = np.where(skip, 0, np.where(hit, 1, 2))
    z = np.where(hit, z32.astype(np.float64), float(z_max))
    z = np.where(skip, 1.0, z)
    fx, fy, cx, cy = (float(_f32(x)) for x in (v.fx, v.fy, v.cx, v.cy))
    if variant == "principal_swap":
        cx, cy = cy, cx
    xn, yn = (ii - cx) / fx, (jj - cy) / fy
    p = np.stack([xn * z, yn * z, z], -1)
    if variant == "x_forward":
        p = np.stack([z, -xn * z, -yn * z], -1)
    q = _f32(v.quat_xyzw)
    if variant == "quat_wxyz":
        q = np.array([q[1], q[2], q[3], q[0]])
    pos, origin, voxel = _f32(v.pos), _f32(f.origin), float(_f32(f.voxel))
    w = p @ quat_R(q).T + pos
    return kind, (w - origin) / voxel, (pos - origin) / voxel


def _flat(dims, c):
    """flat node index of integer coordinates c (..., 3), -1 outside the grid"""
    nx, ny, nz = dims
    inside = (c[..., 0] >= 0) & (c[..., 0] < nx) & (c[..., 1] >= 0) & (c[..., 1] < ny) & (c[..., 2] >= 0) & (c[..., 2] < nz)
    return np.where(inside, (c[..., 2] * ny + c[..., 1]) * nx + c[..., 0], -1)


def _candidates(dims, u, tol):
    """(decided (...,), cand (..., 8)): the nodes the points u (..., 3) can fall in under a perturbation of
    tol per axis (-1: outside the grid), and whether all eight agree."""
    lo, hi = np.floor(u + 0.5 - tol).astype(np.int64), np.floor(u + 0.5 + tol).astype(np.int64)
    decided = np.all(lo == hi, axis=-1)
    cand = [_flat(dims, np.stack([(lo, hi)[a][..., 0], (lo, hi)[b][..., 1], (lo, hi)[c][..., 2]], -1))
            for a, b, c in itertools.product((0, 1), repeat=3)]
    return decided, np.stack(cand, -1)


def _samples(uo, du, n):
    """u (R, nmax, 3) and valid (R, nmax) for rays with per-ray sample counts n (R,)"""
    m = np.arange(int(n.max()) if len(n) else 0)
    valid = m[None, :] < n[:, None]
    t = m[None, :] / n[:, None]
    return uo + t[..., None] * du[:, None, :], valid


def integrate(case, tol=None):
    """The four sets of one image (see the module docstring)."""
    dims = case.field.dims
    nvox = int(np.prod(dims))
    tol = tol_u(case) if tol is None else tol
    kind, ue, uo = _rays(case)
    sets = {k: np.zeros(nvox, bool) for k in ("F_certain", "F_possible", "O_certain", "O_possible")}
    live = kind > 0
    kind, ue = kind[live], ue[live]
    e_decided, e_cand = _candidates(dims, ue, tol)
    ret = kind == 1
    for c in range(8):
        sets["O_possible"][e_cand[ret, c][e_cand[ret, c] >= 0]] = True
    sure = ret & e_decided & (e_cand[:, 0] >= 0)
    sets["O_certain"][e_cand[sure, 0]] = True
    if case.view.carve and len(kind):
        e_cand = np.where(ret[:, None], e_cand, -1)           # a miss excludes nothing
        e_sure = np.where(ret, e_decided, True)
        du = ue - uo
        L2 = 2.0 * np.max(np.abs(du), axis=-1)
        n_lo = np.clip(np.ceil(L2 - 2.0 * tol), 1, MAX_SAMPLES).astype(np.int64)
        n_hi = np.clip(np.ceil(L2 + 2.0 * tol), 1, MAX_SAMPLES).astype(np.int64)
        for n, certain_ok in ((n_lo, n_lo == n_hi), (n_hi, np.zeros(len(n_hi), bool))):
            rows = np.ones(len(n), bool) if n is n_lo else (n_lo != n_hi)
            if not rows.any():
                continue
            u, valid = _samples(uo, du[rows], n[rows])
            decided, cand = _candidates(dims, u, tol)
            ec, es = e_cand[rows], e_sure[rows]
            own = np.any((cand[..., :1] == ec[:, None, :]) & (ec[:, None, :] >= 0), axis=-1)   # a candidate of the end node
            cert = valid & decided & (cand[..., 0] >= 0) & ~own & certain_ok[rows][:, None]
            sets["F_certain"][cand[..., 0][cert]] = True
            for c in range(8):
                excluded = es[:, None] & (cand[..., c] == ec[:, :1]) & (ec[:, :1] >= 0)
                poss = valid & (cand[..., c] >= 0) & ~excluded
                sets["F_possible"][cand[..., c][poss]] = True
    shape = dims[::-1]
    out = {k: a.reshape(shape) for k, a in sets.items()}
    assert not (out["F_certain"] & ~out["F_possible"]).any() and not (out["O_certain"] & ~out["O_possible"]).any()
    return out


def undecided(sets):
    def share(c, p):
        return 0.0 if p.sum() == 0 else 1.0 - float(c.sum()) / float(p.sum())
    return share(sets["F_certain"], sets["F_possible"]), share(sets["O_certain"], sets["O_possible"])


def check(before, after, sets):
    """The violations of the rule (an empty list: the map passes)."""
    before, after = np.asarray(before) != 0, np.asarray(after)
    bad = []
    if not np.isin(after, (0, 1)).all():
        bad.append("a node holds something other than 0 or 1")
    after = after != 0
    n = int((sets["O_certain"] & ~after).sum())
    if n:
        bad.append(f"{n} of {int(sets['O_certain'].sum())} certain end nodes are not occupied")
    must_free = sets["F_certain"] & ~sets["O_possible"]
    n = int((must_free & after).sum())
    if n:
        bad.append(f"{n} of {int(must_free.sum())} certainly carved nodes are not free")
    untouched = ~(sets["F_possible"] | sets["O_possible"])
    n = int((untouched & (after != before)).sum())
    if n:
        bad.append(f"{n} nodes outside F_possible U O_possible changed")
    return bad


# ------------------------------------------------------------------- a plain float64 implementation
def model(case, before, variant=None):
    """The map after one image by the definition in float64, no tolerance; `variant`: a planted mistake."""
    assert variant is None or variant in VARIANTS
    dims = case.field.dims
    occ = (np.asarray(before) != 0).astype(np.uint8).ravel().copy()
    kind, ue, uo = _rays(case, variant)

    def node(u):
        return _flat(dims, np.floor(u if variant == "cell_corner" else u + 0.5).astype(np.int64))

    marks = (kind == 1) | ((kind == 2) & (variant == "miss_marks"))
    end = np.where(marks, node(ue), -1)
    own = np.where(kind == 1, node(ue), -1)
    du = ue - uo
    n = np.clip(np.ceil(2.0 * np.max(np.abs(du), axis=-1)), 1, MAX_SAMPLES).astype(np.int64)

    def carve(rows):
        if not case.view.carve or not rows.any():
            return
        u, valid = _samples(uo, du[rows], n[rows])
        s = node(u)
        keep = valid & (s >= 0)
        if variant != "endpoint_cleared":
            keep &= s != own[rows][:, None]
        occ[s[keep]] = 0

    def mark(rows):
        e = end[rows]
        occ[e[e >= 0]] = 1

    live = kind > 0
    if variant == "endpoint_cleared":
        for r in np.flatnonzero(live):
            one = np.zeros(len(kind), bool)
            one[r] = True
            mark(one)
            carve(one)
    elif variant == "free_wins":
        mark(live)
        carve(live)
    else:
        carve(live)
        mark(live)
    return occ.reshape(dims[::-1])


def shifted(before, shift):
    """mppi_shift_map's map by numpy slices: new[iz, iy, ix] = old[iz + sz, iy + sy, ix + sx], 0 outside."""
    before = np.asarray(before)
    out = np.zeros_like(before)
    nz, ny, nx = before.shape
    sx, sy, sz = (int(s) for s in shift)

    def rng(n, s):
        lo, hi = max(0, -s), min(n, n - s)
        return (slice(lo, hi), slice(lo + s, hi + s)) if lo < hi else None
    r = [rng(nz, sz), rng(ny, sy), rng(nx, sx)]
    if all(x is not None for x in r):
        out[r[0][0], r[1][0], r[2][0]] = before[r[0][1], r[1][1], r[2][1]]
    return out
