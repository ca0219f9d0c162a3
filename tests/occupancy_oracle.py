"""The float64 oracle of occupancy grids (mppi_set_occupancy, mppi_occupancy_field; include/mppi_hip.h).

D2_occ / D2_free, the smallest squared index distance of every node to an occupied / a free node, come
from scipy.ndimage.distance_transform_edt(..., return_indices=True): the indices of the nearest seed,
from which the squared distance is an exact integer (checked against brute force below at the small
grids, test_capi_occupancy_cpu.py).  The empty and the full grid -- a seed set without members, which
scipy leaves undefined -- are handled here: D2 = NONE.  The value is, in float64 over the fp32 voxel,

    d = +-voxel (sqrt(D2) - 0.5), clamped to [-cap, +cap];   NONE reads the cap itself

with cap = float32(max_dist) when max_dist > 0, else float32(voxel) * float32(nx + ny + nz).

Tolerance against float64 (derived, not measured): the code forms sqrtf, a subtraction and a product,
three correctly rounded fp32 operations of relative error 2^-24 each on a value of magnitude at most
voxel * max(1, sqrt(D2)), then a clamp that adds none:

    tol(n) = 4 * 2^-24 * voxel * max(1, sqrt(D2(n)))

One unit of error in a D2 moves d by voxel (sqrt(D2 + 1) - sqrt(D2)) ~ voxel / (2 sqrt(D2)); field()
asserts that this is more than RESOLVE = 100 times the tolerance for every D2 of the case the clamp leaves
alone, which holds while D2 < ~20900 (a distance of 144 nodes).  At dims up to 512 the ratio falls to ~8,
so a case whose uncapped distances reach further is given a cap (uncapped_or below: 140 voxels), never a
wider tolerance.

mistakes(): the fields four mistakes would give, for the tests to assert -- on the oracle alone -- that a
case can show them: the 0.5 offset dropped, the seed sets swapped, one axis' pass skipped (three of them).
The fourth of the issue's list, the x-pair's second word taken from ix, lives in the packing and is
asserted through field_sample by the tests themselves.
"""
import numpy as np
from scipy import ndimage

NONE = np.int64(1) << 40      # "no seed of this set in the grid"
RESOLVE = 100.0
EPS = 2.0 ** -24
FAR_D2 = 20000                # beyond this an uncapped case cannot meet RESOLVE
FAR_CAP_VOXELS = 140.0        # (140.5^2 = 19740 < 20900)

DIMS = [(2, 2, 2), (33, 20, 24), (70, 5, 3), (512, 4, 4), (4, 512, 4), (4, 4, 512), (64, 64, 16)]   # (nx, ny, nz)
PATTERNS = ["empty", "full", "corner", "box", "face", "random", "checker"]
VOXEL = 0.05


def pattern(name, dims, seed=0):
    """occ (nz, ny, nx) bool.  box: [n // 4, max(n // 4 + 1, 3 n // 4)) per axis; face: the whole face at index 0
    of the shortest axis (the first of them), so its distances stay short on the long grids; random: 2 % of
    the nodes, at least one."""
    nx, ny, nz = dims
    occ = np.zeros((nz, ny, nx), bool)
    if name == "full":
        occ[:] = True
    elif name == "corner":
        occ[nz - 1, 0, nx - 1] = True
    elif name == "box":
        lo = [n // 4 for n in (nz, ny, nx)]
        hi = [max(n // 4 + 1, 3 * n // 4) for n in (nz, ny, nx)]
        occ[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    elif name == "face":
        ax = int(np.argmin(dims))            # 0: x, 1: y, 2: z
        idx = [slice(None)] * 3
        idx[2 - ax] = 0
        occ[tuple(idx)] = True
    elif name == "random":
        rng = np.random.default_rng(1000 * seed + nx + 7 * ny + 13 * nz)
        occ = rng.random((nz, ny, nx)) < 0.02
        if not occ.any():
            occ[rng.integers(nz), rng.integers(ny), rng.integers(nx)] = True
    elif name == "checker":
        z, y, x = np.indices((nz, ny, nx))
        occ = ((x + y + z) % 2) == 0
    elif name != "empty":
        raise KeyError(name)
    return occ


def squared_distances(occ):
    """(D2_occ, D2_free) int64, NONE where the set is empty."""
    occ = np.asarray(occ, bool)
    grid = np.indices(occ.shape)

    def to_seeds(seeds):
        if not seeds.any():
            return np.full(occ.shape, NONE, np.int64)
        idx = ndimage.distance_transform_edt(~seeds, return_distances=False, return_indices=True)
        return ((idx.astype(np.int64) - grid) ** 2).sum(0)
    return to_seeds(occ), to_seeds(~occ)


def brute_squared_distances(occ):
    """The same by brute force (small grids only)."""
    occ = np.asarray(occ, bool)
    pts = np.argwhere(np.ones_like(occ)).astype(np.int64)

    def to_seeds(seeds):
        s = np.argwhere(seeds).astype(np.int64)
        if not len(s):
            return np.full(occ.shape, NONE, np.int64)
        return ((pts[:, None, :] - s[None, :, :]) ** 2).sum(-1).min(1).reshape(occ.shape)
    return to_seeds(occ), to_seeds(~occ)


def cap_of(dims, voxel, max_dist):
    v = np.float32(voxel)
    if max_dist is not None and max_dist > 0:
        return float(np.float32(max_dist))
    return float(v * np.float32(dims[0] + dims[1] + dims[2]))


def value(D2_occ, D2_free, occ, voxel, cap, offset=0.5):
    v = float(np.float32(voxel))
    D2 = np.where(occ, D2_free, D2_occ)
    mag = np.where(D2 >= NONE, cap, np.minimum(v * (np.sqrt(np.minimum(D2, NONE).astype(np.float64)) - offset), cap))
    return np.where(occ, -mag, mag), D2


def field(occ, dims, voxel, max_dist=None, resolve=True):
    """dict(d float64 (nz, ny, nx), D2 int64 (the set that counts per node), tol, cap, unclamped mask)."""
    occ = np.asarray(occ, bool)
    assert occ.shape == tuple(dims[::-1])
    v = float(np.float32(voxel))
    cap = cap_of(dims, voxel, max_dist)
    Do, Df = squared_distances(occ)
    d, D2 = value(Do, Df, occ, voxel, cap)
    root = np.sqrt(np.minimum(D2, NONE).astype(np.float64))
    tol = 4.0 * EPS * v * np.maximum(1.0, np.where(D2 >= NONE, 1.0, root))
    free = (D2 < NONE) & (np.abs(d) < cap)     # the nodes the clamp leaves alone
    if resolve and free.any():
        u = np.unique(D2[free]).astype(np.float64)
        move = v * (np.sqrt(u + 1.0) - np.sqrt(u))
        ratio = float(np.min(move / (4.0 * EPS * v * np.maximum(1.0, np.sqrt(u)))))
        assert ratio > RESOLVE, f"a unit of D2 moves d by only {ratio:.1f} x the tolerance (D2 up to {int(u.max())}): shrink or cap the case"
    return dict(d=d, D2=D2, D2_occ=Do, D2_free=Df, tol=tol, cap=cap, unclamped=free, occ=occ)


def uncapped_or(occ, dims, voxel):
    """max_dist for a case's "no cap" variant: None while every distance of the grid can be resolved at
    RESOLVE x the tolerance, else FAR_CAP_VOXELS voxels (module docstring)."""
    occ = np.asarray(occ, bool)
    Do, Df = squared_distances(occ)
    D2 = np.where(occ, Df, Do)
    far = D2[D2 < NONE]
    return None if not far.size or far.max() <= FAR_D2 else FAR_CAP_VOXELS * float(np.float32(voxel))


def _skip_axis(seeds, axis):
    """D2 to `seeds` with one axis' pass left out: only seeds at the node's own index on that axis count."""
    out = np.full(seeds.shape, NONE, np.int64)
    for i in range(seeds.shape[axis]):
        sl = [slice(None)] * 3
        sl[axis] = slice(i, i + 1)
        sub = seeds[tuple(sl)]
        if sub.any():
            idx = ndimage.distance_transform_edt(~sub, return_distances=False, return_indices=True)
            out[tuple(sl)] = ((idx.astype(np.int64) - np.indices(sub.shape)) ** 2).sum(0)
    return out


def mistakes(ref, voxel):
    """name -> the worst |mistaken d - d| / tol over the grid."""
    occ, cap = ref["occ"], ref["cap"]
    out = {}
    wrong = {"no_offset": value(ref["D2_occ"], ref["D2_free"], occ, voxel, cap, offset=0.0)[0],
             "swapped": value(ref["D2_free"], ref["D2_occ"], ~occ, voxel, cap)[0]}
    for axis, name in ((2, "skip_x"), (1, "skip_y"), (0, "skip_z")):
        wrong[name] = value(_skip_axis(occ, axis), _skip_axis(~occ, axis), occ, voxel, cap)[0]
    for name, d in wrong.items():
        out[name] = float(np.max(np.abs(d - ref["d"]) / ref["tol"]))
    return out
