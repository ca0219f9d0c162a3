"""Distance-field environments (mppi_create_scene_field, mppi_set_distance_field) without a GPU: the
exports and the binding, every error of the descriptor and of the data through the host-side layout
path (mppi_debug_field_layout), the packed buffer against a numpy restatement, the library's own
sampler (mppi_debug_field_sample: csrc/mppi_field.h field_sample, the inline the kernels run) against
the float64 oracle (tests/field_oracle.py) with its tolerance and Lipschitz constant, hostile
coordinates, the field launchers' kernel choice and argument layout, and the drop-in classes.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import field_oracle as FO
import obstacle_oracle as OO
import test_capi_obstacles_cpu as TC
from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd import build as B
from quadrotor_manipulator_mppi_amd.engine import DistanceField, Scene, make_config

ROOT = TC.ROOT
DRONE, ARM, WB, QUAD = TC.DRONE, TC.ARM, TC.WB, TC.QUAD
HDR_W = 16   # csrc/mppi_field.h
NEW = ("mppi_create_scene_field", "mppi_set_distance_field")
_bind = TC._bind


# ------------------------------------------------------------------------- exports and config
def test_exports_binding_and_header_text():
    with open(os.path.join(ROOT, "include", "mppi_hip.h")) as f:
        header = f.read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in capi.PROTOTYPES, name
    for name in ("mppi_debug_field_layout", "mppi_debug_field_sample", "mppi_debug_field_step_launches",
                 "mppi_debug_field_rollout_kernels"):
        assert hasattr(L, name) and name in capi.DEBUG_PROTOTYPES, name
    assert re.search(r"#define\s+MPPI_FIELD_MAX_VOXELS\s+\(1\s*<<\s*21\)", header) and capi.FIELD_MAX_VOXELS == 1 << 21
    assert "mppi_field_desc" in header and "pad the grid" in header and "clamped position" in header
    assert re.search(r"#define\s+MPPI_ABI_VERSION\s+10\b", header)
    assert L.mppi_abi_version() == 10 == capi.ABI_VERSION
    sizes = [C.c_int32(), C.c_int32(), C.c_int32()]
    L.mppi_struct_sizes(*[C.byref(s) for s in sizes])
    assert tuple(s.value for s in sizes) == (C.sizeof(capi.Config), C.sizeof(capi.Joint), C.sizeof(capi.Stats))
    assert C.sizeof(capi.BodySphere) == 20 and C.sizeof(capi.Scene) == 4 + 16 * 20 + 12
    assert C.sizeof(capi.FieldDesc) == 32


def _layout(cfg, desc, origin=None, d=None, words=False):
    f = _bind("mppi_debug_field_layout")
    fd = desc.to_c() if isinstance(desc, DistanceField) else desc
    o = None if origin is None else np.ascontiguousarray(origin, np.float32)
    dd = None if d is None else np.ascontiguousarray(d, np.float32)
    w = None
    if words:
        w = np.full(HDR_W + 2 * int(np.prod(fd.dims[:])), -7.0, np.float32)
    st = f(C.byref(cfg), None if fd is None else C.byref(fd), capi.fptr(o), capi.fptr(dd), capi.fptr(w))
    return (st, w) if words else st


def _wall_sphere(dims=FO.DIMS, voxel=FO.VOXEL, origin=(-0.31, 0.17, 0.83)):
    """The tolerance check's field: a wall united with a sphere, not symmetric in any pair of axes."""
    def sdf(X, Y, Z):
        P = np.stack([X, Y, Z], -1)
        n = np.array([0.48, 0.6, 0.64])
        wall = (P - (np.asarray(origin) + [0.9, 0.5, 0.4])) @ -n
        ball = np.linalg.norm(P - (np.asarray(origin) + [0.35, 0.55, 0.3]), axis=-1) - 0.22
        return np.minimum(wall, ball)
    return FO.rasterise(sdf, dims, voxel, origin)


@pytest.mark.parametrize("model", ["drone", "arm", "wholebody"])
def test_descriptor_and_data_errors(model):
    cfg = make_config(model, n_samples=64, n_horizon=32)
    ok = DistanceField(FO.DIMS, FO.VOXEL, (0.1, -0.2, 0.3))
    assert _layout(cfg, ok) == capi.OK, capi.lib().mppi_last_error()
    assert _layout(cfg, None) == capi.ERR_INVALID_ARG                        # a NULL descriptor
    for dims in ((1, 20, 16), (24, 513, 16), (24, 20, 0), (-3, 20, 16), (512, 512, 16), (256, 256, 33)):
        assert _layout(cfg, DistanceField(dims, 0.05)) == capi.ERR_INVALID_ARG, dims
    assert _layout(cfg, DistanceField((512, 512, 8), 0.05)) == capi.OK          # exactly MPPI_FIELD_MAX_VOXELS
    assert _layout(cfg, DistanceField((2, 2, 2), 0.05)) == capi.OK
    for voxel in (0.0, -0.05, np.nan, np.inf, 1e-45):
        assert _layout(cfg, DistanceField(FO.DIMS, voxel)) == capi.ERR_INVALID_ARG, voxel
    for o in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
        assert _layout(cfg, DistanceField(FO.DIMS, FO.VOXEL, o)) == capi.ERR_INVALID_ARG, o
        assert _layout(cfg, ok, origin=o) == capi.ERR_INVALID_ARG, o
    c = ok.to_c()
    c.reserved = 1                                                           # documented as 0
    assert _layout(cfg, c) == capi.ERR_INVALID_ARG and b"reserved" in capi.lib().mppi_last_error()
    d = np.ones(ok.shape, np.float32)
    assert _layout(cfg, ok, d=d) == capi.OK
    for idx, x in (((0, 0, 0), np.nan), ((15, 19, 23), np.inf), ((7, 3, 11), -np.inf)):
        bad = d.copy()
        bad[idx] = x
        assert _layout(cfg, ok, d=bad) == capi.ERR_INVALID_ARG, (idx, x)


def test_quadrotor_field_is_refused():
    """Through the validation mppi_create_scene_field itself runs (field_engine_validate: the default scene's
    scene_validate refuses the model), and -- before any device is looked for -- through the entry point."""
    cfg = make_config("quadrotor", n_samples=64, n_horizon=32)
    assert _layout(cfg, DistanceField(FO.DIMS, FO.VOXEL)) == capi.ERR_INVALID_ARG
    assert b"QUADROTOR" in capi.lib().mppi_last_error()
    L, h = capi.lib(), C.c_void_p()
    fd = DistanceField(FO.DIMS, FO.VOXEL).to_c()
    assert L.mppi_create_scene_field(C.byref(cfg), None, C.byref(fd), C.byref(h)) == capi.ERR_INVALID_ARG and not h.value
    assert b"QUADROTOR" in L.mppi_last_error()
    arm = make_config("arm", n_samples=64, n_horizon=32)
    assert L.mppi_create_scene_field(C.byref(arm), None, None, C.byref(h)) == capi.ERR_INVALID_ARG    # a NULL descriptor
    bad = DistanceField((1, 20, 16), FO.VOXEL).to_c()
    assert L.mppi_create_scene_field(C.byref(arm), None, C.byref(bad), C.byref(h)) == capi.ERR_INVALID_ARG and not h.value
    assert L.mppi_set_distance_field(None, None, None) == capi.ERR_INVALID_ARG                      # a NULL engine
    from quadrotor_manipulator_mppi_amd.mppi_solver.quadrotor_mppi import MPPI
    with pytest.raises(NotImplementedError):
        MPPI(field=DistanceField(FO.DIMS, FO.VOXEL))


def test_packed_layout_against_numpy():
    cfg = make_config("arm", n_samples=64, n_horizon=32)
    fld = _wall_sphere()
    nx, ny, nz = fld.dims
    desc = DistanceField(fld.dims, fld.voxel, fld.origin)
    new_origin = np.array([1.5, -2.25, 0.125], np.float32)
    for origin, d in ((None, fld.d), (new_origin, fld.d), (None, None)):
        st, w = _layout(cfg, desc, origin=origin, d=d, words=True)
        assert st == capi.OK
        wi = w.view(np.int32)
        assert np.array_equal(w[:3], fld.origin if origin is None else new_origin)
        assert w[3] == np.float32(1.0) / np.float32(fld.voxel) and w[11] == np.float32(fld.voxel)
        assert list(wi[4:7]) == [nx, ny, nz] and wi[7] == (0 if d is None else 1)
        assert wi[8] == nx and wi[9] == nx * ny and wi[10] == nx * ny * nz and not wi[12:16].any()
        cells = w[HDR_W:].reshape(nz, ny, nx, 2)
        if d is None:
            assert not cells.any()
        else:
            assert np.array_equal(cells[..., 0], fld.d)
            assert np.array_equal(cells[..., :-1, 1], fld.d[..., 1:])
            assert np.array_equal(cells[..., -1, 1], fld.d[..., -1])


def _sample(words, pts):
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    val = np.empty(len(pts), np.float32)
    idx = np.empty((len(pts), 8), np.int32)
    st = _bind("mppi_debug_field_sample")(capi.fptr(words), len(pts), capi.fptr(pts), capi.fptr(val),
                                          idx.ctypes.data_as(C.POINTER(C.c_int32)))
    assert st == capi.OK
    return val, idx


def test_sampler_against_the_oracle_and_the_lipschitz_bound():
    """1e5 points, a quarter of them outside the grid: |d_lib - d_ref| <= TOL_D (same float32 points
    into both, so TOL_C = 0), the ratio printed; and the interpolant's measured Lipschitz ratio
    against G on 1e5 random pairs."""
    cfg = make_config("arm", n_samples=64, n_horizon=32)
    fld = _wall_sphere()
    st, words = _layout(cfg, DistanceField(fld.dims, fld.voxel, fld.origin), d=fld.d, words=True)
    assert st == capi.OK
    rng = np.random.default_rng(5)
    lo = fld.origin.astype(np.float64)
    span = fld.voxel * (np.asarray(fld.dims) - 1.0)
    pts = (lo + span * rng.uniform(-0.05, 1.05, size=(100000, 3))).astype(np.float32)
    outside = np.any((pts < lo) | (pts > lo + span), axis=1)
    assert 0.2 < outside.mean() < 0.35
    val, idx = _sample(words, pts)
    ref = FO.sample(fld, pts.astype(np.float64))
    tol = fld.tol_d(pts.astype(np.float64))
    ratio = float(np.max(np.abs(val.astype(np.float64) - ref) / tol))
    print(f"field sampler vs the float64 oracle: max |err| / TOL_D = {ratio:.3f} (G = {fld.G:.2f}, TOL_D ~ {tol.mean():.2e})")
    assert ratio <= 1.0
    assert idx.min() >= 0 and idx.max() < int(np.prod(fld.dims))
    # the eight indices are the cell's corners, x fastest
    nx, ny, _ = fld.dims
    assert np.array_equal(idx - idx[:, :1], np.tile([0, 1, nx, nx + 1, nx * ny, nx * ny + 1, nx * ny + nx, nx * ny + nx + 1],
                                                    (len(pts), 1)))
    a = lo + span * rng.uniform(-0.05, 1.05, size=(100000, 3))
    b = a + rng.normal(size=a.shape) * fld.voxel * 0.3
    lip = np.abs(FO.sample(fld, a) - FO.sample(fld, b)) / np.abs(a - b).max(axis=1)
    print(f"measured Lipschitz ratio max |dd| / |dc|_inf / G = {lip.max() / fld.G:.3f}")
    assert lip.max() <= fld.G * (1 + 1e-9)
    # every mistake of the oracle's list moves the sampled values well past TOL_D
    for variant in ("axis_order", "cell_centred", "nearest", "no_origin"):
        dv = np.abs(FO.sample(fld, pts.astype(np.float64), variant) - ref)
        assert dv.max() > 1e3 * tol.max(), variant


def test_hostile_coordinates_land_on_the_grid():
    cfg = make_config("arm", n_samples=64, n_horizon=32)
    fld = _wall_sphere()
    st, words = _layout(cfg, DistanceField(fld.dims, fld.voxel, fld.origin), d=fld.d, words=True)
    assert st == capi.OK
    lo = fld.origin.astype(np.float64)
    hi = (lo + np.float32(fld.voxel) * (np.asarray(fld.dims) - 1.0)).astype(np.float32)
    specials = [np.nan, np.inf, -np.inf, 1e30, -1e30, 3.4e38, -3.4e38, 0.0]
    pts = [(x, y, z) for x in specials for y in specials[:5] for z in specials[:5]]
    pts += [tuple(hi), (hi[0], lo[1], lo[2]), (lo[0], hi[1], lo[2]), (lo[0], lo[1], hi[2]), tuple(np.nextafter(hi, np.inf)),
            tuple(lo), tuple(np.nextafter(lo.astype(np.float32), -np.inf))]
    val, idx = _sample(words, pts)
    assert np.isfinite(val).all()
    assert idx.min() >= 0 and idx.max() < int(np.prod(fld.dims))
    # the far corner reads the last node, a NaN coordinate the clamped position 0 on that axis
    assert val[len(pts) - 7] == fld.d[-1, -1, -1]
    v_nan, _ = _sample(words, [(np.nan, lo[1] + 0.2, lo[2] + 0.2)])
    v_0, _ = _sample(words, [(lo[0], lo[1] + 0.2, lo[2] + 0.2)])
    assert v_nan[0] == v_0[0]


# ---------------------------------------------------------------------------- rollout symbols
@pytest.mark.parametrize("model,A,f64,unit,H,V", TC.CASES, ids=[f"m{m}-f{f}-H{H}-V{V}" for m, _, f, _, H, V in TC.CASES])
def test_field_symbols(model, A, f64, unit, H, V):
    blob = None
    for terms in (0, 32, 32 | capi.COST_CENTER):
        if model == DRONE and terms & 31:
            continue
        st, full, quiet, seg, nch = TC._kernels("mppi_debug_field_rollout_kernels", model, A, H, V=V, f64=f64, cost_terms=terms)
        assert st == 0 and full == quiet, "field engines run the full kernel on every step"
        assert full.startswith(f"_Z12k_rollout_dfILi{model}ELi{A}ELi{nch}ELi{seg}ELb{f64}ELb{int(V == 1)}EEv"), full
        if blob is None:
            with open(B.code_object_path(B.LIB, unit(seg, nch)), "rb") as f:
                blob = f.read()
        assert (full + ".kd").encode() in blob, (unit(seg, nch), full)
    # a scene engine and a plain one: the symbols as they were
    st, full, quiet, _, _ = TC._kernels("mppi_debug_scene_rollout_kernels", model, A, H, V=V, f64=f64)
    assert st == 0 and "k_rollout_ob" in full and "_df" not in full
    st, full, quiet, _, _ = TC._kernels("mppi_debug_rollout_kernels", model, A, H, V=V, f64=f64)
    assert st == 0 and "_df" not in full and "_ob" not in full and "_df" not in quiet


def test_no_quadrotor_field_kernel():
    st, _, _, _, _ = TC._kernels("mppi_debug_field_rollout_kernels", QUAD, 4, 32)
    assert st == capi.ERR_INVALID_ARG


# ---------------------------------------------------------------------------- argument layout
def _launches(cfg, scene, desc, **sw):
    words = (C.c_int32 * len(TC.SW_ORDER))(*[sw.get(k, 0) for k in TC.SW_ORDER])
    buf = C.create_string_buffer(4096)
    arg = C.c_uint64(0)
    sc, fd = scene.to_c(), desc.to_c()
    st = _bind("mppi_debug_field_step_launches")(C.byref(cfg), C.byref(sc), C.byref(fd), words, buf, len(buf), C.byref(arg))
    assert st == capi.OK, capi.lib().mppi_last_error()
    return [TC.LINE.fullmatch(ln).groups() for ln in buf.value.decode().splitlines()], arg.value


@pytest.mark.parametrize("path,n", [(0, 3), (2, 3), (3, 1)], ids=["hip-batch", "native-batch", "native-call"])
@pytest.mark.parametrize("model", ["arm", "wholebody", "drone"])
def test_step_launches_carry_the_field_pointer(model, path, n):
    """HIP batch, native batch and native call of a field engine: the field rollout on every step, its
    argument block the scene launch's plus the 8 bytes of the field pointer -- at offset 64, after the
    scene pointer and before the trailing DevParams -- grid, block and LDS the scene launch's, the
    finalize unchanged."""
    cfg = make_config(model, n_samples=256, n_horizon=32)
    scene = Scene.default(cfg)
    df, arg = _launches(cfg, scene, DistanceField(FO.DIMS, FO.VOXEL), path=path, n=n)
    ob = TC._launches(cfg, scene, path=path, n=n)
    assert arg == 0x8000, hex(arg)   # the stand-in field buffer of the described engine
    assert len(df) == len(ob) == (4 if n > 1 else 2)
    for d, o in zip(df, ob):
        assert d[:2] == o[:2]
        if d[1] == "rollout":
            assert "k_rollout_df" in d[2] and "k_rollout_ob" in o[2]
            assert int(d[6]) == int(o[6]) + 8, (d, o)
            assert d[3:6] == o[3:6]   # grid, block, LDS
        else:
            assert d[2:] == o[2:]


def test_scene_and_plain_engines_are_described_as_before():
    for model in ("arm", "drone", "wholebody"):
        cfg = make_config(model, n_samples=256, n_horizon=32)
        for path, n in ((0, 3), (2, 3)):
            assert TC._launches(cfg, None, path=path, n=n) == TC._launches(cfg, plain=True, path=path, n=n)
            assert all("_df" not in ln[2] for ln in TC._launches(cfg, Scene.default(cfg), path=path, n=n))


# ------------------------------------------------------------------------- python layer, drop-ins
def test_distance_field_constructors():
    f = DistanceField.from_boxes([((0.2, 0.1, 0.0), (0.4, 0.5, 0.3))], FO.DIMS, FO.VOXEL, origin=(0.0, 0.0, -0.1))
    assert f.d.shape == (16, 20, 24) and f.d.dtype == np.float32
    X, Y, Z = f.nodes()
    assert X[0, 0, 5] == pytest.approx(0.25) and Y[0, 3, 0] == pytest.approx(0.15) and Z[2, 0, 0] == pytest.approx(0.0)
    assert f.d[4, 6, 6] == pytest.approx(-0.1, abs=1e-6)      # (0.3, 0.3, 0.1): 0.1 m inside, nearest face x or z
    assert f.d[4, 6, 12] == pytest.approx(0.2, abs=1e-6)      # (0.6, 0.3, 0.1): 0.2 m off the x = 0.4 face
    g = DistanceField.from_function(lambda X, Y, Z: X + 2 * Y + 3 * Z, (3, 4, 5), 0.5)
    assert g.d.shape == (5, 4, 3) and g.d[4, 3, 2] == 1.0 + 3.0 + 6.0
    with pytest.raises(ValueError):
        DistanceField(FO.DIMS, FO.VOXEL, d=np.zeros((24, 20, 16), np.float32))   # (nx, ny, nz) order is refused
    c = f.to_c()
    assert list(c.dims) == [24, 20, 16] and c.voxel == np.float32(0.05)


class _FakeEngine:
    made = []

    def __init__(self, cfg, scene=None, field=None):
        self.cfg, self.scene, self.field, self.calls = cfg, scene, field, []
        _FakeEngine.made.append(self)

    def set_u_prev(self, u):
        pass

    def set_distance_field(self, d, origin=None):
        self.calls.append(("set", d, origin))

    def clear_distance_field(self):
        self.calls.append(("clear",))


def test_dropin_field_plumbing(monkeypatch):
    from quadrotor_manipulator_mppi_amd.mppi_solver import _base
    from quadrotor_manipulator_mppi_amd.mppi_solver.drone_mppi import MPPI as Drone
    monkeypatch.setattr(_base, "Engine", _FakeEngine)
    _FakeEngine.made.clear()
    f = DistanceField.from_function(lambda X, Y, Z: Z - 0.2, FO.DIMS, FO.VOXEL)
    s = Drone(n_samples=64, n_timestep=32, field=f)
    e = s._ensure_engine((False, 64, 32))
    assert e.field is f and e.scene is None          # (Engine itself takes Scene.default for a field without a scene)
    s._sync_obstacles(e)
    assert e.calls[-1][0] == "set" and e.calls[-1][1] is f.d and len(e.calls) == 1
    s._sync_obstacles(e)
    assert len(e.calls) == 1                          # unchanged: not sent again
    s.set_distance_field(f.d + 1.0, origin=(1.0, 2.0, 3.0))
    s._sync_obstacles(e)
    assert e.calls[-1][0] == "set" and np.array_equal(e.calls[-1][2], np.float32([1, 2, 3]))
    s.clear_distance_field()
    s._sync_obstacles(e)
    assert e.calls[-1] == ("clear",)
    plain = Drone(n_samples=64, n_timestep=32)
    with pytest.raises(RuntimeError):
        plain.set_distance_field(f.d)
    with pytest.raises(RuntimeError):
        plain.clear_distance_field()
    with pytest.raises(ValueError):
        s.set_distance_field(np.zeros((2, 2, 2), np.float32))


def test_oracle_placement_meets_its_conditions(monkeypatch):
    """The GPU file's arm case, on the CPU alone: a third of the samples carry the field term and each
    of the five mistakes shows at more than 100 x the tolerance (the GPU tests assert the same first)."""
    import torch
    import test_gpu_distance_field as TF
    c = TF._arm_case(monkeypatch, "f64-h32")
    ref = c["step"]()
    FO.assert_case_can_fail(c["step"], ref, what="arm f64-h32 (CPU)")
    assert torch.isfinite(ref["S"]).all()
