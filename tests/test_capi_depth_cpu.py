"""Depth images into the occupancy map (mppi_integrate_depth, mppi_shift_map, mppi_get_occupancy,
mppi_depth_integrate_host; csrc/mppi_depth.hip, csrc/mppi_depth.h), without a GPU: the float64 oracle
(tests/depth_oracle.py) stays inside its cap on its own and catches each planted mistake; the host twin
meets the oracle's rule on the whole case list, is idempotent, and sequences frames as specified; the
refusals carry their messages; the struct is 80 bytes and the ABI version unchanged; the three kernels are
in the new unit's code object; the window move equals a numpy slice-and-zero-fill; the wire decoders
round-trip and refuse what they must; the classes refuse map calls without a field.
"""
import ctypes as C

import numpy as np
import pytest

import depth_oracle as DO
from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd import build as B
from quadrotor_manipulator_mppi_amd.engine import DepthView, DistanceField, depth_integrate_host

UNIT = "mppi_depth.hip"
IDS = [c.name for c in DO.CASES]


def view_of(case, **over):
    kw = dict(vars(case.view))
    kw.update(over)
    return DepthView(**kw)


def field_of(case):
    return DistanceField(case.field.dims, case.field.voxel, case.field.origin)


def host(case, before, **over):
    return depth_integrate_host(field_of(case), before, case.depth, view_of(case, **over))


@pytest.fixture(scope="module")
def oracle():
    """The four sets of every case, computed once."""
    return {c.name: DO.integrate(c) for c in DO.CASES}


# ================================================================================ the oracle on its own
def test_the_tolerance_is_the_derived_one():
    c = DO.CASES[0]
    assert 0.5e-4 < DO.tol_u(c) < 2e-4, "coordinates up to 4 m at voxel 0.05: about 1e-4 voxels"
    assert all(DO.tol_u(k) < 2e-3 for k in DO.CASES)


@pytest.mark.parametrize("case", DO.CASES, ids=IDS)
def test_the_oracle_stays_inside_its_cap(oracle, case):
    s = oracle[case.name]
    f, o = DO.undecided(s)
    print(case.name, f"tol_u {DO.tol_u(case):.3g}; undecided F {f:.4f} of {int(s['F_possible'].sum())}, O {o:.4f} of {int(s['O_possible'].sum())}")
    assert f <= DO.CAP and o <= DO.CAP
    if "away" in case.name or "nan" in case.name:
        assert not s["F_possible"].any() and not s["O_possible"].any()
    elif "inf" in case.name:
        assert s["F_certain"].any() and not s["O_possible"].any()
    elif "markonly" in case.name:
        assert not s["F_possible"].any() and s["O_certain"].any()
    else:
        assert s["F_certain"].any() and s["O_certain"].any()


@pytest.mark.parametrize("case", DO.CASES, ids=IDS)
def test_the_float64_model_passes_the_rule(oracle, case):
    before = DO.before_map(case)
    assert DO.check(before, DO.model(case, before), oracle[case.name]) == []


@pytest.mark.parametrize("variant", DO.VARIANTS)
def test_each_planted_mistake_violates_the_rule(oracle, variant):
    caught = []
    for case in DO.CASES:
        before = DO.before_map(case)
        if DO.check(before, DO.model(case, before, variant), oracle[case.name]):
            caught.append(case.name)
    print(variant, "caught on", caught)
    assert caught, variant


# ====================================================================================== the host twin
@pytest.mark.parametrize("case", DO.CASES, ids=IDS)
def test_host_twin_meets_the_oracle_rule(oracle, case):
    before = DO.before_map(case)
    after = host(case, before)
    assert after.dtype == np.uint8 and after.shape == before.shape
    assert DO.check(before, after, oracle[case.name]) == []
    assert np.array_equal(host(case, after), after), "the same frame twice gives the same map"
    if "away" in case.name or "nan" in case.name:
        assert np.array_equal(after, before)
    # into an empty and into a full map
    for fill in (0, 255):
        start = np.full_like(before, fill)
        assert DO.check(start, host(case, start), oracle[case.name]) == []


def test_two_frames_in_sequence():
    """The second frame carves what the first marked where its rays pass, and marks its own end points."""
    a, b = DO.CASES[0], DO.CASES[2]   # the same grid from two poses
    assert a.field.dims == b.field.dims
    empty = np.zeros(a.field.dims[::-1], np.uint8)
    m1 = host(a, empty)
    m2 = host(b, m1)
    sb = DO.integrate(b)
    assert DO.check(m1, m2, sb) == []
    assert m1.any() and (m2 & ~m1.astype(bool)).any(), "the second frame marks new nodes"
    assert not np.array_equal(host(a, host(b, empty)), m2), "the order of the frames matters"


def test_carve_zero_marks_only():
    case = DO.CASES[0]
    before = DO.before_map(case)
    after = host(case, before, carve=False)
    full = host(case, before)
    assert not (before.astype(bool) & ~after.astype(bool)).any(), "nothing is cleared"
    added = after.astype(bool) & ~before.astype(bool)
    assert added.any() and not (added & ~full.astype(bool)).any(), "the marks are the full frame's marks"
    assert (before.astype(bool) & ~full.astype(bool)).any(), "and the full frame does carve"


def test_a_return_on_z_max_marks_and_a_value_above_it_does_not():
    case = next(c for c in DO.CASES if "zmax" in c.name)
    empty = np.zeros(case.field.dims[::-1], np.uint8)
    on = host(case, empty)
    assert on.any()
    above = depth_integrate_host(field_of(case), empty, np.nextafter(case.depth, np.float32(np.inf)), view_of(case))
    assert not above.any()


def test_hostile_values_form_no_address():
    """NaN, +-inf, negatives and 3e38 in the image, and a pose at 1e30: the call returns and only 0 / 1 come back."""
    case = DO.CASES[3]
    before = DO.before_map(case)
    bad = np.array([np.nan, np.inf, -np.inf, -1.0, 3e38, 0.0, 1.0] * 5, np.float32).reshape(case.depth.shape)
    for over in ({}, {"pos": (1e30, -1e30, 1e30)}, {"pos": (3e38, 3e38, -3e38), "z_max": 200.0}):
        after = depth_integrate_host(field_of(case), before, bad, view_of(case, **over))
        assert np.isin(after, (0, 1)).all()
        if "pos" in over:
            assert np.array_equal(after, before), "a camera that far away reaches nothing"


# ========================================================================================== refusals
def _status(case, view=None, depth=0, occ=0, field=None):
    v = view_of(case).to_c() if view is None else view
    d = case.depth if isinstance(depth, int) else depth
    o = np.zeros(case.field.dims[::-1], np.uint8) if isinstance(occ, int) else occ
    desc = field_of(case).to_c() if field is None else field
    st = capi.lib().mppi_depth_integrate_host(C.byref(desc), None if v is False else C.byref(v), capi.fptr(d),
                                              None if o is None else o.ctypes.data_as(C.POINTER(C.c_uint8)))
    return st, capi.lib().mppi_last_error().decode()


def test_refusals_carry_their_messages():
    case = DO.CASES[3]
    assert _status(case)[0] == capi.OK
    assert _status(case, view=False) == (capi.ERR_INVALID_ARG, "depth: null view")
    assert _status(case, depth=None) == (capi.ERR_INVALID_ARG, "depth: null image")
    st, msg = _status(case, occ=None)
    assert st == capi.ERR_INVALID_ARG and "null map" in msg

    def bad(**kw):
        v = view_of(case).to_c()
        for k, x in kw.items():
            if isinstance(x, tuple):
                getattr(v, k)[x[0]] = x[1]
            else:
                setattr(v, k, x)
        st, msg = _status(case, view=v)
        assert st == capi.ERR_INVALID_ARG, kw
        return msg
    assert "image" in bad(width=0) and "image" in bad(height=-1) and "image" in bad(width=1 << 11, height=1 << 10)
    assert "stride" in bad(stride=0)
    assert "carve" in bad(carve=2)
    for k in ("fx", "fy", "cx", "cy", "z_min", "z_max"):
        assert "non-finite" in bad(**{k: float("nan")}) and "non-finite" in bad(**{k: float("inf")})
    assert "non-finite" in bad(pos=(1, float("inf"))) and "non-finite" in bad(quat_xyzw=(2, float("nan")))
    assert "focal" in bad(fx=0.0) and "focal" in bad(fy=-1.0)
    assert "z range" in bad(z_min=-0.1) and "z range" in bad(z_min=2.0, z_max=2.0)
    assert "z range" in bad(z_max=4097.0 * case.field.voxel)
    v = view_of(case).to_c()
    v.z_max = 4096.0 * case.field.voxel * 0.999
    assert _status(case, view=v)[0] == capi.OK
    v = view_of(case).to_c()
    for i in range(4):
        v.quat_xyzw[i] *= 0.5     # squared norm 1.5625 / 4
    assert "quaternion" in _status(case, view=v)[1] and _status(case, view=v)[0] == capi.ERR_INVALID_ARG
    for i in range(4):
        v.quat_xyzw[i] *= 4.0
    assert "quaternion" in _status(case, view=v)[1]
    for i in range(3):
        assert "reserved" in bad(reserved=(i, 1))
    desc = field_of(case).to_c()
    desc.dims[0] = 513
    assert _status(case, field=desc)[0] == capi.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        depth_integrate_host(field_of(case), np.zeros(case.field.dims[::-1], np.uint8), case.depth[:-1], view_of(case))
    with pytest.raises(TypeError):
        depth_integrate_host(field_of(case), np.zeros(case.field.dims[::-1], np.float32), case.depth, view_of(case))


def test_a_scaled_quaternion_is_normalised():
    case = DO.CASES[3]
    before = DO.before_map(case)
    q = np.asarray(case.view.quat_xyzw)
    assert abs(float(q @ q) - 1.5625) < 1e-6
    a = host(case, before)
    b = host(case, before, quat_xyzw=tuple(q / np.linalg.norm(q)))
    assert DO.check(before, b, DO.integrate(case)) == [] and np.mean(a != b) < 0.01


# ============================================================================== the structs, the unit
def test_struct_size_and_abi():
    assert C.sizeof(capi.DepthViewC) == 80
    assert capi.lib().mppi_abi_version() == capi.ABI_VERSION == 10
    assert capi.DEPTH_MAX_PIXELS == 1 << 20 and capi.DEPTH_MAX_SAMPLES == 16384
    # no other struct changed
    assert (C.sizeof(capi.FieldDesc), C.sizeof(capi.Stats), C.sizeof(capi.Joint), C.sizeof(capi.BodySphere)) == (32, 24, 48, 20)
    assert (C.sizeof(capi.Config), C.sizeof(capi.Scene), C.sizeof(capi.SelfCollision)) == (2168, 336, 276)
    sizes = [C.c_int32() for _ in range(3)]
    capi.lib().mppi_struct_sizes(*[C.byref(s) for s in sizes])
    assert [s.value for s in sizes] == [C.sizeof(capi.Config), C.sizeof(capi.Joint), C.sizeof(capi.Stats)]
    for name in ("mppi_integrate_depth", "mppi_shift_map", "mppi_get_occupancy", "mppi_depth_integrate_host"):
        assert name in capi.PROTOTYPES and hasattr(capi.lib(), name)


def test_the_kernels_are_in_the_new_unit():
    assert UNIT in B.KERNEL_UNITS
    res = B.kernel_resources(B.code_object_path(B.LIB, UNIT))
    names = sorted(res)
    print({k: res[k] for k in names})
    assert len(names) == 3
    for kern, sig in (("k_depth_carve", "N4mppi11DepthParamsE"), ("k_depth_mark", "N4mppi11DepthParamsE"),
                      ("k_map_shift", "N4mppi11ShiftParamsE")):
        sym = f"_Z{len(kern)}{kern}{sig}"
        assert sym in res, (sym, names)
        assert res[sym]["scratch"] == 0 and res[sym]["lds"] == 0 and res[sym]["vspill"] == 0
        others = [u for u in B.KERNEL_UNITS if u != UNIT and (sym + ".kd").encode() in open(B.code_object_path(B.LIB, u), "rb").read()]
        assert others == []


# ===================================================================================== the window move
def _shift(dims, occ, shift, origin=(0.25, -0.5, 1.0), voxel=0.05):
    f = capi.lib().mppi_debug_map_shift
    f.restype, f.argtypes = capi.DEBUG_PROTOTYPES["mppi_debug_map_shift"]
    desc = DistanceField(dims, voxel, origin).to_c()
    out, o = np.full(occ.shape, 7, np.uint8), np.empty(3, np.float32)
    st = f(C.byref(desc), (C.c_int32 * 3)(*shift), occ.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(C.POINTER(C.c_uint8)), capi.fptr(o))
    return st, out, o


@pytest.mark.parametrize("dims", [(16, 12, 10), (33, 17, 9), (512, 2, 2)], ids=lambda d: "x".join(map(str, d)))
def test_shift_equals_a_numpy_slice_and_zero_fill(dims):
    rng = np.random.default_rng(4)
    occ = (rng.random(dims[::-1]) < 0.3).astype(np.uint8) * rng.integers(1, 256, dims[::-1]).astype(np.uint8)
    for shift in [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, -1), (3, -1, 1), (dims[0] - 1, 0, 0), (dims[0], 0, 0),
                  (0, -dims[1], 0), (2 ** 31 - 1, 0, 0), (0, 0, -2 ** 31)]:
        st, out, o = _shift(dims, occ, shift)
        assert st == capi.OK, shift
        assert np.array_equal(out, DO.shifted(occ != 0, shift).astype(np.uint8)), shift
        want = [np.float32(np.float64(np.float32(s)) * np.float64(np.float32(0.05)) + np.float64(np.float32(x0)))
                for s, x0 in zip(shift, (0.25, -0.5, 1.0))]
        assert np.array_equal(o, np.float32(want)), (shift, o, want)
    assert np.array_equal(_shift(dims, occ, (0, 0, 0))[1], (occ != 0).astype(np.uint8)), "a zero shift changes nothing"
    assert not _shift(dims, occ, (0, dims[1], 0))[1].any(), "|s| >= n clears the map"
    st, _, _ = _shift(dims, occ, (2 ** 31 - 1, 0, 0), voxel=3e37)
    assert st == capi.ERR_INVALID_ARG and "origin" in capi.lib().mppi_last_error().decode()


# ============================================================================================ the wire
def test_wire_decoders_round_trip():
    from quadrotor_manipulator_mppi_amd.mppi_solver import wire as W
    d = DO.CASES[3].depth
    h, w = d.shape
    img = W.Image(W.Header(7, 12, 34, "camera_depth_optical_frame"), h, w, "32FC1", 0, 4 * w + 8,
                  b"".join(r.tobytes() + b"\xAA" * 8 for r in d))
    back = W.Image.deserialize(img.serialize())
    assert back == img
    assert np.array_equal(W.depth_from_image(back).view(np.uint32), d.view(np.uint32)), "row padding dropped, bits kept"
    mm = np.array([[0, 1000, 65535], [1, 250, 0]], np.uint16)
    got = W.depth_from_image(W.Image(W.Header(), 2, 3, "16UC1", 0, 6, mm.tobytes()))
    assert got.dtype == np.float32 and np.isnan(got[0, 0]) and np.isnan(got[1, 2])
    assert np.array_equal(got[~np.isnan(got)], (np.float32([1000, 65535, 1, 250]) * np.float32(1e-3)))
    K = [554.25, 0.0, 320.5, 0.0, 554.25, 240.5, 0.0, 0.0, 1.0]
    ci = W.CameraInfo(W.Header(1, 2, 3, "f"), 480, 640, "plumb_bob", np.zeros(5), np.array(K), np.eye(3).ravel(),
                      np.arange(12.0), 1, 2, (3, 4, 5, 6, True))
    cb = W.CameraInfo.deserialize(ci.serialize())
    assert (cb.header, cb.height, cb.width, cb.distortion_model, cb.binning_x, cb.binning_y, cb.roi) == \
        (ci.header, 480, 640, "plumb_bob", 1, 2, (3, 4, 5, 6, True))
    for a, b in ((cb.D, ci.D), (cb.K, ci.K), (cb.R, ci.R), (cb.P, ci.P)):
        assert np.array_equal(a, b)
    v = DepthView.from_camera_info(cb.K, cb.width, cb.height, z_max=4.0, stride=2)
    assert (v.fx, v.fy, v.cx, v.cy, v.width, v.height, v.stride, v.z_max) == (554.25, 554.25, 320.5, 240.5, 640, 480, 2, 4.0)
    assert C.sizeof(v.to_c()) == 80 and v.to_c().carve == 1


def test_wire_refusals():
    from quadrotor_manipulator_mppi_amd.mppi_solver import wire as W
    ok = W.Image(W.Header(), 2, 3, "32FC1", 0, 12, bytes(24))
    assert W.depth_from_image(ok).shape == (2, 3)
    for bad in (W.Image(W.Header(), 2, 3, "rgb8", 0, 9, bytes(18)), W.Image(W.Header(), 2, 3, "32FC1", 1, 12, bytes(24)),
                W.Image(W.Header(), 2, 3, "32FC1", 0, 12, bytes(23)), W.Image(W.Header(), 2, 3, "16UC1", 0, 4, bytes(24)),
                W.Image(W.Header(), 0, 3, "32FC1", 0, 12, b"")):
        with pytest.raises(W.WireError):
            W.depth_from_image(bad)
    buf = ok.serialize()
    for cut in (buf[:-1], buf + b"\0", buf[:10]):
        with pytest.raises(W.WireError):
            W.Image.deserialize(cut)
    with pytest.raises(W.WireError):
        W.CameraInfo.deserialize(W.CameraInfo().serialize()[:-1])
    with pytest.raises(W.WireError):
        W.CameraInfo(K=np.zeros(8)).serialize()


# ========================================================================================= the classes
def test_class_methods_raise_without_a_field():
    from quadrotor_manipulator_mppi_amd.mppi_solver._base import SolverBase
    s = SolverBase.__new__(SolverBase)
    v = view_of(DO.CASES[3])
    for call in (lambda: s.integrate_depth(DO.CASES[3].depth, v), lambda: s.shift_map((1, 0, 0)), lambda: s.get_occupancy()):
        with pytest.raises(RuntimeError, match="field="):
            call()
    from quadrotor_manipulator_mppi_amd import distributed as D
    for name in ("integrate_depth", "shift_map", "get_occupancy"):
        assert any(hasattr(cls, name) and hasattr(cls, "set_occupancy") for cls in vars(D).values() if isinstance(cls, type)), name
