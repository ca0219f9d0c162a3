"""GPU tests of depth images into the occupancy map (mppi_integrate_depth, mppi_shift_map, mppi_get_occupancy;
csrc/mppi_depth.hip): the device's carve and mark passes, the window move, their hand-over to the transform
and their ordering with the step.  Engines are model="arm", K = 64, H = 32, injected noise, as in
test_gpu_occupancy.py.

A. the case list (depth_oracle.CASES: grids (16,12,10), (33,17,9), (48,40,32), (512,2,2); images 1x1, 7x5,
   64x48; stride 1 and 3; the camera inside the grid, outside looking in, looking away; all-NaN, all-+inf
   and a return exactly on z_max; mark only): get_occupancy() equals the host twin with np.array_equal and
   passes the oracle's rule, and get_distance_field() equals mppi_occupancy_field of that map bit for bit.
B. through the step: one engine integrates six frames rendered from a placed map (test_gpu_distance_field's
   slab and blob, seen from the six sides), a twin is given set_occupancy(first.get_occupancy()); both step
   to bit-equal S and clearances.  Asserted on tests/field_oracle.py first: a third of the samples carry a
   nonzero field term under the integrated map's field.
C. sequences, all equal to the host replay: two frames from two poses, set_occupancy then a frame,
   shift_map then a frame, a frame followed at once by run_steps(3) on either dispatch path.
D. hostile values inside a valid view: NaN, +-inf, negatives and 3e38 in the image and a pose at 1e30 --
   values a sensor really delivers, which by the definition form no address; the map equals the host
   twin's and the next step is finite.
E. the getters' and setters' statuses on engines without a field.
F. the drop-in route: map calls made on the arm solver class before its first control call run behind it, a
   refused call is not queued and the next good one goes through, and the map survives an engine change.
"""
import ctypes as C

import numpy as np
import pytest

import depth_oracle as DO
import field_oracle as FO
import obstacle_oracle as OO
import test_gpu_distance_field as TD
import test_gpu_obstacles as TG
import test_gpu_occupancy as TOC
import tracking_oracle as TO
from test_capi_depth_cpu import field_of, host, view_of

pytestmark = pytest.mark.gpu

IDS = [c.name for c in DO.CASES]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _field_of_map(occ, dims, voxel, origin, max_dist=None):
    from quadrotor_manipulator_mppi_amd.engine import DistanceField
    return DistanceField.from_occupancy(occ, dims, voxel, tuple(float(x) for x in origin), max_dist).d


# ================================================================================ A. the case list
@pytest.fixture(scope="module")
def engines():
    """One small field engine per (grid, voxel) of the list, made at first use."""
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    made = {}

    def get(case):
        key = (case.field.dims, case.field.voxel)
        if key not in made:
            made[key] = Engine(make_config(model="arm", n_samples=64, n_horizon=32, noise="injected"),
                               scene=TG._scene(OO.SceneSpec(TG.ARM_BODY)), field=field_of(case))
        return made[key]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def oracle():
    return {c.name: DO.integrate(c) for c in DO.CASES}


@pytest.mark.parametrize("case", DO.CASES, ids=IDS)
def test_device_map_matches_host_and_oracle(engines, oracle, case):
    e = engines(case)
    before = DO.before_map(case)
    want = host(case, before)
    f, o = DO.undecided(oracle[case.name])
    print(case.name, f"undecided F {f:.4f} O {o:.4f}; host: {int(before.sum())} -> {int(want.sum())} occupied nodes")
    assert DO.check(before, want, oracle[case.name]) == []
    for max_dist in (None, 3.5 * case.field.voxel):
        e.set_occupancy(before * 255, origin=case.field.origin)
        e.integrate_depth(case.depth, view_of(case), max_dist=max_dist)
        got = e.get_occupancy()
        assert got.dtype == np.uint8 and np.array_equal(got, want), case.name + ": device map vs the host twin"
        assert DO.check(before, got, oracle[case.name]) == []
        d, origin = e.get_distance_field()
        assert np.array_equal(origin, np.float32(case.field.origin))
        ref = _field_of_map(got, case.field.dims, case.field.voxel, case.field.origin, max_dist)
        assert np.array_equal(_bits(d), _bits(ref)), case.name + ": the field of the map, bit for bit"
    e.integrate_depth(case.depth, view_of(case))   # the same frame again: the same map
    assert np.array_equal(e.get_occupancy(), want)


# ==================================================================== B. equivalence through the step
def _render(occ, dims, voxel, origin, view):
    """A depth image of the map occ seen through `view`, by a float64 march (a test input, not a reference)."""
    R = DO.quat_R(view.quat_xyzw)
    jj, ii = np.meshgrid(np.arange(view.height), np.arange(view.width), indexing="ij")
    ray = np.stack([(ii - view.cx) / view.fx, (jj - view.cy) / view.fy, np.ones(ii.shape)], -1) @ R.T
    depth = np.full(ii.shape, np.inf, np.float32)
    for z in np.arange(view.z_max - 1e-3, view.z_min, -0.2 * voxel):   # far to near: the nearest hit stays
        u = (np.asarray(view.pos) + z * ray - np.asarray(origin, np.float64)) / voxel
        n = np.floor(u + 0.5).astype(int)
        inside = np.all((n >= 0) & (n < np.asarray(dims)), axis=-1)
        hit = np.zeros(ii.shape, bool)
        hit[inside] = occ[n[inside][:, 2], n[inside][:, 1], n[inside][:, 0]] != 0
        depth[hit] = z
    return depth


def _six_views(dims, voxel, origin):
    from quadrotor_manipulator_mppi_amd.engine import DepthView
    centre = np.asarray(origin, np.float64) + 0.5 * voxel * (np.asarray(dims) - 1)
    views = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            away = np.zeros(3)
            away[axis] = sign
            pos = centre + away * (0.5 * voxel * dims[axis] + 0.9) + 0.013 * np.array([1.0, -2.0, 3.0])
            fwd = centre - pos + np.array([0.011, 0.017, 0.007])
            up = (0.0, 0.0, 1.0) if axis != 2 else (0.0, 1.0, 0.0)
            views.append(DepthView(64, 48, 44.0, 44.0, 31.7, 23.6, tuple(pos), tuple(DO.look_at(fwd, up)), 0.2, 2.6, 1, True))
    return views


def test_step_equals_the_map_handed_over(monkeypatch):
    from quadrotor_manipulator_mppi_amd.engine import depth_integrate_host
    c, occ, _ = TOC._occupancy_case(monkeypatch)
    fld0 = c["field"]
    dims, voxel, origin = fld0.dims, fld0.voxel, tuple(float(x) for x in fld0.origin)
    desc = TD._desc(fld0)
    views = _six_views(dims, voxel, origin)
    frames = [_render(occ, dims, voxel, origin, v) for v in views]
    # ---- on the host and the oracle, before the GPU
    m = np.zeros(dims[::-1], np.uint8)
    for v, img in zip(views, frames):
        m = depth_integrate_host(desc, m, img, v)
    fld = FO.Field(dims, voxel, fld0.origin, _field_of_map(m, dims, voxel, origin))
    ob = FO.term(c["frames"], c["spec"], TD.NO_OBS, fld, 0.01, TO.TOL_EE)
    frac = float(np.mean(ob["S_field"] > 0.0))
    print(f"depth step: {int(m.sum())} of {int(occ.sum())} occupied nodes seen; {100 * frac:.0f}% of the samples carry a "
          "nonzero field term (need 33%)")
    assert m.any() and not (m.astype(bool) & ~occ).any(), "every marked node is a node of the placed map"
    assert frac >= 1.0 / 3.0
    # ---- the device
    a, b = TD._engine(c["spec"], fld0, **c["eng"]), TD._engine(c["spec"], fld0, **c["eng"])
    TG._arm_target(c, a)
    for v, img in zip(views, frames):
        a.integrate_depth(img, v)
    a.set_u_prev(c["u"].numpy())
    _, _, st = a.step(TD.ARM_STATE, c["noise"].numpy()[None])
    assert not st[0].nonfinite
    got = a.get_occupancy()
    assert np.array_equal(got, m), "six frames: device map vs the host replay"
    TG._arm_target(c, b)
    b.set_occupancy(got)
    b.set_u_prev(c["u"].numpy())
    b.step(TD.ARM_STATE, c["noise"].numpy()[None])
    Sa, Sb = a.get_costs()[0], b.get_costs()[0]
    assert np.array_equal(_bits(Sa), _bits(Sb)), "S: the integrating engine vs its map handed over"
    assert np.array_equal(_bits(a.get_clearances()[0]), _bits(b.get_clearances()[0]))
    assert np.array_equal(_bits(a.get_distance_field()[0]), _bits(fld.d))
    ref = c["step"](None, fld)   # and the term is the oracle's for that field
    TG._close_S(Sa, ref, "depth step")
    a.close()
    b.close()


# ================================================================================== C. sequences
def test_sequences_equal_the_host_replay(engines):
    from quadrotor_manipulator_mppi_amd.engine import DistanceField, depth_integrate_host
    a, b = DO.CASES[0], DO.CASES[2]   # the same grid from two poses
    e = engines(a)
    dims, voxel, origin = a.field.dims, a.field.voxel, a.field.origin
    empty = np.zeros(dims[::-1], np.uint8)
    # ---- two frames from two poses
    e.set_occupancy(empty, origin=origin)
    e.integrate_depth(a.depth, view_of(a))
    e.integrate_depth(b.depth, view_of(b))
    want = host(b, host(a, empty))
    assert np.array_equal(e.get_occupancy(), want) and want.any()
    # ---- set_occupancy then a frame
    seed = DO.before_map(a, seed=9, share=0.2)
    e.set_occupancy(seed)
    e.integrate_depth(b.depth, view_of(b), max_dist=0.3)
    want = host(b, seed)
    assert np.array_equal(e.get_occupancy(), want)
    assert np.array_equal(_bits(e.get_distance_field()[0]), _bits(_field_of_map(want, dims, voxel, origin, 0.3)))
    # ---- set_distance_field and a clear leave the map alone
    e.set_distance_field(np.ones(dims[::-1], np.float32))
    e.clear_distance_field()
    assert e.get_distance_field() is None and np.array_equal(e.get_occupancy(), want)
    # ---- shift_map then a frame: the window and the origin move, the frame lands in the moved grid
    shift = (3, -2, 1)
    e.shift_map(shift)
    moved = DO.shifted(want, shift)
    assert np.array_equal(e.get_occupancy(), moved)
    new_origin = np.float32([np.float32(np.float64(np.float32(s)) * np.float64(np.float32(voxel)) + np.float64(np.float32(o)))
                             for s, o in zip(shift, origin)])
    d, o = e.get_distance_field()
    assert np.array_equal(o, new_origin)
    assert np.array_equal(_bits(d), _bits(_field_of_map(moved, dims, voxel, new_origin)))
    e.integrate_depth(a.depth, view_of(a))
    want = depth_integrate_host(DistanceField(dims, voxel, tuple(float(x) for x in new_origin)), moved, a.depth, view_of(a))
    assert np.array_equal(e.get_occupancy(), want) and not np.array_equal(want, host(a, moved)), "the moved origin is used"
    e.shift_map((0, 0, 0))
    assert np.array_equal(e.get_occupancy(), want), "a zero shift changes nothing"
    e.shift_map((0, dims[1], 0))
    assert not e.get_occupancy().any(), "|s| >= n clears the map"
    e.set_occupancy(empty, origin=origin)


def _frame_for(origin):
    """A 64x48 frame of test_gpu_occupancy's first map, seen from outside the grid's -x face, and that map
    with clutter in its free space for the frame to carve."""
    from quadrotor_manipulator_mppi_amd.engine import DepthView
    first, _ = TOC._maps(origin)
    pos = np.asarray(origin) + np.array([-0.613, 0.5 * FO.VOXEL * FO.DIMS[1] + 0.021, 0.5 * FO.VOXEL * FO.DIMS[2] + 0.033])
    view = DepthView(64, 48, 40.0, 40.0, 31.6, 23.7, tuple(pos), tuple(DO.look_at((1.0, 0.02, -0.05))), 0.2, 2.4, 1, True)
    clutter = np.random.default_rng(12).random(first.shape) < 0.1
    return view, _render(first, FO.DIMS, FO.VOXEL, origin, view), (first | clutter).astype(np.uint8)


@pytest.mark.parametrize("mode", ["aql", "hip"])
def test_integrate_depth_is_ordered_before_the_next_batch(monkeypatch, mode):
    """A frame followed at once by run_steps(3) ends on the bits of a synchronise placed between them, and
    on the bits of an engine that was handed the resulting map."""
    from quadrotor_manipulator_mppi_amd.engine import DistanceField, depth_integrate_host
    got = {}
    for sync_between in (False, True):
        e, origin = TOC._philox_engine(monkeypatch, mode)
        view, img, first = _frame_for(origin)
        e.set_occupancy(first)
        e.integrate_depth(img, view)
        if sync_between:
            e.synchronize()
        e.run_steps(3)
        e.synchronize()
        got[sync_between] = TOC._bits(e)
        want = depth_integrate_host(DistanceField(FO.DIMS, FO.VOXEL, origin), first, img, view)
        assert np.array_equal(e.get_occupancy(), want) and int((want != first).sum()) > 100, "the frame carved the clutter"
        if sync_between:
            e2, _ = TOC._philox_engine(monkeypatch, mode)
            e2.set_occupancy(want)
            e2.run_steps(3)
            e2.synchronize()
            for x, y in zip(TOC._bits(e2), got[True]):
                assert np.array_equal(x, y), "the integrated map's field is the one the steps met"
            e3, _ = TOC._philox_engine(monkeypatch, mode)
            e3.set_occupancy(first)
            e3.run_steps(3)
            e3.synchronize()
            assert not np.array_equal(TOC._bits(e3)[0], got[True][0]), "the frame shows in the costs"
            e2.close()
            e3.close()
        e.close()
    for x, y in zip(got[False], got[True]):
        assert np.array_equal(x, y), mode


# ================================================================ D. hostile values in a valid view
def test_hostile_values_form_no_address(engines):
    case = DO.CASES[0]
    e = engines(case)
    before = DO.before_map(case)
    h, w = case.depth.shape
    vals = np.array([np.nan, np.inf, -np.inf, -1.0, 3e38, 0.0, 1.0, 1.7], np.float32)
    bad = vals[(np.arange(h * w) * 5 + 3) % len(vals)].reshape(h, w)
    for over in ({}, {"pos": (1e30, -1e30, 1e30)}, {"pos": (case.view.pos[0], 1e30, case.view.pos[2])}):
        e.set_occupancy(before, origin=case.field.origin)
        e.integrate_depth(bad, view_of(case, **over))
        got = e.get_occupancy()
        assert np.array_equal(got, host_bad(case, before, bad, over)), over
        if over:
            assert np.array_equal(got, before), "a camera that far away reaches nothing"
        else:
            assert not np.array_equal(got, before), "the finite values carve and mark"
    e.set_target(TO.TPOS, TO.TQUAT)
    _, _, st = e.step(TG.ARM_STATE, np.zeros((1, 64, 32, 7), np.float32))
    assert not st[0].nonfinite and np.isfinite(e.get_costs()).all() and np.isfinite(e.get_clearances()).all()
    e.set_occupancy(np.zeros_like(before), origin=case.field.origin)


def host_bad(case, before, bad, over):
    from quadrotor_manipulator_mppi_amd.engine import depth_integrate_host
    return depth_integrate_host(field_of(case), before, bad, view_of(case, **over))


# ================================================================== E. engines without a field
def test_engines_without_a_field_refuse():
    from quadrotor_manipulator_mppi_amd import _capi as capi
    case = DO.CASES[3]
    v = view_of(case)
    spec = OO.SceneSpec(TG.ARM_BODY)
    L = capi.lib()
    occ = np.zeros(case.field.dims[::-1], np.uint8)
    for e in (TG._engine(spec, model="arm", n_samples=64, n_horizon=32), TG._engine(None, model="arm", n_samples=64, n_horizon=32)):
        for call in (lambda: e.integrate_depth(case.depth, v), lambda: e.shift_map((1, 0, 0)), lambda: e.get_occupancy()):
            with pytest.raises(RuntimeError):
                call()
        vc = v.to_c()
        assert L.mppi_integrate_depth(e._h, C.byref(vc), capi.fptr(case.depth), 0.0) == capi.ERR_STATE
        assert L.mppi_shift_map(e._h, (C.c_int32 * 3)(1, 0, 0), 0.0) == capi.ERR_STATE
        assert L.mppi_get_occupancy(e._h, occ.ctypes.data_as(C.POINTER(C.c_uint8))) == capi.ERR_STATE
        e.close()
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    f = Engine(make_config(model="arm", n_samples=64, n_horizon=32, noise="injected"), scene=TG._scene(spec), field=field_of(case))
    assert not f.get_occupancy().any() and f.get_distance_field() is None, "all free before the first map call"
    vc = v.to_c()
    assert L.mppi_integrate_depth(f._h, None, capi.fptr(case.depth), 0.0) == capi.ERR_INVALID_ARG
    assert L.mppi_integrate_depth(f._h, C.byref(vc), None, 0.0) == capi.ERR_INVALID_ARG
    assert L.mppi_integrate_depth(f._h, C.byref(vc), capi.fptr(case.depth), float("nan")) == capi.ERR_INVALID_ARG
    assert L.mppi_integrate_depth(f._h, C.byref(vc), capi.fptr(case.depth), float("inf")) == capi.ERR_INVALID_ARG
    vc.fx = 0.0
    assert L.mppi_integrate_depth(f._h, C.byref(vc), capi.fptr(case.depth), 0.0) == capi.ERR_INVALID_ARG
    assert L.mppi_shift_map(f._h, None, 0.0) == capi.ERR_INVALID_ARG
    assert L.mppi_shift_map(f._h, (C.c_int32 * 3)(1, 0, 0), float("nan")) == capi.ERR_INVALID_ARG
    assert L.mppi_get_occupancy(f._h, None) == capi.ERR_INVALID_ARG
    assert not f.get_occupancy().any() and f.get_distance_field() is None, "the refused calls changed nothing"
    with pytest.raises(ValueError):
        f.integrate_depth(case.depth[:-1], v)
    # the first map call on a fresh engine: the map starts all free
    f.integrate_depth(case.depth, v)
    assert np.array_equal(f.get_occupancy(), host(case, occ)) and f.get_distance_field() is not None
    f.close()


# ================================================================================ F. the drop-in route
def test_solver_route_queues_refuses_and_hands_the_map_over():
    from quadrotor_manipulator_mppi_amd import _capi as capi
    from quadrotor_manipulator_mppi_amd.engine import DistanceField, depth_integrate_host
    from quadrotor_manipulator_mppi_amd.mppi_solver.mppi import MPPI
    case = DO.CASES[0]
    v = view_of(case)
    dims, voxel, origin = case.field.dims, case.field.voxel, case.field.origin
    s = MPPI(n_samples=64, n_horizon=32, verbose=False, field=field_of(case))
    seed = DO.before_map(case)
    s.set_occupancy(seed)
    s.integrate_depth(case.depth, v, max_dist=0.4)            # before the engine exists
    with pytest.raises(capi.MPPIError):
        s.integrate_depth(case.depth, view_of(case, fx=0.0))   # a camera that is not up yet: K all zero
    s.shift_map((2, -1, 0), max_dist=0.4)
    assert s.get_occupancy() is None
    q = np.array([0, 0, 1, 0, 0, 0, 1, 1.57, 1.7, 0, 4.4, 0, 4.71, 0.0])
    s.update_joint(q.astype(np.float32), np.zeros(13, np.float32))
    s.compute_control_input()
    want = DO.shifted(host(case, seed), (2, -1, 0))
    new_origin = np.float32([np.float32(np.float64(np.float32(k)) * np.float64(np.float32(voxel)) + np.float64(np.float32(o)))
                             for k, o in zip((2, -1, 0), origin)])
    assert np.array_equal(s.get_occupancy(), want)
    d, o = s.get_distance_field()
    assert np.array_equal(o, new_origin) and np.array_equal(_bits(d), _bits(_field_of_map(want, dims, voxel, new_origin, 0.4)))
    s.compute_control_input()
    assert np.array_equal(s.get_occupancy(), want), "no op runs twice"
    first = s._engine
    s.update_joint(q, np.zeros(13))   # a float64 state: another engine
    s.compute_control_input()
    assert s._engine is not first
    assert np.array_equal(s.get_occupancy(), want), "the map survives the engine change"
    d2, o2 = s.get_distance_field()
    assert np.array_equal(o2, new_origin) and np.array_equal(_bits(d2), _bits(d))
    s.integrate_depth(case.depth, v)   # and a frame on the new engine lands in the moved window
    moved = DistanceField(dims, voxel, tuple(float(x) for x in new_origin))
    assert np.array_equal(s.get_occupancy(), depth_integrate_host(moved, want, case.depth, v))
    s._engine.close()
