"""GPU tests of occupancy grids (mppi_set_occupancy, mppi_get_distance_field; csrc/mppi_edt.hip): the
device's distance transform, its hand-over to the field kernels and its ordering with the step.

A. the grid list (occupancy_oracle.DIMS x PATTERNS, each with no cap and with a cap of 3.5 voxels): what
   get_distance_field returns equals the host helper (mppi_occupancy_field) bit for bit and the float64
   oracle (tests/occupancy_oracle.py) within its derived tolerance, and its sign is the occupancy at every
   node; the whole device buffer -- header and both words of every x-pair -- equals the host's packing of
   the host helper's field, and field_sample (the host's mppi_debug_field_sample) agrees over both buffers
   on points between the nodes.  Before a case looks at the GPU it asserts on the oracle alone which of
   the mistakes it can show (the 0.5 offset dropped, the seed sets swapped, an axis' pass skipped, the
   x-pair's second word taken from ix).  "No cap" is max_dist None wherever the oracle can resolve a unit of
   D2 at 100 x its tolerance; a single corner node on the 512-long grids cannot (D2 up to 511^2: the ratio
   is 8), and is capped at 140 voxels instead (occupancy_oracle.uncapped_or), as its docstring derives.
B. equivalence through the step: an arm engine (K = 64, H = 32, injected noise) given set_occupancy(occ)
   and a twin given set_distance_field(get_distance_field()) step to bit-equal S and clearances; the map
   is the sign of test_gpu_distance_field's own placed field (a slab on the hand sphere's path and a blob),
   so that -- asserted on tests/field_oracle.py first -- a third of the samples carry a nonzero field term.
C. ordering: set_occupancy followed at once by run_steps(3) on either dispatch path, a second map set
   right after the first, set_occupancy then clear_distance_field, get_distance_field after
   set_distance_field.
D. engines without a field refuse both calls.
"""
import ctypes as C

import numpy as np
import pytest

import field_oracle as FO
import obstacle_oracle as OO
import occupancy_oracle as OC
import test_gpu_distance_field as TD
import test_gpu_obstacles as TG
import tracking_oracle as TO
from test_capi_occupancy_cpu import check_against_oracle

pytestmark = pytest.mark.gpu

VOXEL = OC.VOXEL
ORIGIN = (0.25, -0.5, 1.0)


# ================================================================================ A. the grid list
@pytest.fixture(scope="module")
def engines():
    """One small field engine per grid of the list, made at first use."""
    from quadrotor_manipulator_mppi_amd.engine import DistanceField, Engine, make_config
    made = {}

    def get(dims):
        if dims not in made:
            made[dims] = Engine(make_config(model="arm", n_samples=64, n_horizon=32, noise="injected"),
                                scene=TG._scene(OO.SceneSpec(TG.ARM_BODY)), field=DistanceField(dims, VOXEL, ORIGIN))
        return made[dims]
    yield get
    for e in made.values():
        e.close()


def _device_words(e):
    from quadrotor_manipulator_mppi_amd import _capi as capi
    f = capi.lib().mppi_debug_field_words
    f.restype, f.argtypes = capi.DEBUG_PROTOTYPES["mppi_debug_field_words"]
    words = np.empty(16 + 2 * int(np.prod(e.field.dims)), np.float32)
    assert f(e._h, capi.fptr(words)) == 0
    return words


def _host_words(dims, d, origin=ORIGIN, pair_from_ix=False):
    """The host's packing of d (mppi_debug_field_layout); pair_from_ix: the mistake -- both words of a pair from ix."""
    from quadrotor_manipulator_mppi_amd import _capi as capi
    from quadrotor_manipulator_mppi_amd.engine import DistanceField, make_config
    f = capi.lib().mppi_debug_field_layout
    f.restype, f.argtypes = capi.DEBUG_PROTOTYPES["mppi_debug_field_layout"]
    cfg, desc = make_config(model="arm", n_samples=64, n_horizon=32), DistanceField(dims, VOXEL, origin).to_c()
    words = np.empty(16 + 2 * d.size, np.float32)
    assert f(C.byref(cfg), C.byref(desc), None, capi.fptr(np.ascontiguousarray(d, np.float32)), capi.fptr(words)) == 0
    if pair_from_ix:
        words[17::2] = words[16::2]
    return words


def _sample(words, pts):
    from quadrotor_manipulator_mppi_amd import _capi as capi
    f = capi.lib().mppi_debug_field_sample
    f.restype, f.argtypes = capi.DEBUG_PROTOTYPES["mppi_debug_field_sample"]
    pts = np.ascontiguousarray(pts, np.float32)
    val = np.empty(len(pts), np.float32)
    assert f(capi.fptr(words), len(pts), capi.fptr(pts), capi.fptr(val), None) == 0
    return val


def _between_nodes(dims, d, n=4000, seed=5):
    """World points inside the grid, off the nodes (fractions in [0.2, 0.8] of a cell on every axis): n at
    random, and one in each of up to n cells across which the field d changes along x (evenly picked)."""
    rng = np.random.default_rng(seed)
    cell = np.stack([rng.integers(0, dims[a] - 1, n) for a in range(3)], -1)
    izyx = np.argwhere(np.diff(d, axis=2) != 0.0)
    izyx = izyx[:: max(1, len(izyx) // n)][:n]
    along_x = np.minimum(izyx[:, ::-1], np.asarray(dims) - 2)
    cell = np.concatenate([cell, along_x])
    return np.asarray(ORIGIN) + VOXEL * (cell + rng.uniform(0.2, 0.8, (len(cell), 3)))


@pytest.mark.parametrize("dims", OC.DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("name", OC.PATTERNS)
def test_device_field_matches_host_and_oracle(engines, dims, name):
    from quadrotor_manipulator_mppi_amd.engine import DistanceField
    occ = OC.pattern(name, dims)
    for max_dist in (OC.uncapped_or(occ, dims, VOXEL), 3.5 * VOXEL):
        what = f"{dims} {name} max_dist {max_dist}"
        # ---- on the oracle alone: the mistakes this case can show
        ref = OC.field(occ, dims, VOXEL, max_dist)
        host = DistanceField.from_occupancy(occ, dims, VOXEL, ORIGIN, max_dist).d
        pts = _between_nodes(dims, host)
        m = OC.mistakes(ref, VOXEL)
        right, wrong = _sample(_host_words(dims, host), pts), _sample(_host_words(dims, host, pair_from_ix=True), pts)
        m["pair_from_ix"] = float(np.max(np.abs(right.astype(np.float64) - wrong) / (4.0 * OC.EPS * VOXEL * max(dims))))
        print(what, {k: f"{v:.3g}" for k, v in m.items()})
        assert m["swapped"] > OC.RESOLVE, what
        if name not in ("empty", "full"):
            assert m["no_offset"] > OC.RESOLVE, what
        if name in ("corner", "box", "random"):   # (a seed off the planes of every axis, d varying along x)
            assert min(m["skip_x"], m["skip_y"], m["skip_z"], m["pair_from_ix"]) > OC.RESOLVE, what
        # ---- the device
        e = engines(dims)
        e.set_occupancy(occ if name != "checker" else occ.astype(np.uint8) * 255, max_dist=max_dist)
        got = e.get_distance_field()
        assert got is not None
        d, origin = got
        assert d.dtype == np.float32 and d.shape == dims[::-1]
        assert np.array_equal(origin, np.float32(ORIGIN))
        assert np.array_equal(d.view(np.uint32), host.view(np.uint32)), what + ": device vs the host helper, bit for bit"
        check_against_oracle(d, ref, "device " + what)
        words, want = _device_words(e), _host_words(dims, host)
        assert np.array_equal(words.view(np.uint32), want.view(np.uint32)), what + ": header and both words of every x-pair"
        assert np.array_equal(_sample(words, pts).view(np.uint32), right.view(np.uint32)), what


def test_a_moved_origin_goes_with_the_map(engines):
    dims = (33, 20, 24)
    e = engines(dims)
    occ = OC.pattern("box", dims)
    e.set_occupancy(occ, origin=(1.0, 2.0, 3.0))
    d, origin = e.get_distance_field()
    assert np.array_equal(origin, np.float32([1.0, 2.0, 3.0]))
    e.set_occupancy(occ)   # None keeps it
    assert np.array_equal(e.get_distance_field()[1], np.float32([1.0, 2.0, 3.0]))
    e.set_occupancy(occ, origin=ORIGIN)
    assert np.array_equal(e.get_distance_field()[0], d)


# ==================================================================== B. equivalence through the step
def _occupancy_case(monkeypatch):
    """test_gpu_distance_field's arm case with the sign of its placed field as the map."""
    from quadrotor_manipulator_mppi_amd.engine import DistanceField
    c = TD._arm_case(monkeypatch, "f64-h32")
    occ = c["field"].d < 0.0
    host = DistanceField.from_occupancy(occ, c["field"].dims, c["field"].voxel, tuple(float(x) for x in c["field"].origin)).d
    fld = FO.Field(c["field"].dims, c["field"].voxel, c["field"].origin, host)
    return c, occ, fld


def test_step_equals_the_uploaded_field(monkeypatch):
    c, occ, fld = _occupancy_case(monkeypatch)
    # on the oracle, before the GPU: a third of the samples carry a nonzero field term under the map's field
    ob = FO.term(c["frames"], c["spec"], TD.NO_OBS, fld, 0.01, TO.TOL_EE)
    frac = float(np.mean(ob["S_field"] > 0.0))
    print(f"occupancy step: {int(occ.sum())} occupied nodes; {100 * frac:.0f}% of the samples carry a nonzero field term (need 33%)")
    assert occ.any() and frac >= 1.0 / 3.0
    a, b = TD._engine(c["spec"], c["field"], **c["eng"]), TD._engine(c["spec"], c["field"], **c["eng"])
    TG._arm_target(c, a)
    a.set_occupancy(occ)
    a.set_u_prev(c["u"].numpy())
    _, _, st = a.step(TD.ARM_STATE, c["noise"].numpy()[None])
    assert not st[0].nonfinite
    d, origin = a.get_distance_field()
    assert np.array_equal(d.view(np.uint32), fld.d.view(np.uint32))
    TD._run_arm(c, b, field=d, origin=origin)
    Sa, Sb = a.get_costs()[0], b.get_costs()[0]
    assert np.array_equal(Sa.view(np.uint32), Sb.view(np.uint32)), "S: occupancy engine vs its field uploaded"
    assert np.array_equal(a.get_clearances()[0].view(np.uint32), b.get_clearances()[0].view(np.uint32))
    # and the term is the oracle's for that field
    ref = c["step"](None, fld)
    TG._close_S(Sa, ref, "occupancy step")
    TG._check_clr(a, 0, ref, ref["obs"]["tol_clr"], "occupancy step")
    a.close()
    b.close()


# ================================================================================== C. ordering
def _philox_engine(monkeypatch, mode):
    from quadrotor_manipulator_mppi_amd.engine import DistanceField, Engine, make_config
    monkeypatch.setenv("MPPI_DISPATCH", mode)
    origin = (-0.9, -0.3, 0.9)
    e = Engine(make_config(model="arm", n_samples=256, n_horizon=32, seed=11), scene=TG._scene(OO.SceneSpec(TG.ARM_BODY)),
               field=DistanceField(FO.DIMS, FO.VOXEL, origin))
    e.set_target(TO.TPOS, TO.TQUAT)
    e.set_state(TG.ARM_STATE)
    return e, origin


def _maps(origin):
    """Two different maps: a floor 0.15 m up the grid with a box on it; the box alone, elsewhere."""
    from quadrotor_manipulator_mppi_amd.engine import DistanceField
    floor = ((-9.0, -9.0, -9.0), (9.0, 9.0, origin[2] + 0.15))
    box1 = ((origin[0] + 0.2, origin[1] + 0.2, origin[2]), (origin[0] + 0.5, origin[1] + 0.5, origin[2] + 0.5))
    box2 = ((origin[0] + 0.6, origin[1] + 0.4, origin[2] + 0.2), (origin[0] + 0.9, origin[1] + 0.8, origin[2] + 0.6))
    first = DistanceField.from_boxes([floor, box1], FO.DIMS, FO.VOXEL, origin).d < 0.0
    second = DistanceField.from_boxes([box2], FO.DIMS, FO.VOXEL, origin).d < 0.0
    assert first.any() and second.any() and not np.array_equal(first, second)
    return first, second


def _bits(e):
    return tuple(x.copy().view(np.uint32) for x in (e.get_costs()[0], e.get_clearances()[0], e.get_u_prev()[0]))


@pytest.mark.parametrize("mode", ["aql", "hip"])
def test_set_occupancy_is_ordered_before_the_next_batch(monkeypatch, mode):
    """set_occupancy then run_steps(3) with no synchronise between ends on the bits of a synchronise placed
    between them; a second map set right after the first yields the second map's field."""
    from quadrotor_manipulator_mppi_amd.engine import DistanceField
    got = {}
    for sync_between in (False, True):
        e, origin = _philox_engine(monkeypatch, mode)
        first, second = _maps(origin)
        e.set_occupancy(first)
        e.set_occupancy(second)   # (at once: the first transform's scratch and cells are overwritten in stream order)
        if sync_between:
            e.synchronize()
        e.run_steps(3)
        e.synchronize()
        got[sync_between] = _bits(e)
        d, _ = e.get_distance_field()
        want = DistanceField.from_occupancy(second, FO.DIMS, FO.VOXEL, origin).d
        assert np.array_equal(d.view(np.uint32), want.view(np.uint32)), "the second map's field, no stale scratch"
        if sync_between:   # the field is met, and it is the second map that is met
            e2, _ = _philox_engine(monkeypatch, mode)
            e2.set_occupancy(first)
            e2.run_steps(3)
            e2.synchronize()
            assert not np.array_equal(_bits(e2)[0], got[True][0]), "the two maps give different costs"
            e2.close()
        e.close()
    for a, b in zip(got[False], got[True]):
        assert np.array_equal(a, b), mode


def test_clear_after_set_occupancy_gives_the_scene_engine(monkeypatch):
    c, occ, fld = _occupancy_case(monkeypatch)
    scene = TD._engine(c["spec"], None, **c["eng"])
    TD._run_arm(c, scene, field=None)
    e = TD._engine(c["spec"], c["field"], **c["eng"])
    assert e.get_distance_field() is None
    e.set_occupancy(occ)
    TD._run_arm(c, e, field=None)
    assert np.max(np.abs(e.get_costs()[0] - scene.get_costs()[0])) > 1.0, "the map shows"
    e.clear_distance_field()
    assert e.get_distance_field() is None
    TD._run_arm(c, e, field=None)
    assert np.array_equal(e.get_costs()[0].view(np.uint32), scene.get_costs()[0].view(np.uint32))
    assert np.array_equal(e.get_clearances()[0], scene.get_clearances()[0])
    # set_distance_field afterwards, on the same engine: read back bit for bit
    e.set_distance_field(c["field"].d, origin=(0.5, 0.25, -1.0))
    d, origin = e.get_distance_field()
    assert np.array_equal(d.view(np.uint32), c["field"].d.view(np.uint32)) and np.array_equal(origin, np.float32([0.5, 0.25, -1.0]))
    e.set_occupancy(occ, origin=c["field"].origin)   # and the map again after an upload
    assert np.array_equal(e.get_distance_field()[0].view(np.uint32), fld.d.view(np.uint32))
    scene.close()
    e.close()


# ================================================================== D. engines without a field
def test_engines_without_a_field_refuse(monkeypatch):
    from quadrotor_manipulator_mppi_amd import _capi as capi
    spec = OO.SceneSpec(TG.ARM_BODY)
    occ = np.zeros(FO.DIMS[::-1], np.uint8)
    for e in (TG._engine(spec, model="arm", n_samples=64, n_horizon=32), TG._engine(None, model="arm", n_samples=64, n_horizon=32)):
        with pytest.raises(RuntimeError):
            e.set_occupancy(occ)
        with pytest.raises(RuntimeError):
            e.get_distance_field()
        L = capi.lib()
        assert L.mppi_set_occupancy(e._h, None, occ.ctypes.data_as(C.POINTER(C.c_uint8)), 0.0) == capi.ERR_STATE
        assert L.mppi_get_distance_field(e._h, None, None, None) == capi.ERR_STATE
        e.close()
    f = TD._engine(spec, FO.Field(FO.DIMS, FO.VOXEL, np.zeros(3), np.zeros(FO.DIMS[::-1], np.float32)), model="arm", n_samples=64, n_horizon=32)
    L = capi.lib()
    assert L.mppi_set_occupancy(f._h, None, None, 0.0) == capi.ERR_INVALID_ARG
    assert L.mppi_set_occupancy(f._h, None, occ.ctypes.data_as(C.POINTER(C.c_uint8)), float("nan")) == capi.ERR_INVALID_ARG
    assert L.mppi_set_occupancy(f._h, capi.fptr(np.float32([0.0, np.inf, 0.0])), occ.ctypes.data_as(C.POINTER(C.c_uint8)), 0.0) == capi.ERR_INVALID_ARG
    assert f.get_distance_field() is None, "the refused calls changed nothing"
    with pytest.raises(TypeError):
        f.set_occupancy(occ.astype(np.float32))
    with pytest.raises(ValueError):
        f.set_occupancy(occ[:-1])
    f.close()
