"""Occupancy grids (mppi_set_occupancy, mppi_get_distance_field, mppi_occupancy_field; csrc/mppi_edt.hip),
CPU side: the host helper -- the same definition and the same inline for the value as the device
transform -- against the float64 oracle (tests/occupancy_oracle.py) on the grid list of
tests/test_gpu_occupancy.py, the oracle's squared distances against brute force, the error returns, the
three prototypes in header and binding at ABI 10, the new unit's gfx950 code object and the kernels its
launcher names at in-bounds geometry, and DistanceField.from_occupancy.  The GPU side is
tests/test_gpu_occupancy.py."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import occupancy_oracle as OC
from conftest import ROOT
from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd import build as B
from quadrotor_manipulator_mppi_amd.engine import DistanceField

UNIT = "mppi_edt.hip"
U8 = C.POINTER(C.c_uint8)


def _host(occ, dims, voxel=OC.VOXEL, max_dist=None):
    return DistanceField.from_occupancy(occ, dims, voxel, max_dist=max_dist).d


def _raw(desc, occ, max_dist, out):
    return capi.lib().mppi_occupancy_field(None if desc is None else C.byref(desc), None if occ is None else occ.ctypes.data_as(U8),
                                           max_dist, None if out is None else capi.fptr(out))


def check_against_oracle(d, ref, what):
    """d float32 against the oracle within its tolerance, and the sign equal to the occupancy at every node."""
    err = np.abs(d.astype(np.float64) - ref["d"])
    worst = float(np.max(err / ref["tol"]))
    print(f"{what}: worst |d - oracle| = {err.max():.3e} m, {worst:.3f} x the tolerance; "
          f"{int(ref['unclamped'].sum())} of {d.size} nodes off the cap")
    assert worst <= 1.0, what
    assert np.array_equal(d < 0.0, ref["occ"]), what + ": the sign is the occupancy"
    assert np.all(np.abs(d) <= np.float32(ref["cap"])), what


# ------------------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("dims", [(2, 2, 2), (7, 5, 3), (12, 9, 10)])
def test_oracle_squared_distances_are_exact(dims):
    for name in OC.PATTERNS:
        occ = OC.pattern(name, dims)
        for got, want in zip(OC.squared_distances(occ), OC.brute_squared_distances(occ)):
            assert np.array_equal(got, want), (dims, name)


def test_oracle_refuses_a_case_it_cannot_resolve():
    dims = (512, 4, 4)
    occ = OC.pattern("corner", dims)
    with pytest.raises(AssertionError):
        OC.field(occ, dims, OC.VOXEL, None)
    assert OC.uncapped_or(occ, dims, OC.VOXEL) == pytest.approx(140 * OC.VOXEL)
    OC.field(occ, dims, OC.VOXEL, OC.uncapped_or(occ, dims, OC.VOXEL))
    assert OC.uncapped_or(OC.pattern("box", dims), dims, OC.VOXEL) is None


# ------------------------------------------------------------------------ the host helper vs the oracle
@pytest.mark.parametrize("dims", OC.DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("name", OC.PATTERNS)
def test_host_helper_matches_oracle(dims, name):
    occ = OC.pattern(name, dims)
    for max_dist in (OC.uncapped_or(occ, dims, OC.VOXEL), 3.5 * OC.VOXEL):
        ref = OC.field(occ, dims, OC.VOXEL, max_dist)
        d = _host(occ, dims, max_dist=max_dist)
        assert d.dtype == np.float32 and d.shape == dims[::-1]
        check_against_oracle(d, ref, f"host {dims} {name} max_dist {max_dist}")
        if name == "empty":
            assert np.all(d == np.float32(ref["cap"]))
        if name == "full":
            assert np.all(d == -np.float32(ref["cap"]))


@pytest.mark.parametrize("dims", [(33, 20, 24), (512, 4, 4), (4, 4, 512)], ids=lambda d: "x".join(map(str, d)))
def test_cases_can_show_the_mistakes(dims):
    """On the oracle alone: the seed sets swapped shows in every pattern, the 0.5 offset dropped wherever a
    node is off the cap, a skipped axis pass in the patterns with a seed off that axis' planes."""
    for name in OC.PATTERNS:
        occ = OC.pattern(name, dims)
        ref = OC.field(occ, dims, OC.VOXEL, 3.5 * OC.VOXEL)
        m = OC.mistakes(ref, OC.VOXEL)
        print(dims, name, {k: f"{v:.3g}" for k, v in m.items()})
        assert m["swapped"] > OC.RESOLVE
        if name not in ("empty", "full"):
            assert m["no_offset"] > OC.RESOLVE
        if name in ("corner", "box", "random"):
            assert min(m["skip_x"], m["skip_y"], m["skip_z"]) > OC.RESOLVE


def test_no_cap_and_huge_cap():
    dims = (9, 8, 7)
    occ = OC.pattern("box", dims)
    free = _host(occ, dims)
    assert np.array_equal(free, _host(occ, dims, max_dist=0.0)) and np.array_equal(free, _host(occ, dims, max_dist=-1.0))
    assert np.array_equal(free, _host(occ, dims, max_dist=1e6))   # a cap no node reaches changes nothing
    assert np.all(_host(OC.pattern("empty", dims), dims, max_dist=1e6) == np.float32(1e6))
    assert np.all(_host(OC.pattern("full", dims), dims, max_dist=1e6) == np.float32(-1e6))
    # one free node in a full grid: the face lies half a voxel from it
    occ = OC.pattern("full", dims)
    occ[3, 4, 5] = False
    d = _host(occ, dims)
    assert d[3, 4, 5] == np.float32(0.5 * np.float32(OC.VOXEL)) and d[3, 4, 6] == -d[3, 4, 5]


def test_uint8_values_other_than_one_are_occupied():
    dims = (6, 5, 4)
    occ = OC.pattern("random", dims, seed=3) | OC.pattern("corner", dims)
    as_bool = _host(occ, dims)
    as_bytes = _host(np.where(occ, 255, 0).astype(np.uint8), dims)
    odd = _host(np.where(occ, 2, 0).astype(np.uint8), dims)
    assert np.array_equal(as_bool, as_bytes) and np.array_equal(as_bool, odd)


# ------------------------------------------------------------------------------------ error returns
def test_host_helper_error_returns():
    f = DistanceField((6, 5, 4), OC.VOXEL)
    desc = f.to_c()
    occ = np.zeros(f.shape, np.uint8)
    out = np.zeros(f.shape, np.float32)
    assert _raw(desc, occ, 0.0, out) == capi.OK
    assert _raw(None, occ, 0.0, out) == capi.ERR_INVALID_ARG
    assert _raw(desc, None, 0.0, out) == capi.ERR_INVALID_ARG
    assert _raw(desc, occ, 0.0, None) == capi.ERR_INVALID_ARG
    assert _raw(desc, occ, float("nan"), out) == capi.ERR_INVALID_ARG
    assert _raw(desc, occ, float("inf"), out) == capi.ERR_INVALID_ARG
    assert _raw(desc, occ, float("-inf"), out) == capi.OK   # (<= 0: no cap)
    for dims in [(1, 5, 4), (6, 513, 4), (512, 512, 16)]:
        bad = DistanceField(dims, OC.VOXEL).to_c()
        assert _raw(bad, occ, 0.0, out) == capi.ERR_INVALID_ARG
    bad = f.to_c()
    bad.voxel = 0.0
    assert _raw(bad, occ, 0.0, out) == capi.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        DistanceField.from_occupancy(np.zeros((4, 5, 7), bool), (6, 5, 4), OC.VOXEL)
    with pytest.raises(TypeError):
        DistanceField.from_occupancy(np.zeros(f.shape, np.float32), (6, 5, 4), OC.VOXEL)
    with pytest.raises(capi.MPPIError):
        DistanceField.from_occupancy(occ, (6, 5, 4), OC.VOXEL, max_dist=float("nan"))


def test_set_and_get_refuse_a_null_engine():
    L = capi.lib()
    occ = np.zeros(8, np.uint8)
    assert L.mppi_set_occupancy(None, None, occ.ctypes.data_as(U8), 0.0) == capi.ERR_INVALID_ARG
    assert L.mppi_get_distance_field(None, None, None, None) == capi.ERR_INVALID_ARG


# ------------------------------------------------------------------- header, binding, ABI, code object
def test_header_declares_and_library_exports_the_three_functions():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mppi_hip.h")).read(), flags=re.S)
    assert re.search(r"mppi_status\s+mppi_set_occupancy\s*\(\s*mppi_engine\s*\*\s*e\s*,\s*const\s+float\s*\*\s*origin3\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*occ_zyx\s*,\s*float\s+max_dist\s*\)\s*;", src)
    assert re.search(r"mppi_status\s+mppi_get_distance_field\s*\(\s*mppi_engine\s*\*\s*e\s*,\s*int32_t\s*\*\s*is_set\s*,"
                     r"\s*float\s*\*\s*origin3\s*,\s*float\s*\*\s*d_zyx\s*\)\s*;", src)
    assert re.search(r"mppi_status\s+mppi_occupancy_field\s*\(\s*const\s+mppi_field_desc\s*\*\s*desc\s*,\s*const\s+uint8_t\s*\*\s*occ_zyx\s*,"
                     r"\s*float\s+max_dist\s*,\s*float\s*\*\s*d_zyx\s*\)\s*;", src)
    assert "#define MPPI_ABI_VERSION 10" in src
    L = capi.lib()
    for name in ("mppi_set_occupancy", "mppi_get_distance_field", "mppi_occupancy_field"):
        assert hasattr(L, name) and name in capi.PROTOTYPES, name
    assert L.mppi_abi_version() == 10 and capi.ABI_VERSION == 10
    assert capi.PROTOTYPES["mppi_set_occupancy"] == (C.c_int32, [C.c_void_p, capi._F, U8, C.c_float])


def _code_object():
    assert UNIT in B.KERNEL_UNITS
    path = B.code_object_path(B.LIB, UNIT)
    assert os.path.exists(path), f"{path} missing (python -m quadrotor_manipulator_mppi_amd.build)"
    return path


def test_edt_unit_has_a_gfx950_code_object():
    with open(_code_object(), "rb") as f:
        head = f.read(64)
    assert head[:4] == b"\x7fELF"
    (e_machine,) = struct.unpack_from("<H", head, 18)
    assert e_machine == 224   # EM_AMDGPU
    (flags,) = struct.unpack_from("<I", head, 48)
    assert flags & 0xFF == 0x4F, f"not gfx950 (mach {flags & 0xFF:#x})"


def _edt_kernels(nx, ny, nz):
    f = capi.lib().mppi_debug_edt_kernels
    f.restype, f.argtypes = capi.DEBUG_PROTOTYPES["mppi_debug_edt_kernels"]
    buf = C.create_string_buffer(2048)
    if f((C.c_int32 * 3)(nx, ny, nz), buf, 2048) != 0:
        return None
    out = []
    for one in buf.value.decode().split("; "):
        m = re.fullmatch(r"(\S+) grid (\d+)x(\d+) block (\d+) lds (\d+)", one)
        assert m, buf.value
        out.append((m.group(1),) + tuple(int(m.group(i)) for i in range(2, 6)))
    return out


@pytest.mark.parametrize("dims", OC.DIMS + [(512, 512, 8), (8, 512, 512), (128, 128, 128)], ids=lambda d: "x".join(map(str, d)))
def test_edt_launch_symbols_and_geometry(dims):
    """The four launches' symbols are in the unit's code object; the x pass has a wave per row, the y and z
    passes a block per tile of 16 columns and per z (y) with both grids' lines in at most 64 KiB of LDS,
    the finish a thread per node."""
    nx, ny, nz = dims
    with open(_code_object(), "rb") as f:
        blob = f.read()
    launches = _edt_kernels(nx, ny, nz)
    assert launches and len(launches) == 4
    for sym, gx, gy, block, lds in launches:
        assert (sym + ".kd").encode() in blob, f"{sym}.kd not in the unit's code object"
        assert "k_edt" in sym and block == 256 and lds <= 65536
    tiles = (nx + 15) // 16
    assert "k_edt_x" in launches[0][0] and launches[0][1:3] == ((ny * nz + 3) // 4, 1) and launches[0][4] == 0
    assert "k_edt_axis" in launches[1][0] and launches[1][1:3] == (tiles, nz) and launches[1][4] == 2 * ny * 16 * 4
    assert "k_edt_axis" in launches[2][0] and launches[2][1:3] == (tiles, ny) and launches[2][4] == 2 * nz * 16 * 4
    assert "k_edt_finish" in launches[3][0] and launches[3][1:3] == ((nx * ny * nz + 255) // 256, 1)


def test_edt_launcher_refuses_dims_outside_the_field_limits():
    for dims in [(1, 4, 4), (4, 0, 4), (4, 4, 513), (512, 512, 16), (-2, 4, 4)]:
        assert _edt_kernels(*dims) is None, dims


# -------------------------------------------------------------------- the drop-in and sharded passthroughs
class _RecordingEngine:
    def __init__(self):
        self.calls = []

    def set_occupancy(self, occ, origin=None, max_dist=None):
        self.calls.append(("occ", occ.copy(), origin, max_dist))

    def set_distance_field(self, d, origin=None):
        self.calls.append(("sdf", d.copy(), origin))

    def clear_distance_field(self):
        self.calls.append(("clear",))

    def get_distance_field(self):
        return "the engine's"


def test_dropin_set_occupancy_reaches_the_engine_once_per_change():
    from quadrotor_manipulator_mppi_amd.mppi_solver._base import SolverBase
    s = object.__new__(SolverBase)   # (no engine, no GPU: the field bookkeeping only)
    s._engine = None
    with pytest.raises(RuntimeError):
        s.set_occupancy(np.zeros((4, 5, 6), bool))
    with pytest.raises(RuntimeError):
        s.get_distance_field()
    s._init_field(DistanceField((6, 5, 4), OC.VOXEL))
    assert s.get_distance_field() is None   # before the first control call has made the engine
    occ = OC.pattern("box", (6, 5, 4))
    s.set_occupancy(occ, origin=(1, 2, 3), max_dist=0.3)
    occ_before = occ.copy()
    occ[:] = False                          # the caller's array is free on return
    eng = _RecordingEngine()
    s._sync_field(eng)
    s._sync_field(eng)                      # unchanged: not sent again
    assert len(eng.calls) == 1 and eng.calls[0][0] == "occ" and eng.calls[0][3] == 0.3
    assert np.array_equal(eng.calls[0][1], occ_before.view(np.uint8)) and np.array_equal(eng.calls[0][2], np.float32([1, 2, 3]))
    s.set_distance_field(np.ones((4, 5, 6), np.float32))
    s._sync_field(eng)
    s.clear_distance_field()
    s._sync_field(eng)
    assert [c[0] for c in eng.calls] == ["occ", "sdf", "clear"]
    s._engine = eng
    assert s.get_distance_field() == "the engine's"
    with pytest.raises(ValueError):
        s.set_occupancy(np.zeros((4, 5, 7), bool))


def test_sharded_engine_passes_the_map_to_its_rank():
    from quadrotor_manipulator_mppi_amd.distributed import ShardedEngine
    se = object.__new__(ShardedEngine)   # (no Engine, no HIP stream)
    se.engine = _RecordingEngine()
    se.set_occupancy(np.ones((2, 2, 2), np.uint8), None, 0.5)
    assert se.engine.calls[0][0] == "occ" and se.engine.calls[0][3] == 0.5
    assert se.get_distance_field() == "the engine's"


# ----------------------------------------------------------------------------------- from_occupancy
def test_from_occupancy_round_trip():
    dims, origin = (12, 10, 8), (0.5, -1.0, 0.25)
    occ = OC.pattern("box", dims)
    f = DistanceField.from_occupancy(occ, dims, OC.VOXEL, origin, max_dist=0.2)
    assert f.dims == dims and f.origin == origin and f.d.shape == (8, 10, 12) and f.d.dtype == np.float32
    assert np.array_equal(f.d < 0.0, occ)
    assert float(np.abs(f.d).max()) == pytest.approx(0.2)
    again = DistanceField.from_occupancy(f.d < 0.0, dims, OC.VOXEL, origin, max_dist=0.2)   # the field's sign is the map
    assert np.array_equal(again.d, f.d)
    g = DistanceField(dims, OC.VOXEL, origin, f.d)   # usable as a field engine's data
    assert np.array_equal(g.d, f.d)
