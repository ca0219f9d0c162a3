"""The nominal plan (mppi_get_plan, csrc/mppi_plan.hip), CPU side: the header declares the entry
point and the library exports it at ABI 10, the plan unit has its own gfx950 code object, and the
launcher -- described into a capture target, without a GPU (mppi_debug_plan_kernel) -- names a
kernel that code object holds, at one block per vehicle with one lane per horizon step.  The GPU
side is tests/test_gpu_plan.py."""
import ctypes as C
import os
import re
import struct

import pytest

from conftest import ROOT
from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd import build as B

DRONE, ARM, WB, QUAD = capi.MODEL_DRONE, capi.MODEL_ARM, capi.MODEL_WHOLEBODY, capi.MODEL_QUADROTOR
UNIT = "mppi_plan.hip"


def _plan_kernel(model, A, H, V=1, f64=0, literal=0):
    L = capi.lib()
    f = L.mppi_debug_plan_kernel
    f.restype = C.c_int32
    f.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_int32]
    g = (C.c_int32 * 6)(model, A, H, V, f64, literal)
    buf = C.create_string_buffer(256)
    assert f(g, buf, 256) == 0
    m = re.fullmatch(r"(\S+) grid (\d+) block (\d+)", buf.value.decode())
    assert m, buf.value
    return m.group(1), int(m.group(2)), int(m.group(3))


def _code_object():
    assert UNIT in B.KERNEL_UNITS
    path = B.code_object_path(B.LIB, UNIT)
    assert os.path.exists(path), f"{path} missing (python -m quadrotor_manipulator_mppi_amd.build)"
    return path


def test_header_declares_and_library_exports_get_plan():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mppi_hip.h")).read(), flags=re.S)
    assert re.search(r"mppi_status\s+mppi_get_plan\s*\(\s*mppi_engine\s*\*\s*e\s*,\s*float\s*\*\s*traj\s*,\s*float\s*\*"
                     r"\s*cost_t\s*,\s*float\s*\*\s*pos_err\s*,\s*float\s*\*\s*S\s*\)\s*;", src)
    assert "#define MPPI_ABI_VERSION 10" in src
    L = capi.lib()
    assert hasattr(L, "mppi_get_plan") and "mppi_get_plan" in capi.PROTOTYPES
    assert L.mppi_abi_version() == 10 and capi.ABI_VERSION == 10


def test_plan_unit_has_a_gfx950_code_object():
    with open(_code_object(), "rb") as f:
        head = f.read(64)
    assert head[:4] == b"\x7fELF"
    (e_machine,) = struct.unpack_from("<H", head, 18)
    assert e_machine == 224   # EM_AMDGPU
    (flags,) = struct.unpack_from("<I", head, 48)
    assert flags & 0xFF == 0x4F, f"not gfx950 (mach {flags & 0xFF:#x})"


CONFIGS = [(DRONE, 3, 0, 0), (ARM, 7, 0, 0), (ARM, 7, 1, 0), (WB, 10, 0, 0)]


@pytest.mark.parametrize("H", [20, 32, 64, 96, 256])
def test_plan_launch_symbol_and_geometry(H):
    """Every configuration's symbol is in the code object, its block is 64 * ceil(H/64) threads and
    its grid is V; the quadrotor's (H <= 64) likewise, in both quad_literal_jinv modes."""
    with open(_code_object(), "rb") as f:
        blob = f.read()
    cfgs = CONFIGS + ([(QUAD, 4, 0, 0), (QUAD, 4, 0, 1)] if H <= 64 else [])
    seen = set()
    for model, A, f64, lit in cfgs:
        for V in (1, 3, 64):
            sym, grid, block = _plan_kernel(model, A, H, V, f64, lit)
            assert (sym + ".kd").encode() in blob, f"{sym}.kd not in the plan unit's code object"
            assert "k_plan" in sym
            assert block == 64 * ((H + 63) // 64) and grid == V, (model, H, V, grid, block)
            seen.add(sym)
    assert len(seen) == len(cfgs)   # one kernel per (model, state dtype / literal mode)


def test_plan_launcher_refuses_what_it_has_no_kernel_for():
    L = capi.lib()
    f = L.mppi_debug_plan_kernel
    f.restype = C.c_int32
    f.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_int32]
    buf = C.create_string_buffer(256)
    for bad in [(ARM, 6, 32, 1, 0, 0), (QUAD, 4, 65, 1, 0, 0), (DRONE, 3, 257, 1, 0, 0), (DRONE, 3, 0, 1, 0, 0)]:
        assert f((C.c_int32 * 6)(*bad), buf, 256) != 0, bad
