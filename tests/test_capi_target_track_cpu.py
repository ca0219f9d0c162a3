"""Target tracking (MPPI_COST_TARGET_TRACK, mppi_set_target_trajectory) without a GPU: the export and
the binding, config validation through the host-side layout path (mppi_debug_layout: validate and
layout_of, as tools/layout_host_check.cpp reaches them), the rollout launchers' kernel choice
(mppi_debug_rollout_kernels), and the argument layout of a tracking engine's step launches
(mppi_debug_step_launches).

The plan kernel's symbols and launch geometry are unchanged for the recorded sweep: the existing
fixture test (tests/test_capi_plan_cpu.py) covers that and is not repeated here.
"""
import ctypes as C
import os
import re

import pytest

from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd import build as B
from quadrotor_manipulator_mppi_amd.engine import cost_term_bits, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRONE, ARM, WB, QUAD = capi.MODEL_DRONE, capi.MODEL_ARM, capi.MODEL_WHOLEBODY, capi.MODEL_QUADROTOR
TRACK = 32


# ------------------------------------------------------------------------- exports and config
def test_export_and_binding():
    with open(os.path.join(ROOT, "include", "mppi_hip.h")) as f:
        header = f.read()
    assert re.search(r"mppi_status\s+mppi_set_target_trajectory\s*\(\s*mppi_engine\*", header)
    assert re.search(r"MPPI_COST_TARGET_TRACK\s*=?\s*32", header)
    L = capi.lib()
    assert hasattr(L, "mppi_set_target_trajectory")
    assert "mppi_set_target_trajectory" in capi.PROTOTYPES
    assert capi.COST_TARGET_TRACK == TRACK
    assert cost_term_bits(["target_track"]) == TRACK
    assert cost_term_bits(("target_track", "center")) == TRACK | capi.COST_CENTER
    assert L.mppi_abi_version() == 10 == capi.ABI_VERSION
    sizes = [C.c_int32(), C.c_int32(), C.c_int32()]
    L.mppi_struct_sizes(*[C.byref(s) for s in sizes])
    assert tuple(s.value for s in sizes) == (C.sizeof(capi.Config), C.sizeof(capi.Joint), C.sizeof(capi.Stats))


def _layout_status(model, bits):
    L = capi.lib()
    f = L.mppi_debug_layout
    f.restype, f.argtypes = C.c_int32, [C.POINTER(capi.Config), C.POINTER(C.c_int32), C.c_int32]
    cfg = make_config(model, n_samples=64, n_horizon=32)
    cfg.cost_terms = bits
    out = (C.c_int32 * 28)()
    return f(C.byref(cfg), out, 28)


@pytest.mark.parametrize("model", ["drone", "arm", "wholebody", "quadrotor"])
def test_the_bit_is_accepted_on_every_model(model):
    assert _layout_status(model, TRACK) == capi.OK, capi.lib().mppi_last_error()
    assert _layout_status(model, 64) == capi.ERR_INVALID_ARG
    assert _layout_status(model, 64 | TRACK) == capi.ERR_INVALID_ARG
    assert _layout_status(model, 1 << 20) == capi.ERR_INVALID_ARG


@pytest.mark.parametrize("model", ["drone", "quadrotor"])
@pytest.mark.parametrize("bit", [1, 2, 4, 8, 16])
def test_costmanager_terms_stay_refused_on_the_vehicles(model, bit):
    assert _layout_status(model, bit) == capi.ERR_INVALID_ARG
    assert _layout_status(model, bit | TRACK) == capi.ERR_INVALID_ARG


@pytest.mark.parametrize("model", ["arm", "wholebody"])
def test_costmanager_terms_go_with_tracking_on_the_arms(model):
    assert _layout_status(model, 31) == capi.OK
    assert _layout_status(model, 31 | TRACK) == capi.OK


def test_layout_without_the_bit_allocates_no_tables_with_it():
    """cost_terms = 32 alone builds none of the CostManager tables: the layout's parameter digest
    differs from the plain engine's in the cost_terms word only, and the geometry is the same."""
    L = capi.lib()
    f = L.mppi_debug_layout
    f.restype, f.argtypes = C.c_int32, [C.POINTER(capi.Config), C.POINTER(C.c_int32), C.c_int32]
    outs = []
    for bits in (0, TRACK):
        cfg = make_config("arm", n_samples=256, n_horizon=32)
        cfg.cost_terms = bits
        out = (C.c_int32 * 28)()
        assert f(C.byref(cfg), out, 28) == capi.OK
        outs.append(list(out))
    assert outs[0][:26] == outs[1][:26]          # geometry, sizes, offsets
    assert outs[0][26:] != outs[1][26:]          # the digest over DevParams (cost_terms)


# ---------------------------------------------------------------------------- rollout symbols
def _kernels(model, A, H, V=1, f64=0, cost_terms=0, iters=1, threads=512):
    L = capi.lib()
    f = L.mppi_debug_rollout_kernels
    f.restype = C.c_int32
    f.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_char_p, C.c_int32]
    seg, nch = (32 if H <= 32 else 64), (1 if H <= 64 else 2 if H <= 128 else 4)
    g = (C.c_int32 * 15)(model, A, H, seg, nch, iters, threads, V, f64, capi.NOISE_PHILOX, 0, cost_terms, 0, 0, 0)
    full, quiet = C.create_string_buffer(192), C.create_string_buffer(192)
    assert f(g, full, quiet, 192) == 0, (model, A, H, V, cost_terms)
    return full.value.decode(), quiet.value.decode(), seg, nch


# (model, A, fp64 state, the unit of its kernels at (seg, nch))
ROWS = [
    (DRONE, 3, 0, lambda seg, nch: "mppi_rollout_drone.hip"),
    (ARM, 7, 0, lambda seg, nch: "mppi_rollout_arm32.hip"),
    (ARM, 7, 1, lambda seg, nch: "mppi_rollout_arm_h32.hip" if (seg, nch) == (32, 1) else "mppi_rollout_arm.hip"),
    (WB, 10, 0, lambda seg, nch: "mppi_rollout_wb.hip"),
    (QUAD, 4, 0, lambda seg, nch: "mppi_rollout_quad.hip"),
]
HORIZONS = (20, 32, 64, 128, 200)


def _cases():
    for model, A, f64, unit in ROWS:
        for H in HORIZONS:
            if model == QUAD and H > 64:   # (k_rollout_quad: H <= 64, as today)
                continue
            for V in (1, 3):
                yield model, A, f64, unit, H, V


@pytest.mark.parametrize("model,A,f64,unit,H,V", list(_cases()),
                         ids=[f"m{m}-f{f}-H{H}-V{V}" for m, _, f, _, H, V in _cases()])
def test_tracking_symbols(model, A, f64, unit, H, V):
    blob = None
    for terms in (TRACK, TRACK | capi.COST_CENTER):
        if model in (DRONE, QUAD) and terms != TRACK:
            continue
        full, quiet, seg, nch = _kernels(model, A, H, V=V, f64=f64, cost_terms=terms)
        assert full == quiet, "tracking engines run the full kernel on every step"
        vone = int(V == 1)
        if model == QUAD:
            assert full.startswith(f"_Z17k_rollout_quad_ttILb{vone}ELb0ELi1ELi"), full
        else:
            assert full.startswith(f"_Z12k_rollout_ttILi{model}ELi{A}ELi{nch}ELi{seg}ELb{f64}ELb{vone}EEv"), full
        if blob is None:
            with open(B.code_object_path(B.LIB, unit(seg, nch)), "rb") as f:
                blob = f.read()
        assert (full + ".kd").encode() in blob, (unit(seg, nch), full)
    # without the bit: today's symbols
    for terms in (0, capi.COST_CENTER):
        if model in (DRONE, QUAD) and terms:
            continue
        full, quiet, _, _ = _kernels(model, A, H, V=V, f64=f64, cost_terms=terms)
        assert "_tt" not in full and "_tt" not in quiet, (full, quiet)
        assert ("k_rollout_quad" in full) == (model == QUAD)


def test_tracking_loops_groups_and_takes_any_block_size():
    for kw in (dict(iters=16, threads=128), dict(iters=3), dict(threads=256)):
        full, quiet, _, _ = _kernels(ARM, 7, 32, f64=1, cost_terms=TRACK, **kw)
        assert full == quiet and full.startswith("_Z12k_rollout_ttILi1ELi7ELi1ELi32ELb1ELb1EEv")


# ---------------------------------------------------------------------------- argument layout
SW_ORDER = ("path", "n", "peer", "comm", "timing", "generic", "out_dbg")
LINE = re.compile(r"(early|last) (rollout|pack|finalize) (\S+) grid (\d+) block (\d+) lds (\d+) args (\d+) fnv ([0-9a-f]{16})")


def _launches(cfg, **sw):
    f = capi.lib().mppi_debug_step_launches
    f.restype, f.argtypes = capi.DEBUG_PROTOTYPES["mppi_debug_step_launches"]
    buf = C.create_string_buffer(4096)
    st = f(C.byref(cfg), (C.c_int32 * len(SW_ORDER))(*[sw.get(k, 0) for k in SW_ORDER]), buf, len(buf))
    assert st == capi.OK, capi.lib().mppi_last_error()
    return [LINE.fullmatch(ln).groups() for ln in buf.value.decode().splitlines()]


@pytest.mark.parametrize("path,n", [(0, 3), (2, 3), (3, 1)], ids=["hip-batch", "native-batch", "native-call"])
def test_step_launches_carry_the_table_pointer(path, n):
    """HIP batch, native batch, native call of a tracking arm engine: the tracking rollout on every
    step, its argument block the extended (XC) launch's plus the 8 bytes of the table pointer, the
    finalize as the XC engine's."""
    kw = dict(n_samples=256, n_horizon=32)
    trk = _launches(make_config("arm", cost_terms=("target_track",), **kw), path=path, n=n)
    xc = _launches(make_config("arm", cost_terms=("center",), cost_weights={"w_center": 0.0}, **kw), path=path, n=n)
    assert len(trk) == len(xc) == (4 if n > 1 else 2)
    for t, x in zip(trk, xc):
        assert t[:2] == x[:2]
        if t[1] == "rollout":
            assert "k_rollout_tt" in t[2] and "k_rollout_tt" not in x[2]
            assert int(t[6]) == int(x[6]) + 8, (t, x)
            assert t[3:6] == x[3:6]            # grid, block, LDS as the XC launch
        else:
            assert t[2:7] == x[2:7]            # the finalize: same kernel, geometry and argument size


def test_quadrotor_tracking_launch_adds_the_rows_to_lds():
    kw = dict(n_samples=256, n_horizon=32)
    trk = _launches(make_config("quadrotor", cost_terms=("target_track",), **kw), path=0, n=1)
    fix = _launches(make_config("quadrotor", **kw), path=0, n=1)
    t, x = trk[0], fix[0]
    assert "k_rollout_quad_tt" in t[2] and int(t[6]) == int(x[6]) + 8
    assert int(t[5]) == int(x[5]) + (32 + 1) * 4 * 4   # the (H + 1, 4) target rows
