"""Obstacle avoidance (mppi_create_scene, mppi_set_obstacles) without a GPU: the exports and the
binding, every error of the scene and of an obstacle set through the host-side layout path
(mppi_debug_scene_layout, mppi_debug_obstacles: validate, scene_validate, scene_body_table,
obstacles_validate / obstacles_fill, as tools/obstacle_host_check.cpp reaches them), the scene
launchers' kernel choice (mppi_debug_scene_rollout_kernels) and the argument layout of a scene engine's
step launches (mppi_debug_scene_step_launches).  An engine without a scene gets the symbols and
descriptions it had: the existing golden tests cover that, one identity is repeated here.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd import build as B
from quadrotor_manipulator_mppi_amd.engine import Scene, make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRONE, ARM, WB, QUAD = capi.MODEL_DRONE, capi.MODEL_ARM, capi.MODEL_WHOLEBODY, capi.MODEL_QUADROTOR
BODY_W, OBS_W, RNG, SPH = 92, 132, 8, 28   # csrc/mppi_obstacles.h
NEW = ("mppi_scene_default", "mppi_create_scene", "mppi_set_obstacles", "mppi_get_clearances", "mppi_get_plan_clearance")


def _bind(name):
    f = getattr(capi.lib(), name)
    f.restype, f.argtypes = capi.DEBUG_PROTOTYPES[name]
    return f


# ------------------------------------------------------------------------- exports and config
def test_exports_and_binding():
    with open(os.path.join(ROOT, "include", "mppi_hip.h")) as f:
        header = f.read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in capi.PROTOTYPES, name
    assert re.search(r"#define\s+MPPI_MAX_OBSTACLES\s+16", header) and capi.MAX_OBSTACLES == 16
    assert re.search(r"#define\s+MPPI_MAX_BODY_SPHERES\s+16", header) and capi.MAX_BODY_SPHERES == 16
    assert re.search(r"#define\s+MPPI_ABI_VERSION\s+10\b", header)
    assert L.mppi_abi_version() == 10 == capi.ABI_VERSION
    sizes = [C.c_int32(), C.c_int32(), C.c_int32()]
    L.mppi_struct_sizes(*[C.byref(s) for s in sizes])
    assert tuple(s.value for s in sizes) == (C.sizeof(capi.Config), C.sizeof(capi.Joint), C.sizeof(capi.Stats))
    assert C.sizeof(capi.BodySphere) == 20 and C.sizeof(capi.Scene) == 4 + 16 * 20 + 12


def _layout(cfg, scene, table=False):
    f = _bind("mppi_debug_scene_layout")
    sc = scene.to_c() if isinstance(scene, Scene) else scene
    t = np.zeros(BODY_W, np.float32)
    order = (C.c_int32 * 16)()
    st = f(C.byref(cfg), C.byref(sc), capi.fptr(t), order)
    return (st, t, list(order)) if table else st


@pytest.mark.parametrize("model", ["drone", "arm", "wholebody"])
def test_default_scene_and_its_errors(model):
    cfg = make_config(model, n_samples=64, n_horizon=32)
    s = Scene.default(cfg)
    assert (s.w_obs, round(s.margin, 6), s.penalty) == (100.0, 0.05, 1e4)
    moving = [j for j in range(cfg.n_joints) if cfg.joints[j].type != capi.JOINT_FIXED]
    want = ([(-1, 0.30)] if model != "arm" else []) + ([(j, 0.05) for j in moving] if model != "drone" else [])
    assert [(f, round(r, 6)) for f, _, r in s.body] == want
    assert all(o == (0.0, 0.0, 0.0) for _, o, _ in s.body)
    from quadrotor_manipulator_mppi_amd.robot import body_spheres as BS
    from quadrotor_manipulator_mppi_amd.robot.urdf_chain import load_chain
    assert [(f, o, round(r, 6)) for f, o, r in s.body] == [(f, o, r) for f, o, r in BS.default_body(model, load_chain())]
    assert (BS.W_OBS, BS.MARGIN, BS.PENALTY) == (100.0, 0.05, 1e4)
    assert _layout(cfg, s) == capi.OK, capi.lib().mppi_last_error()
    nj = 0 if model == "drone" else cfg.n_joints
    bad = [Scene(((nj, (0, 0, 0), 0.1),)), Scene(((-2, (0, 0, 0), 0.1),)), Scene(((-1, (0, 0, 0), 0.0),)),
           Scene(((-1, (0, 0, 0), -0.1),)), Scene(((-1, (0, 0, 0), math.nan),)), Scene(((-1, (0, math.inf, 0), 0.1),)),
           Scene(s.body, w_obs=-1.0), Scene(s.body, margin=-0.01), Scene(s.body, penalty=-1.0), Scene(s.body, w_obs=math.nan)]
    for b in bad:
        assert _layout(cfg, b) == capi.ERR_INVALID_ARG, b
    c = s.to_c()
    for n in (-1, 17):
        c.n_body = n
        assert _layout(cfg, c) == capi.ERR_INVALID_ARG
    assert _layout(cfg, Scene(())) == capi.OK   # no body spheres: a scene engine that never meets anything
    if model == "drone":
        assert _layout(cfg, Scene(((0, (0, 0, 0), 0.1),))) == capi.ERR_INVALID_ARG   # no chain: frame -1 only


def test_quadrotor_scene_is_refused():
    cfg = make_config("quadrotor", n_samples=64, n_horizon=32)
    assert _layout(cfg, Scene(((-1, (0, 0, 0), 0.3),))) == capi.ERR_INVALID_ARG
    assert _layout(cfg, Scene.default(cfg)) == capi.ERR_INVALID_ARG
    from quadrotor_manipulator_mppi_amd.mppi_solver.quadrotor_mppi import MPPI
    with pytest.raises(NotImplementedError):
        MPPI(scene=True)


def test_body_table_folds_and_sorts():
    """The Kinova chain's leading fixed joint is folded into the base (j0 = 1): spheres on frames -1
    and 0 land in slot 0, frame f >= 1 in slot f; the table is sorted by slot, stable."""
    cfg = make_config("arm", n_samples=64, n_horizon=32)
    body = ((7, (0.0, 0.0, -0.1), 0.04), (0, (0.0, 0.02, 0.08), 0.07), (3, (0.01, 0.0, 0.0), 0.05),
            (-1, (0.0, 0.0, -0.05), 0.09), (3, (0.0, 0.03, 0.0), 0.06), (1, (0.0, 0.0, 0.0), 0.05))
    st, t, order = _layout(cfg, Scene(body, w_obs=7.0, margin=0.1, penalty=3.0), table=True)
    assert st == capi.OK
    w = t.view(np.int32)
    assert w[0] == 6 and (t[1], t[2], t[3]) == (7.0, np.float32(0.1), 3.0) and w[6] == 64
    assert order[:6] == [1, 3, 5, 2, 4, 0]
    rng = list(w[RNG:RNG + 18])
    assert rng[:9] == [0, 2, 3, 3, 5, 5, 5, 5, 6] and rng[9:] == [6] * 9
    for i, b in enumerate(order[:6]):
        assert t[SPH + 4 * i + 3] == np.float32(body[b][2])
        if body[b][0] >= 1:
            assert tuple(t[SPH + 4 * i:SPH + 4 * i + 3]) == tuple(np.float32(body[b][1]))
    # frame -1's offset seen from the folded frame: O_0^-1 (o, 1); frame 0's is its own
    J = cfg.joints[0]
    O = np.zeros(16, np.float32)
    capi.lib().mppi_joint_origin(C.byref(J), capi.fptr(O))
    O = O.reshape(4, 4).astype(np.float64)
    want = np.linalg.inv(O) @ np.array([0.0, 0.0, -0.05, 1.0])
    assert np.allclose(t[SPH + 4:SPH + 7], want[:3], atol=1e-6)
    assert np.allclose(t[SPH:SPH + 3], np.float32(body[1][1]), atol=0)


def test_obstacle_set_errors_and_block():
    f = _bind("mppi_debug_obstacles")
    c = np.arange(48, dtype=np.float32).reshape(16, 3) * 0.1
    r = np.full(16, 0.05, np.float32)
    v = np.ones((16, 3), np.float32)
    blk = np.full(OBS_W, -1.0, np.float32)
    assert f(2, 1, 16, capi.fptr(c), capi.fptr(r), capi.fptr(v), capi.fptr(blk)) == capi.OK
    assert blk.view(np.int32)[0] == 16 and np.array_equal(blk[4:].reshape(16, 8)[:, :3], c)
    assert np.array_equal(blk[4:].reshape(16, 8)[:, 3], r) and np.array_equal(blk[4:].reshape(16, 8)[:, 4:7], v)
    assert f(2, 0, 3, capi.fptr(c), capi.fptr(r), None, capi.fptr(blk)) == capi.OK          # NULL velocities: static
    assert blk.view(np.int32)[0] == 3 and not blk[4:].reshape(16, 8)[:, 4:].any() and not blk[4 + 24:].any()
    assert f(2, 0, 0, None, None, None, capi.fptr(blk)) == capi.OK and not blk.any()          # n = 0 clears
    for veh, n in ((2, 1), (-1, 1), (0, 17), (0, -1)):
        assert f(2, veh, n, capi.fptr(c), capi.fptr(r), None, None) == capi.ERR_INVALID_ARG
    for arr, i, x in ((r, 2, 0.0), (r, 0, -1.0), (r, 1, np.nan), (c, (3, 1), np.inf), (v, (15, 2), np.nan)):
        a = arr.copy()
        a[i] = x
        args = [capi.fptr(a if arr is c else c), capi.fptr(a if arr is r else r), capi.fptr(a if arr is v else v)]
        assert f(2, 0, 16, *args, None) == capi.ERR_INVALID_ARG, (i, x)


# ---------------------------------------------------------------------------- rollout symbols
def _kernels(hook, model, A, H, V=1, f64=0, cost_terms=0, iters=1, threads=512):
    f = _bind(hook) if hook in capi.DEBUG_PROTOTYPES else getattr(capi.lib(), hook)
    f.restype, f.argtypes = C.c_int32, [C.POINTER(C.c_int32), C.c_char_p, C.c_char_p, C.c_int32]
    seg, nch = (32 if H <= 32 else 64), (1 if H <= 64 else 2 if H <= 128 else 4)
    g = (C.c_int32 * 15)(model, A, H, seg, nch, iters, threads, V, f64, capi.NOISE_PHILOX, 0, cost_terms, 0, 0, 0)
    full, quiet = C.create_string_buffer(192), C.create_string_buffer(192)
    st = f(g, full, quiet, 192)
    return st, full.value.decode(), quiet.value.decode(), seg, nch


ROWS = [
    (DRONE, 3, 0, lambda seg, nch: "mppi_rollout_drone.hip"),
    (ARM, 7, 0, lambda seg, nch: "mppi_rollout_arm32.hip"),
    (ARM, 7, 1, lambda seg, nch: "mppi_rollout_arm_h32.hip" if (seg, nch) == (32, 1) else "mppi_rollout_arm.hip"),
    (WB, 10, 0, lambda seg, nch: "mppi_rollout_wb.hip"),
]
CASES = [(m, A, f, u, H, V) for m, A, f, u in ROWS for H in (20, 32, 64, 128, 200) for V in (1, 3)]


@pytest.mark.parametrize("model,A,f64,unit,H,V", CASES, ids=[f"m{m}-f{f}-H{H}-V{V}" for m, _, f, _, H, V in CASES])
def test_scene_symbols(model, A, f64, unit, H, V):
    blob = None
    for terms in (0, 32, 32 | capi.COST_CENTER, capi.COST_CENTER):
        if model == DRONE and terms & 31:
            continue
        st, full, quiet, seg, nch = _kernels("mppi_debug_scene_rollout_kernels", model, A, H, V=V, f64=f64, cost_terms=terms)
        assert st == 0 and full == quiet, "scene engines run the full kernel on every step"
        assert full.startswith(f"_Z12k_rollout_obILi{model}ELi{A}ELi{nch}ELi{seg}ELb{f64}ELb{int(V == 1)}EEv"), full
        if blob is None:
            with open(B.code_object_path(B.LIB, unit(seg, nch)), "rb") as f:
                blob = f.read()
        assert (full + ".kd").encode() in blob, (unit(seg, nch), full)
    # without a scene: the symbols as they were
    for terms in (0, 32):
        st, full, quiet, _, _ = _kernels("mppi_debug_rollout_kernels", model, A, H, V=V, f64=f64, cost_terms=terms)
        assert st == 0 and "_ob" not in full and "_ob" not in quiet, (full, quiet)


def test_no_quadrotor_scene_kernel():
    st, _, _, _, _ = _kernels("mppi_debug_scene_rollout_kernels", QUAD, 4, 32)
    assert st == capi.ERR_INVALID_ARG


def test_scene_kernel_loops_groups_and_takes_any_block_size():
    for kw in (dict(iters=16, threads=128), dict(iters=3), dict(threads=256)):
        st, full, quiet, _, _ = _kernels("mppi_debug_scene_rollout_kernels", ARM, 7, 32, f64=1, **kw)
        assert st == 0 and full == quiet and full.startswith("_Z12k_rollout_obILi1ELi7ELi1ELi32ELb1ELb1EEv")


# ---------------------------------------------------------------------------- argument layout
SW_ORDER = ("path", "n", "peer", "comm", "timing", "generic", "out_dbg")
LINE = re.compile(r"(early|last) (rollout|pack|finalize) (\S+) grid (\d+) block (\d+) lds (\d+) args (\d+) fnv ([0-9a-f]{16})")


def _launches(cfg, scene=None, plain=False, **sw):
    words = (C.c_int32 * len(SW_ORDER))(*[sw.get(k, 0) for k in SW_ORDER])
    buf = C.create_string_buffer(4096)
    if plain:
        st = _bind("mppi_debug_step_launches")(C.byref(cfg), words, buf, len(buf))
    else:
        sc = None if scene is None else C.byref(scene.to_c())
        st = _bind("mppi_debug_scene_step_launches")(C.byref(cfg), sc, words, buf, len(buf))
    assert st == capi.OK, capi.lib().mppi_last_error()
    return [LINE.fullmatch(ln).groups() for ln in buf.value.decode().splitlines()]


@pytest.mark.parametrize("path,n", [(0, 3), (2, 3), (3, 1)], ids=["hip-batch", "native-batch", "native-call"])
@pytest.mark.parametrize("terms", [(), ("target_track",)], ids=["fixed-target", "tracking"])
def test_step_launches_carry_the_scene_pointer(path, n, terms):
    """HIP batch, native batch, native call of a scene arm engine, with and without the tracking bit:
    the scene rollout on every step, its argument block the tracking launch's plus the 8 bytes of the
    scene pointer (before the trailing DevParams, whose size is unchanged), its LDS the tracking
    launch's plus the clearance runs, the finalize as the tracking engine's."""
    kw = dict(n_samples=256, n_horizon=32)
    cfg = make_config("arm", cost_terms=terms, **kw)
    ob = _launches(cfg, Scene.default(cfg), path=path, n=n)
    trk = _launches(make_config("arm", cost_terms=("target_track",), **kw), path=path, n=n)
    assert len(ob) == len(trk) == (4 if n > 1 else 2)
    for o, t in zip(ob, trk):
        assert o[:2] == t[:2]
        if o[1] == "rollout":
            assert "k_rollout_ob" in o[2] and "k_rollout_tt" in t[2]
            assert int(o[6]) == int(t[6]) + 8, (o, t)
            assert o[3:5] == t[3:5]                                 # grid, block
            runs = int(o[3]) and (512 // 64) * 2                    # one group of 8 waves x 2 rollouts
            assert int(o[5]) == int(t[5]) + 4 * ((runs + 3) & ~3)   # LDS + the block's clearance run
        else:
            assert o[2:7] == t[2:7]


def test_an_engine_without_a_scene_is_described_as_before():
    for model, terms in (("arm", ()), ("arm", ("target_track",)), ("drone", ()), ("wholebody", ("center",)), ("quadrotor", ())):
        cfg = make_config(model, n_samples=256, n_horizon=32, cost_terms=terms)
        for path, n in ((0, 3), (2, 3)):
            assert _launches(cfg, None, path=path, n=n) == _launches(cfg, plain=True, path=path, n=n)
