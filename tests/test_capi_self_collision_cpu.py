"""Self-collision avoidance (mppi_create_scene_self) without a GPU: the exports and the binding, every error
of a pair list through the host-side layout path (mppi_debug_self_layout: validate, scene_validate,
self_validate, self_layout, self_table, as tools/self_collision_host_check.cpp reaches them), the default
pairs, the table's index mapping, the self launchers' kernel choice (mppi_debug_self_rollout_kernels), the
argument layout of a self engine's step launches (mppi_debug_self_step_launches), the block rule and the
drop-in plumbing.  Engines without pairs get the symbols and descriptions they had.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import pose_envelope as PE
import test_capi_obstacles_cpu as TC
from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd import build as B
from quadrotor_manipulator_mppi_amd.engine import Scene, SelfCollision, make_config

ROOT = TC.ROOT
DRONE, ARM, WB, QUAD = TC.DRONE, TC.ARM, TC.WB, TC.QUAD
HDR_W, MEM, PAIR, WORD = 120, 8, 24, 7   # csrc/mppi_self.h
NEW = ("mppi_self_collision_default", "mppi_create_scene_self", "mppi_get_self_clearances", "mppi_get_plan_self_clearance")
NEW_DEBUG = ("mppi_debug_self_layout", "mppi_debug_self_rollout_kernels", "mppi_debug_self_step_launches")
# nine body spheres on the Kinova chain's frames -1 .. 7 (tests/test_gpu_obstacles.py ARM_BODY)
ARM_BODY = ((-1, (0.0, 0.0, -0.05), 0.09), (0, (0.0, 0.02, 0.08), 0.07), (1, (0.0, 0.0, 0.0), 0.05),
            (2, (0.0, -0.1, 0.0), 0.05), (3, (0.0, 0.03, -0.04), 0.05), (4, (0.0, 0.1, 0.0), 0.05),
            (5, (0.0, 0.0, 0.0), 0.05), (6, (0.0, 0.0, 0.0), 0.05), (7, (0.0, 0.0, -0.1), 0.04))
PAIRS = ((0, 5), (1, 6), (2, 7), (3, 8), (0, 8))


def _bind(name):
    f = getattr(capi.lib(), name)
    f.restype, f.argtypes = capi.DEBUG_PROTOTYPES[name]
    return f


def _err():
    return capi.lib().mppi_last_error().decode()


def _layout(cfg, scene, sc, full=False):
    f = _bind("mppi_debug_self_layout")
    s = None if scene is None else (scene.to_c() if isinstance(scene, Scene) else scene)
    p = sc.to_c() if isinstance(sc, SelfCollision) else sc
    table, region, out = np.zeros(TC.BODY_W, np.float32), np.zeros(HDR_W, np.float32), (C.c_int32 * 8)()
    st = f(C.byref(cfg), None if s is None else C.byref(s), None if p is None else C.byref(p), capi.fptr(table), capi.fptr(region), out)
    return (st, table, region, list(out)) if full else st


# ------------------------------------------------------------------------- exports and binding
def test_exports_and_binding():
    with open(os.path.join(ROOT, "include", "mppi_hip.h")) as f:
        header = f.read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in capi.PROTOTYPES, name
    for name in NEW_DEBUG:
        assert hasattr(L, name) and name in capi.DEBUG_PROTOTYPES and not re.search(r"\b%s\b" % name, header), name
    assert re.search(r"#define\s+MPPI_MAX_SELF_PAIRS\s+32", header) and capi.MAX_SELF_PAIRS == 32
    assert re.search(r"#define\s+MPPI_ABI_VERSION\s+10\b", header) and L.mppi_abi_version() == 10
    assert C.sizeof(capi.SelfCollision) == 4 + 256 + 16
    assert C.sizeof(capi.Scene) == 4 + 16 * 20 + 12 and C.sizeof(capi.FieldDesc) == 32   # no existing struct grew


# ---------------------------------------------------------------------------------- validation
def test_pair_list_errors_name_the_pair():
    cfg = make_config("arm", n_samples=64, n_horizon=32)
    scene = Scene(ARM_BODY)
    ok = SelfCollision(PAIRS)
    assert _layout(cfg, scene, ok) == capi.OK, _err()
    assert _layout(cfg, scene, SelfCollision(())) == capi.OK            # an empty list: a self engine that meets nothing
    assert _layout(cfg, scene, None) == capi.ERR_INVALID_ARG            # self NULL
    c = ok.to_c()
    for n in (-1, 33):
        c.n_pairs = n
        assert _layout(cfg, scene, c) == capi.ERR_INVALID_ARG and "n_pairs" in _err()
    bad = {"index": ((0, 5), (1, 9)), "index-neg": ((0, 5), (-1, 6)), "itself": ((0, 5), (4, 4)), "repeats": ((0, 5), (1, 6), (5, 0)),
           "rigid": ((0, 5), (0, 1))}
    for what, pairs in bad.items():
        assert _layout(cfg, scene, SelfCollision(pairs)) == capi.ERR_INVALID_ARG, what
        a, b = pairs[-1]
        assert f"pair {len(pairs) - 1} ({a}, {b})" in _err(), (what, _err())
    assert "rigid" in _err()
    for kw in (dict(w_self=-1.0), dict(margin=-0.01), dict(penalty=-1.0), dict(w_self=math.nan), dict(margin=math.inf), dict(penalty=math.nan)):
        assert _layout(cfg, scene, SelfCollision(PAIRS, **kw)) == capi.ERR_INVALID_ARG, kw
    # 32 pairs are accepted: every moving pair of the nine spheres but four
    many = [(a, b) for a in range(9) for b in range(a + 1, 9) if (a, b) != (0, 1)][:32]
    assert len(many) == 32 and _layout(cfg, scene, SelfCollision(many)) == capi.OK, _err()


def test_rigid_pairs_on_both_chains():
    """Frames -1 and 0 of the Kinova chain (joint 0 is fixed and folded into the base slot), and the two
    sides of the generic chain's mid-chain fixed joints."""
    cfg = make_config("arm", n_samples=64, n_horizon=32)
    two = lambda fa, fb: Scene(((fa, (0.0, 0.0, 0.0), 0.05), (fb, (0.0, 0.1, 0.0), 0.05)))  # noqa: E731
    assert _layout(cfg, two(-1, 0), SelfCollision(((0, 1),))) == capi.ERR_INVALID_ARG and "rigid" in _err()
    assert _layout(cfg, two(0, 1), SelfCollision(((0, 1),))) == capi.OK
    gen = make_config("arm", n_samples=64, n_horizon=32, chain=PE.GENERIC_CHAIN)
    for fa, fb, rigid in ((2, 3, True), (6, 7, True), (-1, 0, True), (3, 2, True), (1, 2, False), (3, 4, False), (5, 6, False),
                          (1, 3, False), (2, 9, False)):
        st = _layout(gen, two(fa, fb), SelfCollision(((0, 1),)))
        assert st == (capi.ERR_INVALID_ARG if rigid else capi.OK), (fa, fb, _err())


def test_models():
    """ARM and WHOLEBODY; DRONE has no chain (every pair would be rigid), QUADROTOR no scene."""
    for model, st in (("arm", capi.OK), ("wholebody", capi.OK), ("drone", capi.ERR_INVALID_ARG), ("quadrotor", capi.ERR_INVALID_ARG)):
        cfg = make_config(model, n_samples=64, n_horizon=32)
        assert _layout(cfg, None, SelfCollision(())) == st, (model, _err())


def test_default_pairs():
    """Every pair with at least three moving joints between its frames, in (a, b) order: 10 for the
    default arm scene, 15 for the default whole-body scene; the project's weights."""
    from quadrotor_manipulator_mppi_amd.robot import body_spheres as BS
    assert (BS.W_SELF, BS.MARGIN_SELF, BS.PENALTY_SELF) == (100.0, 0.02, 1e4)
    for model, n in (("arm", 10), ("wholebody", 15)):
        cfg = make_config(model, n_samples=64, n_horizon=32)
        scene = Scene.default(cfg)
        d = SelfCollision.default(cfg)
        assert d == SelfCollision.default(cfg, scene) and hash(d) == hash(SelfCollision.default(cfg, scene))
        assert len(d.pairs) == n, (model, d.pairs)
        assert (d.w_self, round(d.margin, 6), d.penalty) == (100.0, 0.02, 1e4)
        moving = [j for j in range(cfg.n_joints) if cfg.joints[j].type != capi.JOINT_FIXED]
        sep = lambda fa, fb: sum(1 for j in moving if min(fa, fb) < j <= max(fa, fb))  # noqa: E731
        want = [(a, b) for a in range(len(scene.body)) for b in range(a + 1, len(scene.body))
                if sep(scene.body[a][0], scene.body[b][0]) >= 3]
        assert list(d.pairs) == want
        assert _layout(cfg, scene, d) == capi.OK, _err()
    # truncated at 32, still in order
    cfg = make_config("arm", n_samples=64, n_horizon=32)
    body = tuple((1 + (i % 7), (0.0, 0.0, 0.01 * i), 0.03) for i in range(16))
    d = SelfCollision.default(cfg, Scene(body))
    assert len(d.pairs) == 32 and list(d.pairs) == sorted(d.pairs)


def test_table_maps_indices_through_the_sort_order():
    """The shuffled body of test_body_table_folds_and_sorts (sorted order 1, 3, 5, 2, 4, 0): members are
    numbered in sorted order, a sphere in no pair is -1, every row names its spheres' members and the sum
    of their radii; the region's offset sits in the body table's spare word."""
    cfg = make_config("arm", n_samples=64, n_horizon=32)
    body = ((7, (0.0, 0.0, -0.1), 0.04), (0, (0.0, 0.02, 0.08), 0.07), (3, (0.01, 0.0, 0.0), 0.05),
            (-1, (0.0, 0.0, -0.05), 0.09), (3, (0.0, 0.03, 0.0), 0.06), (1, (0.0, 0.0, 0.0), 0.05))
    scene = Scene(body, w_obs=7.0, margin=0.1, penalty=3.0)
    pairs = ((0, 3), (4, 1), (0, 5))   # spheres 0, 1, 3, 4, 5 are members; 2 is not
    st, table, region, out = _layout(cfg, scene, SelfCollision(pairs, w_self=9.0, margin=0.03, penalty=5.0), full=True)
    assert st == capi.OK, _err()
    st0, t0, order = TC._layout(cfg, scene, table=True)
    order = order[:6]
    assert order == [1, 3, 5, 2, 4, 0]
    w, r = table.view(np.int32), region.view(np.int32)
    same = np.ones(TC.BODY_W, bool)
    same[WORD] = False
    assert np.array_equal(table.view(np.uint32)[same], t0.view(np.uint32)[same]) and t0.view(np.int32)[WORD] == 0
    # sorted positions 0..5 hold spheres 1, 3, 5, 2, 4, 0 -> members 0, 1, 2, -1, 3, 4
    assert list(r[MEM:MEM + 16]) == [0, 1, 2, -1, 3, 4] + [-1] * 10
    member = {1: 0, 3: 1, 5: 2, 4: 3, 0: 4}
    assert r[0] == 3 and (region[1], region[2], region[3]) == (9.0, np.float32(0.03), 5.0) and r[4] == 5 == out[1]
    for i, (a, b) in enumerate(pairs):
        assert (r[PAIR + 3 * i], r[PAIR + 3 * i + 1]) == (member[a], member[b])
        assert region[PAIR + 3 * i + 2] == np.float32(body[a][2]) + np.float32(body[b][2])
    assert not region[PAIR + 9:].any()
    # the layout: the region behind a scene engine's buffer, 256 B aligned runs
    al = lambda n: (n + 63) & ~63  # noqa: E731
    V, K, H = 1, 64, 32
    scene_words = al(92 + 132 * V) + al(V * K) + al(V * H)
    assert w[WORD] == out[3] == scene_words
    assert r[5] == scene_words + al(HDR_W) and r[6] == r[5] + al(V * K) and out[4] == r[6] + al(V * H)


# ---------------------------------------------------------------------------- rollout symbols
def _kernels(model, A, H, V=1, f64=0, cost_terms=0, iters=1, threads=256, field=0, members=9):
    f = _bind("mppi_debug_self_rollout_kernels")
    seg, nch = (32 if H <= 32 else 64), (1 if H <= 64 else 2 if H <= 128 else 4)
    g = (C.c_int32 * 17)(model, A, H, seg, nch, iters, threads, V, f64, capi.NOISE_PHILOX, 0, cost_terms, 0, 0, 0, field, members)
    full, quiet = C.create_string_buffer(192), C.create_string_buffer(192)
    st = f(g, full, quiet, 192)
    return st, full.value.decode(), quiet.value.decode(), seg, nch


UNITS = {0: "mppi_rollout_sc.hip", 1: "mppi_rollout_sf.hip"}
ROWS = [(ARM, 7, 0), (ARM, 7, 1), (WB, 10, 0)]
CASES = [(m, A, f, H, V) for m, A, f in ROWS for H in (20, 32, 64, 128, 200) for V in (1, 3)]
_blobs = {}


def _blob(unit):
    if unit not in _blobs:
        with open(B.code_object_path(B.LIB, unit), "rb") as f:
            _blobs[unit] = f.read()
    return _blobs[unit]


@pytest.mark.parametrize("model,A,f64,H,V", CASES, ids=[f"m{m}-f{f}-H{H}-V{V}" for m, _, f, H, V in CASES])
def test_self_symbols(model, A, f64, H, V):
    for field in (0, 1):
        name = "k_rollout_sf" if field else "k_rollout_sc"
        for terms in (0, 32, 32 | capi.COST_CENTER):
            st, full, quiet, seg, nch = _kernels(model, A, H, V=V, f64=f64, cost_terms=terms, field=field, threads=64)
            assert st == 0 and full == quiet, "self engines run the full kernel on every step"
            assert full.startswith(f"_Z12{name}ILi{model}ELi{A}ELi{nch}ELi{seg}ELb{f64}ELb{int(V == 1)}EEv"), full
            holders = [u for u in B.KERNEL_UNITS if (full + ".kd").encode() in _blob(u)]
            assert holders == [UNITS[field]], (full, holders)
    # the scene, field and plain engines' symbols as they were
    for hook, tag in (("mppi_debug_scene_rollout_kernels", "k_rollout_ob"), ("mppi_debug_field_rollout_kernels", "k_rollout_df"),
                      ("mppi_debug_rollout_kernels", "k_rollout")):
        st, full, quiet, _, _ = TC._kernels(hook, model, A, H, V=V, f64=f64)
        assert st == 0 and tag in full and "_sc" not in full and "_sf" not in full and "_sc" not in quiet and "_sf" not in quiet


@pytest.mark.parametrize("unit", sorted(UNITS.values()))
def test_self_kernels_reserve_no_private_segment(unit):
    """Every symbol of the two self units: private segment (scratch) 0 and no spilled VGPR, from the code
    object's own metadata -- what a dispatch reserves, whether or not an instruction addresses it; 24
    symbols per unit; static LDS within the bound the block rule adds."""
    res = B.kernel_resources(B.code_object_path(B.LIB, unit))
    name = "k_rollout_sf" if unit.endswith("sf.hip") else "k_rollout_sc"
    mine = {k: v for k, v in res.items() if name in k}
    assert len(mine) == 24 and len(res) == 24, sorted(res)
    bad = {k: v for k, v in mine.items() if v["scratch"] != 0 or v["vspill"] != 0}
    assert not bad, bad
    assert all(v["lds"] <= 4096 for v in mine.values())


def test_no_drone_or_quadrotor_self_kernel():
    assert _kernels(DRONE, 3, 32)[0] == capi.ERR_INVALID_ARG
    assert _kernels(QUAD, 4, 32)[0] == capi.ERR_INVALID_ARG


def test_self_kernel_blocks():
    """Blocks of 64 .. 256 threads, one group or a loop of them; 512 threads and more than 16 members have no launch."""
    for kw in (dict(iters=16, threads=128), dict(iters=3), dict(threads=64, members=16), dict(threads=256, members=0)):
        st, full, quiet, _, _ = _kernels(ARM, 7, 32, f64=1, **kw)
        assert st == 0 and full == quiet and full.startswith("_Z12k_rollout_scILi1ELi7ELi1ELi32ELb1ELb1EEv"), kw
    assert _kernels(ARM, 7, 32, f64=1, threads=512)[0] == capi.ERR_INVALID_ARG
    assert _kernels(ARM, 7, 32, f64=1, members=17)[0] == capi.ERR_INVALID_ARG


# ---------------------------------------------------------------------------- argument layout
def _launches(cfg, scene, sc, field=None, **sw):
    words = (C.c_int32 * len(TC.SW_ORDER))(*[sw.get(k, 0) for k in TC.SW_ORDER])
    buf = C.create_string_buffer(4096)
    s, p = scene.to_c(), sc.to_c()
    fd = None if field is None else field.to_c()
    st = _bind("mppi_debug_self_step_launches")(C.byref(cfg), C.byref(s), None if fd is None else C.byref(fd), C.byref(p), words, buf, len(buf))
    assert st == capi.OK, _err()
    return [TC.LINE.fullmatch(ln).groups() for ln in buf.value.decode().splitlines()]


def _field_launches(cfg, scene, field, **sw):
    words = (C.c_int32 * len(TC.SW_ORDER))(*[sw.get(k, 0) for k in TC.SW_ORDER])
    buf = C.create_string_buffer(4096)
    s, fd = scene.to_c(), field.to_c()
    st = _bind("mppi_debug_field_step_launches")(C.byref(cfg), C.byref(s), C.byref(fd), words, buf, len(buf), None)
    assert st == capi.OK, _err()
    return [TC.LINE.fullmatch(ln).groups() for ln in buf.value.decode().splitlines()]


@pytest.mark.parametrize("path,n", [(0, 3), (2, 3), (3, 1)], ids=["hip-batch", "native-batch", "native-call"])
@pytest.mark.parametrize("with_field", [False, True], ids=["scene", "field"])
def test_step_launches_of_a_self_engine(path, n, with_field):
    """HIP batch, native batch, native call: the self rollout on every step with the grid and block of the
    scene (field) engine of the same block size, an argument block of the same size -- the pair region needs
    no pointer of its own -- and the LDS of self_dyn_lds; the finalize as that engine's."""
    from quadrotor_manipulator_mppi_amd.engine import DistanceField
    kw = dict(n_samples=256, n_horizon=32)
    cfg = make_config("arm", **kw)
    scene, sc = Scene(ARM_BODY), SelfCollision(PAIRS)
    field = DistanceField((8, 8, 8), 0.25) if with_field else None
    st, _, _, out = _layout(cfg, scene, sc, full=True)
    threads, members, lds = out[0], out[1], out[2]
    assert st == capi.OK and threads == 256 and members == 8
    got = _launches(cfg, scene, sc, field, path=path, n=n)
    cfg_b = make_config("arm", block_threads=threads, **kw)
    ref = _field_launches(cfg_b, scene, field, path=path, n=n) if with_field else TC._launches(cfg_b, scene, path=path, n=n)
    assert len(got) == len(ref) == (4 if n > 1 else 2)
    for g, r in zip(got, ref):
        assert g[:2] == r[:2]
        if g[1] == "rollout":
            assert ("k_rollout_sf" if with_field else "k_rollout_sc") in g[2] and ("k_rollout_df" if with_field else "k_rollout_ob") in r[2]
            assert g[3:5] == r[3:5] and int(g[4]) == threads          # grid, block
            assert int(g[6]) <= int(r[6])                              # argument bytes
            runs = (threads // 64) * 2                                 # one group of 4 waves x 2 rollouts
            assert int(g[5]) == lds == int(r[5]) + 4 * ((runs + 3) & ~3) + 4 * 3 * members * threads
            assert int(g[5]) + out[7] <= 64 * 1024
        else:
            assert g[2:7] == r[2:7]


def test_engines_without_pairs_are_described_as_before():
    """A scene engine and a plain engine: the existing hooks' answers (the hooks share the builder the self
    hook extends), the block of 512 threads, and a body table whose spare word stays 0."""
    for model, terms in (("arm", ()), ("arm", ("target_track",)), ("wholebody", ("center",))):
        cfg = make_config(model, n_samples=256, n_horizon=32, cost_terms=terms)
        for path, n in ((0, 3), (2, 3)):
            plain = TC._launches(cfg, plain=True, path=path, n=n)
            assert TC._launches(cfg, None, path=path, n=n) == plain
            sc = TC._launches(cfg, Scene.default(cfg), path=path, n=n)
            assert all(ln[4] == "512" for ln in sc if ln[1] == "rollout") and all("k_rollout_ob" in ln[2] for ln in sc if ln[1] == "rollout")
            assert all("_sc" not in ln[2] and "_sf" not in ln[2] for ln in sc + plain)
        st, t, _ = TC._layout(cfg, Scene.default(cfg), table=True)
        assert st == capi.OK and t.view(np.int32)[WORD] == 0


def test_block_rule():
    """The centre column is 12 B per member and thread: block_threads = 0 picks the largest of 256, 128, 64
    that keeps the block within 64 KiB; an explicit block the kernel cannot serve is refused with a message."""
    scene16 = Scene(tuple((1 + (i % 7), (0.0, 0.0, 0.01 * i), 0.03) for i in range(16)))
    all16 = SelfCollision.default(make_config("arm", n_samples=64, n_horizon=32), scene16)
    assert len({i for p in all16.pairs for i in p}) == 16
    for kw, sc, scene, want in ((dict(), SelfCollision(PAIRS), Scene(ARM_BODY), 256), (dict(), all16, scene16, 128),
                                (dict(block_threads=128), SelfCollision(PAIRS), Scene(ARM_BODY), 128),
                                (dict(block_threads=64), all16, scene16, 64), (dict(n_horizon=200), all16, scene16, 64)):
        cfg = make_config("arm", **{**dict(n_samples=256, n_horizon=32), **kw})
        st, _, _, out = _layout(cfg, scene, sc, full=True)
        assert st == capi.OK and out[0] == want, (kw, out, _err())
        if cfg.n_horizon <= 128:
            assert out[2] + out[7] <= 64 * 1024
    cfg = make_config("arm", n_samples=256, n_horizon=32, block_threads=512)
    assert _layout(cfg, Scene(ARM_BODY), SelfCollision(PAIRS)) == capi.ERR_INVALID_ARG and "block_threads 512" in _err()
    cfg = make_config("arm", n_samples=256, n_horizon=32, block_threads=256)
    assert _layout(cfg, scene16, all16) == capi.ERR_INVALID_ARG and "block_threads 256" in _err() and "LDS" in _err()
    # the same configurations without pairs keep their 512-thread block
    st, t, _ = TC._layout(make_config("arm", n_samples=256, n_horizon=32), scene16, table=True)
    assert st == capi.OK


# ------------------------------------------------------------------------------- drop-in plumbing
class _FakeEngine:
    made = []

    def __init__(self, cfg, **kw):
        self.cfg, self.kw = cfg, kw
        _FakeEngine.made.append(self)

    def set_u_prev(self, u):
        pass

    def get_u_prev(self):
        return np.zeros((1, self.cfg.n_horizon, self.cfg.n_action), np.float32)

    def get_self_clearances(self):
        return np.full((1, self.cfg.n_samples), 0.25, np.float32)

    def close(self):
        pass


def test_dropin_arm_class_forwards_the_pairs(monkeypatch):
    from quadrotor_manipulator_mppi_amd.mppi_solver import _base
    from quadrotor_manipulator_mppi_amd.mppi_solver.mppi import MPPI
    monkeypatch.setattr(_base, "Engine", _FakeEngine)
    _FakeEngine.made.clear()
    scene, sc = Scene(ARM_BODY), SelfCollision(PAIRS)
    for arg, want in ((sc, sc), (True, None)):
        m = MPPI(n_samples=64, n_horizon=16, verbose=False, scene=scene, self_collision=arg)
        e = m._ensure_engine(m._engine_key if m._engine_key is not None else (64, 16))
        assert set(e.kw) == {"scene", "field", "self_collision"} and e.kw["scene"] == scene and e.kw["field"] is None
        got = e.kw["self_collision"]
        assert got == (want if want is not None else SelfCollision.default(e.cfg, scene))
        assert m.get_self_clearances().shape == (64,)
        assert m._ensure_engine(m._engine_key[0]) is e          # the same key: the same engine
    # without scene=: the placeholder spheres and their pairs
    m = MPPI(n_samples=64, n_horizon=16, verbose=False, self_collision=True)
    e = m._ensure_engine((64, 16))
    assert e.kw["scene"] == Scene.default(e.cfg) and len(e.kw["self_collision"].pairs) == 10
    # no pairs: the constructor calls as they were, no new keyword
    _FakeEngine.made.clear()
    m = MPPI(n_samples=64, n_horizon=16, verbose=False, scene=scene)
    assert m._ensure_engine((64, 16)).kw == {"scene": scene, "field": None}
    m = MPPI(n_samples=64, n_horizon=16, verbose=False)
    assert m._ensure_engine((64, 16)).kw == {}
    with pytest.raises(RuntimeError):
        m.get_self_clearances()


def test_drone_and_quadrotor_classes_refuse_pairs():
    from quadrotor_manipulator_mppi_amd.mppi_solver import drone_mppi, quadrotor_mppi
    for mod in (drone_mppi, quadrotor_mppi):
        with pytest.raises(NotImplementedError):
            mod.MPPI(self_collision=True)
        with pytest.raises(NotImplementedError):
            mod.MPPI(self_collision=SelfCollision(()))
