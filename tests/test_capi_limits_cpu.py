"""Rotor limits (mppi_create_limits, mppi_set_limits, mppi_limits_apply) without a GPU: the exports and the
binding, the numpy oracle of the four lines (tests/limits_oracle.py), the host replay (the kernels' own inline,
csrc/mppi_limits.h) against it bit for bit, every refusal, the launches a bounded engine's step paths describe
(mppi_debug_limits_step_launches), the plain kernels' symbols as they were, and the condition the GPU tests'
designs are held to: with the bounds at the 15th and 85th percentile of fl(u + eps), between 10% and 20% of
(k, t) saturate on each side of every bounded dim -- a kernel that ignores a side fails, and no case is all clamp.

A dim whose noise scale is 0 in a design (free_fall's thrust: every a0 is the same number, so no percentile
separates anything) is left unbounded in that design; its other dims are bounded and held to the condition.
"""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import aerial_oracle as A
import limits_oracle as LO
import quad_oracle as Q
from conftest import GOLDEN, ROOT
from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd import build as B
from quadrotor_manipulator_mppi_amd.engine import Limits, limits_apply, make_config

NEW = ("mppi_limits_default", "mppi_create_limits", "mppi_set_limits", "mppi_get_limits", "mppi_limits_apply")
DEBUG = ("mppi_debug_limits_step_launches", "mppi_debug_limits_plan_kernel", "mppi_debug_limits_set")
INF = float("inf")
K, H = 64, 32


def _bind(name):
    f = getattr(capi.lib(), name)
    f.restype, f.argtypes = capi.DEBUG_PROTOTYPES[name]
    return f


def _err():
    return capi.lib().mppi_last_error().decode()


# ------------------------------------------------------------------------- exports and the Python surface
def test_exports_and_binding():
    with open(os.path.join(ROOT, "include", "mppi_hip.h")) as f:
        header = f.read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in capi.PROTOTYPES, name
    for name in DEBUG:
        assert hasattr(L, name) and name in capi.DEBUG_PROTOTYPES and not re.search(r"\b%s\b" % name, header), name
    assert re.search(r"typedef struct \{ float lo\[4\], hi\[4\]; \} mppi_limits;", header)
    assert re.search(r"#define\s+MPPI_ABI_VERSION\s+10\b", header) and L.mppi_abi_version() == 10 == capi.ABI_VERSION
    assert C.sizeof(capi.Limits) == 32
    sizes = [C.c_int32(), C.c_int32(), C.c_int32()]
    L.mppi_struct_sizes(*[C.byref(s) for s in sizes])
    assert tuple(s.value for s in sizes) == (C.sizeof(capi.Config), C.sizeof(capi.Joint), C.sizeof(capi.Stats))   # mppi_config unchanged


def test_default_limits_and_the_python_object():
    for model in ("quadrotor", "aerial"):
        cfg = make_config(model, quad=dict(quad_mass=2.5, quad_gravity=9.81))
        d = Limits.default(cfg)
        assert d.thrust == (0.0, float(np.float32(2.0) * (np.float32(2.5) * np.float32(9.81))))
        assert d.torque == ((-INF, INF),) * 3
    a = Limits(thrust=(0.0, 50.0), torque=((-1.0, 1.0), (-2.0, 2.0), (-INF, 0.5)))
    assert a == Limits.from_c(a.to_c()) and hash(a) == hash(Limits.from_c(a.to_c())) and a != Limits()
    assert np.array_equal(a.lo, np.float32([0, -1, -2, -INF])) and np.array_equal(a.hi, np.float32([50, 1, 2, 0.5]))
    with pytest.raises(ValueError):
        Limits(torque=((-1.0, 1.0),) * 2)


def test_dropin_classes_take_the_keyword():
    from quadrotor_manipulator_mppi_amd.mppi_solver import aerial_mppi, drone_mppi, quadrotor_mppi
    for mod in (quadrotor_mppi, aerial_mppi):
        m = mod.MPPI(limits=True)
        assert m.get_limits() is True
        lim = Limits(thrust=(0.0, 200.0))
        m.set_limits(lim)
        assert m.get_limits() is lim
        with pytest.raises(TypeError):
            m.set_limits((0.0, 1.0))
        plain = mod.MPPI()
        assert plain.get_limits() is None
        with pytest.raises(RuntimeError, match="limits="):
            plain.set_limits(lim)
    with pytest.raises(TypeError):
        drone_mppi.MPPI(limits=True)   # (the point-mass drone's outputs are the finalize's: no limits)


# ------------------------------------------------------------------------------------------ the oracle itself
def test_oracle_on_hand_cases():
    f = np.float32
    u = f([[100.0, 0.0, 0.0, 0.0], [0.1, 0.0, 0.0, 0.0]])
    eps = f([[[-150.0, 0.5, -0.5, 0.0], [0.2, 3.0, -3.0, 1.0]]])
    lo, hi = f([0.0, -1.0, -1.0, -INF]), f([120.0, 1.0, 1.0, INF])
    ap = LO.apply(u, eps, lo, hi)
    assert np.array_equal(ap.ctl[0, 0], f([0.0, 0.5, -0.5, 0.0])) and np.array_equal(ap.eps_eff[0, 0], f([-100.0, 0.5, -0.5, 0.0]))
    assert np.array_equal(ap.ctl[0, 1], f([f(0.1) + f(0.2), 1.0, -1.0, 1.0])) and np.array_equal(ap.eps_eff[0, 1], f([0.2, 1.0, -1.0, 1.0]))
    assert np.array_equal(ap.low, [0.5, 0.0, 0.5, 0.0]) and np.array_equal(ap.high, [0.0, 0.5, 0.0, 0.0])
    # fl(u + fl(v' - u)) can miss the bound by an ulp; the control does not
    rng = np.random.default_rng(3)
    uu = rng.normal(0.0, 50.0, (4096, 4)).astype(f)
    hh = f([150.0, 1.0, 1.0, 1.0]) * f(1.0000001)
    over = (uu + (hh - uu)) > hh
    assert over.any(), "no (u, hi) pair of this draw lands above the bound"
    ap = LO.apply(uu, np.full((1, 4096, 4), 1e4, f), f([-INF] * 4), hh)
    assert np.array_equal(ap.eps_eff[0], hh - uu) and ap.high.min() == 1.0
    assert (ap.ctl[0] <= hh).all() and (ap.ctl[0][over] == np.broadcast_to(hh, uu.shape)[over]).all()
    assert (np.abs(ap.ctl[0] - hh) <= np.spacing(np.maximum(np.abs(uu), hh))).all()


# --------------------------------------------------------------------------------------------- the designs
def _quad_cases():
    for d in Q.DESIGNS:
        u, eps = d.inputs(K, H)
        yield "quad-" + d.name, u, eps, np.float32(d.sigma)


def _aerial_cases():
    for d in A.DESIGNS:
        u, eps = d.inputs(K, H)
        yield "aerial-" + d.name, u[:, :4], eps[..., :4], np.float32(d.sigma[:4])


design_bounds = LO.design_bounds
CASES =list(_quad_cases()) + list(_aerial_cases())


@pytest.mark.parametrize("name,u,eps,sigma", CASES, ids=[c[0] for c in CASES])
def test_design_condition_and_host_replay(name, u, eps, sigma):
    lo, hi, bounded = design_bounds(u, eps, sigma)
    assert bounded.sum() >= 3, name
    ap = LO.apply(u, eps, lo, hi)
    for a in range(4):
        if bounded[a]:
            assert 0.10 <= ap.low[a] <= 0.20 and 0.10 <= ap.high[a] <= 0.20, (name, LO.DIMS[a], ap.low[a], ap.high[a])
        else:
            assert ap.low[a] == ap.high[a] == 0.0
    assert (ap.ctl >= lo).all() and (ap.ctl <= hi).all()
    sat = (u[None] + eps != ap.ctl)
    assert np.array_equal(ap.eps_eff[~sat], eps[~sat]), "an unsaturated draw is untouched"
    lim = Limits((lo[0], hi[0]), tuple((lo[a], hi[a]) for a in (1, 2, 3)))
    e, c = limits_apply(lim, u, eps)
    assert e.dtype == c.dtype == np.float32
    assert np.array_equal(e.view(np.uint32), ap.eps_eff.view(np.uint32)), name
    assert np.array_equal(c.view(np.uint32), ap.ctl.view(np.uint32)), name
    # infinite bounds: eps as given, c = fl(u + eps)
    e, c = limits_apply(Limits(), u, eps)
    assert np.array_equal(e.view(np.uint32), eps.view(np.uint32)) and np.array_equal(c, u[None] + eps)


def test_thrust_floor_alone_saturates_on_a_design_whose_draws_go_negative():
    """Thrust in [0, +inf), everything else open: body2 (m g = 4.45 N under sigma 3 N) draws negative thrust."""
    d = Q.BY_NAME["body2"]
    u, eps = d.inputs(K, H)
    lim = Limits(thrust=(0.0, INF))
    ap = LO.apply(u, eps, lim.lo, lim.hi)
    assert ap.low[0] >= 0.05 and ap.high.max() == 0.0 and ap.low[1:].max() == 0.0, ap.low
    assert (ap.ctl[..., 0] >= 0).all() and np.array_equal(ap.ctl[..., 1:], (u[None] + eps)[..., 1:])
    e, c = limits_apply(lim, u, eps)
    assert np.array_equal(e.view(np.uint32), ap.eps_eff.view(np.uint32)) and np.array_equal(c.view(np.uint32), ap.ctl.view(np.uint32))


# ----------------------------------------------------------------------------------------------- refusals
SW_ORDER = ("path", "n", "peer", "comm", "timing", "generic", "out_dbg")
LINE = re.compile(r"(early|last) (rollout|pack|finalize) (\S+) grid (\d+) block (\d+) lds (\d+) args (\d+) fnv ([0-9a-f]{16})")


def _launches(cfg, limits=None, plain=False, status=False, **sw):
    words = (C.c_int32 * len(SW_ORDER))(*[sw.get(k, 0) for k in SW_ORDER])
    buf = C.create_string_buffer(4096)
    if plain:
        st = _bind("mppi_debug_step_launches")(C.byref(cfg), words, buf, len(buf))
    else:
        lc = None if limits is None else C.byref(limits.to_c())
        st = _bind("mppi_debug_limits_step_launches")(C.byref(cfg), lc, words, buf, len(buf))
    if status:
        return st
    assert st == capi.OK, _err()
    return [LINE.fullmatch(ln).groups() for ln in buf.value.decode().splitlines()]


def test_refusals_name_what_is_wrong():
    quad = make_config("quadrotor", n_samples=64, n_horizon=20)
    nan = float("nan")
    for a, name in enumerate(LO.DIMS):
        for bad in ((nan, 1.0), (0.0, nan), (1.0, 0.5), (INF, -INF)):
            pairs = [(-1.0, 1.0)] * 4
            pairs[a] = bad
            lim = Limits(pairs[0], tuple(pairs[1:]))
            assert _launches(quad, lim, status=True, path=0, n=1) == capi.ERR_INVALID_ARG
            assert name in _err() and f"dim {a}" in _err(), _err()
            assert _bind("mppi_debug_limits_set")(C.byref(quad), 1, C.byref(lim.to_c())) == capi.ERR_INVALID_ARG and name in _err()
            e = np.zeros((1, 1, 4), np.float32)
            with pytest.raises(capi.MPPIError, match=name):
                limits_apply(lim, e[0], e)
    assert _launches(quad, Limits((0.0, 0.0), ((-INF, INF),) * 3), path=0, n=1)   # lo == hi is a bound
    for model in ("drone", "arm", "wholebody"):
        assert _launches(make_config(model, n_samples=64), Limits(), status=True, path=0, n=1) == capi.ERR_INVALID_ARG
        assert model.upper() in _err(), _err()
    assert _launches(make_config("quadrotor", n_samples=64, shard_rank=0, shard_count=2), Limits(), status=True, path=1, n=1) == \
        capi.ERR_INVALID_ARG
    assert "shard" in _err()
    # mppi_set_limits: MPPI_ERR_STATE on an engine created without limits, whatever the bounds
    for lim in (Limits(), Limits(thrust=(1.0, 0.0))):
        assert _bind("mppi_debug_limits_set")(C.byref(quad), 0, C.byref(lim.to_c())) == capi.ERR_STATE
        assert "mppi_create_limits" in _err()
    assert _bind("mppi_debug_limits_set")(C.byref(quad), 1, None) == capi.ERR_INVALID_ARG


# ----------------------------------------------------------------------------------------------- launches
def _template_args(sym, name):
    m = re.fullmatch(r"_Z\d+%s(I.*E)Ev.*" % name, sym)
    assert m, (sym, name)
    return m.group(1)


def _unit_blob(unit):
    with open(B.code_object_path(B.LIB, unit), "rb") as f:
        return f.read()


def _compare(cfg, plain_name, bounded_name, unit, path, n, block=None):
    lim = Limits.default(cfg)
    b, p = _launches(cfg, lim, path=path, n=n), _launches(cfg, None, path=path, n=n)
    assert p == _launches(cfg, plain=True, path=path, n=n), "without limits: what the plain listing lists"
    assert len(b) == len(p) == (4 if n > 1 else 2)
    blob = _unit_blob(unit)
    for x, y in zip(b, p):
        assert x[:2] == y[:2]
        if x[1] == "rollout":
            assert (x[2] + ".kd").encode() in blob, x[2]   # native dispatch finds it in the unit's code object
            if block is not None:
                assert int(x[4]) == block, x
            if y[0] == "last":   # (a plain quadrotor batch's early steps run the quiet form: another symbol, less LDS)
                assert _template_args(x[2], bounded_name) == _template_args(y[2], plain_name)
                assert x[3:6] == y[3:6], (x, y)            # grid, block, LDS
                assert int(x[6]) == int(y[6]) + 8, (x, y)  # + the limits pointer; the trailing DevParams as it was
        else:
            assert x[2:8] == y[2:8], (x, y)                # the finalize is the plain engine's, argument bytes included
    # no quiet form: every step of a batch runs the bounded kernel
    assert len({x[2] for x in b if x[1] == "rollout"}) == 1
    return b


@pytest.mark.parametrize("path,n", [(0, 3), (1, 1), (2, 3), (3, 1)], ids=["hip-batch", "hip-call", "native-batch", "native-call"])
def test_bounded_quadrotor_launches(path, n):
    cfg = make_config("quadrotor", n_samples=64, n_horizon=20)
    b = _compare(cfg, "k_rollout_quad", "k_rollout_quad_b", "mppi_rollout_quad.hip", path, n, block=512)
    assert all(x[2].startswith("_Z16k_rollout_quad_bILb1E") for x in b if x[1] == "rollout")
    trk = make_config("quadrotor", n_samples=64, n_horizon=20, cost_terms=("target_track",))
    b = _compare(trk, "k_rollout_quad_tt", "k_rollout_quad_tt_b", "mppi_rollout_quad.hip", path, n, block=512)
    assert all(x[2].startswith("_Z19k_rollout_quad_tt_bILb1E") for x in b if x[1] == "rollout")


AERIAL_FORMS = [("wide-512", dict(n_samples=256, n_horizon=32), "ILb1ELb0ELi1ELi512E", 512),
                ("narrow-256", dict(n_samples=4096, n_horizon=32, n_vehicles=3), "ILb0ELb0ELi1ELi256E", 256),
                ("four-wave-256", dict(n_samples=16400, n_horizon=20), "ILb1ELb0ELi4ELi256E", 256)]


@pytest.mark.parametrize("tag,kw,targs,block", AERIAL_FORMS, ids=[f[0] for f in AERIAL_FORMS])
def test_bounded_aerial_launches_at_each_block_form(tag, kw, targs, block):
    cfg = make_config("aerial", **kw)
    for path, n in ((0, 3), (2, 3)) + (((3, 1),) if cfg.n_vehicles == 1 else ()):
        b = _compare(cfg, "k_rollout_aerial", "k_rollout_aerial_b", "mppi_limits.hip", path, n, block=block)
        assert all(_template_args(x[2], "k_rollout_aerial_b") == targs for x in b if x[1] == "rollout"), b


def test_quadrotor_narrow_form_is_reached_at_k_8208():
    """The smallest K whose single-vehicle grid leaves the 512-thread form: more than 512 blocks of 16 rollouts."""
    for Kq, block in ((8192, 512), (8208, 256)):
        cfg = make_config("quadrotor", n_samples=Kq, n_horizon=32)
        b = _launches(cfg, Limits.default(cfg), path=1, n=1)
        assert int(b[0][4]) == block and "k_rollout_quad_b" in b[0][2], b


def test_bounded_plan_kernels():
    f, g = _bind("mppi_debug_limits_plan_kernel"), getattr(capi.lib(), "mppi_debug_plan_kernel")
    g.restype, g.argtypes = C.c_int32, [C.POINTER(C.c_int32), C.c_char_p, C.c_int32]
    blob, plain_blob = _unit_blob("mppi_limits.hip"), _unit_blob("mppi_plan.hip")
    for model, A_, name in ((capi.MODEL_QUADROTOR, 4, "k_plan_quad"), (capi.MODEL_AERIAL, 11, "k_plan_aerial")):
        for lit in (0, 1):
            words = (C.c_int32 * 6)(model, A_, 20, 2, 0, lit)
            sb, sp = C.create_string_buffer(256), C.create_string_buffer(256)
            assert f(words, sb, 256) == capi.OK and g(words, sp, 256) == capi.OK
            b, p = sb.value.decode().split(), sp.value.decode().split()
            assert b[1:] == p[1:] == ["grid", "2", "block", "64"]
            assert _template_args(b[0], name + "_b") == _template_args(p[0], name) == f"ILb{lit}E"
            assert (b[0] + ".kd").encode() in blob and (p[0] + ".kd").encode() in plain_blob and (b[0] + ".kd").encode() not in plain_blob
    for model, A_ in ((capi.MODEL_DRONE, 3), (capi.MODEL_ARM, 7), (capi.MODEL_WHOLEBODY, 10)):
        assert f((C.c_int32 * 6)(model, A_, 20, 1, 0, 0), C.create_string_buffer(256), 256) == capi.ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------ symbols
def test_plain_symbols_are_still_there_under_their_old_names():
    """nm on the built library: every quadrotor and aerial rollout symbol the recorded step launches name
    (tests/golden/step_launches.json, recorded before limits), and the aerial kernels' twelve instantiations."""
    nm = shutil.which("nm") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", B.LIB], capture_output=True, text=True, check=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    with open(os.path.join(GOLDEN, "step_launches.json")) as f:
        recorded = [s for s in json.load(f)["symbols"] if "k_rollout_quad" in s]
    assert len(recorded) >= 4 and all(s in have for s in recorded), [s for s in recorded if s not in have]
    tail = "EvjjjjiiPKfN4mppi9DevParamsE"
    forms = [(nw, nt) for nw, nt in ((1, 512), (1, 256), (4, 256))]
    for vone in (0, 1):
        for lit in (0, 1):
            for nw, nt in forms:
                targs = f"ILb{vone}ELb{lit}ELi{nw}ELi{nt}E"
                for name in ("k_rollout_quad", "k_rollout_quad_q", "k_rollout_aerial"):
                    assert f"_Z{len(name)}{name}{targs}{tail}" in have, (name, targs)
                assert f"_Z17k_rollout_quad_tt{targs}EvjjjjiiPKfS1_N4mppi9DevParamsE" in have, targs
                for name in ("k_rollout_quad_b", "k_rollout_aerial_b"):
                    assert f"_Z{len(name)}{name}{targs}EvjjjjiiPKfS1_N4mppi9DevParamsE" in have, (name, targs)
                assert f"_Z19k_rollout_quad_tt_b{targs}EvjjjjiiPKfS1_S1_N4mppi9DevParamsE" in have, targs
