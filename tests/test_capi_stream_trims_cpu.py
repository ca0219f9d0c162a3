"""Shortening the quiet step's instruction streams changed no launch: for the shapes
tests/test_gpu_stream_trims.py runs, the launches of a three-step native batch and of a control
call -- kernel symbol, grid, block, dynamic LDS, argument size and the digest of the argument bytes,
as mppi_debug_step_launches describes them -- equal tests/golden/stream_trims_launches.json, recorded
from the library as it was before the streams were touched; the symbols mppi_debug_rollout_kernels and
mppi_debug_finalize_kernels name are the ones they named then; and every kernel a launch names is
found in exactly one unit's code object.

    python tests/test_capi_stream_trims_cpu.py --record     (MPPI_HIP_LIB: the library to record from)
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import record_step_launches as R  # noqa: E402
from quadrotor_manipulator_mppi_amd import _capi as capi  # noqa: E402
from quadrotor_manipulator_mppi_amd import build as B  # noqa: E402
from quadrotor_manipulator_mppi_amd.engine import make_config  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "stream_trims_launches.json")
ARM64 = dict(model="arm", n_horizon=32, state_f64=True)
# the shapes of tests/test_gpu_stream_trims.py
SHAPES = [dict(ARM64, n_samples=K) for K in (16, 48, 272, 4096)] + [
    dict(model="arm", n_samples=48, n_horizon=32, state_f64=False),
    dict(model="drone", n_samples=48, n_horizon=32),
    dict(model="quadrotor", n_samples=64, n_horizon=32),
    dict(model="wholebody", n_samples=64, n_horizon=64),
    dict(model="wholebody", n_samples=1056, n_horizon=64, blocks_per_vehicle=33),
    dict(model="wholebody", n_samples=64, n_horizon=64, n_vehicles=3),
]
# (a fleet has no native control call: its call is described through HIP)
PATHS = ((R.NATIVE_BATCH, 3), (R.HIP_BATCH, 3), (R.HIP_CALL, 1))


def _name(kw):
    return " ".join(f"{k}={v}" for k, v in kw.items())


def described():
    """{shape and path: its launches, each a list} over SHAPES x PATHS."""
    out = {}
    for kw in SHAPES:
        for path, n in PATHS:
            a = R.launches(make_config(**kw), dict(path=path, n=n))
            out[f"{_name(kw)} path {path} n={n}"] = a if a == R.REFUSED else [list(lch) for lch in a]
    return out


def test_launches_equal_the_recording():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = described()
    assert sorted(got) == sorted(want)
    for what in want:
        assert got[what] == want[what], what
    # not vacuous: every batch's early steps run a quiet rollout and a quiet FINAL, its last step neither
    for what, a in got.items():
        assert a != R.REFUSED, what
        if what.endswith("n=3"):
            early = {lch[1]: lch[2] for lch in a if lch[0] == "early"}
            last = {lch[1]: lch[2] for lch in a if lch[0] == "last"}
            assert any(q in early["rollout"] for q in ("k_rollout_qI", "k_rollout_qlI", "k_rollout_quad_qI")), what
            assert not any(q in last["rollout"] for q in ("k_rollout_qI", "k_rollout_qlI", "k_rollout_quad_qI")), what
            assert early["finalize"].startswith("_Z12k_finalize_sILi") and "ELi2ELi" in early["finalize"], what
            assert last["finalize"].startswith("_Z12k_finalize_sILi") and "ELi1ELi" in last["finalize"], what


def _kernel_pair(fn, words):
    f = getattr(capi.lib(), fn)
    f.restype = C.c_int32
    f.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_char_p, C.c_int32]
    full, quiet = C.create_string_buffer(192), C.create_string_buffer(192)
    assert f((C.c_int32 * len(words))(*words), full, quiet, 192) == 0
    return full.value.decode(), quiet.value.decode()


RSIG = "EEvjjjjiiiPKfPKN4mppi8JointDevENS2_9DevParamsE"
FSIG = "EEvPKfS1_PKN4mppi7FinTailEjjiiiiijNS2_9FinParamsE"


def test_the_launchers_name_the_kernels_they_named():
    """(model, A, H, L, nch, iters, threads, V, f64, noise, store_noise, cost_terms, full Sigma, peer,
    generic) -> (full, quiet) and (A, H, tsz, half, ts, window, records, mode, peer, generic) -> (full,
    quiet), at the default shapes: C3, drone C2, quadrotor, the whole-body shard and its looping form."""
    ph = capi.NOISE_PHILOX
    roll = lambda *w: _kernel_pair("mppi_debug_rollout_kernels", w)   # noqa: E731
    fin = lambda *w: _kernel_pair("mppi_debug_finalize_kernels", w)   # noqa: E731
    assert roll(capi.MODEL_ARM, 7, 32, 32, 1, 1, 512, 1, 1, ph, 0, 0, 0, 0, 0) == \
        ("_Z11k_rollout_sILi1ELi7ELi1ELi32ELb1ELb1ELb0" + RSIG, "_Z11k_rollout_qILi1ELi7ELi1ELi32ELb1ELb1ELb0" + RSIG)
    assert roll(capi.MODEL_DRONE, 3, 32, 32, 1, 1, 512, 1, 0, ph, 0, 0, 0, 0, 0) == \
        ("_Z11k_rollout_sILi0ELi3ELi1ELi32ELb0ELb1ELb0" + RSIG, "_Z11k_rollout_qILi0ELi3ELi1ELi32ELb0ELb1ELb0" + RSIG)
    assert roll(capi.MODEL_WHOLEBODY, 10, 64, 64, 1, 1, 512, 1, 0, ph, 0, 0, 0, 0, 0) == \
        ("_Z11k_rollout_sILi2ELi10ELi1ELi64ELb0ELb1ELb0" + RSIG, "_Z11k_rollout_qILi2ELi10ELi1ELi64ELb0ELb1ELb0" + RSIG)
    assert roll(capi.MODEL_WHOLEBODY, 10, 64, 64, 1, 4, 512, 1, 0, ph, 0, 0, 0, 0, 0) == \
        ("_Z9k_rolloutILi2ELi10ELi1ELi64ELb0ELb1ELb0ELb0" + RSIG, "_Z12k_rollout_qlILi2ELi10ELi1ELi64ELb0ELb1ELb0ELb0" + RSIG)
    assert roll(capi.MODEL_QUADROTOR, 4, 32, 32, 1, 1, 512, 1, 0, ph, 0, 0, 0, 0, 0) == \
        ("_Z14k_rollout_quadILb1ELb0ELi1ELi512EEvjjjjiiPKfN4mppi9DevParamsE",
         "_Z16k_rollout_quad_qILb1ELb0ELi1ELi512EEvjjjjiiPKfN4mppi9DevParamsE")
    for gid, (A, H, win, nrec, nt) in {1: (7, 32, 9, 256, 256), 2: (3, 32, 5, 256, 256), 3: (4, 32, 5, 256, 256),
                                       4: (10, 64, 9, 512, 512)}.items():
        assert fin(A, H, 8, win // 2, H // 8, win, nrec, 0, 0, 0) == \
            (f"_Z12k_finalize_sILi{nt}ELi1ELi{gid}" + FSIG, f"_Z12k_finalize_sILi{nt}ELi2ELi{gid}" + FSIG)


def test_every_launched_kernel_is_in_exactly_one_code_object():
    blobs = {}
    for unit in B.KERNEL_UNITS:
        with open(B.code_object_path(B.LIB, unit), "rb") as f:
            blobs[unit] = f.read()
    syms = {lch[2] for a in described().values() for lch in a}
    assert len(syms) >= 20
    for sym in sorted(syms):
        units = [u for u, blob in blobs.items() if (sym + ".kd").encode() in blob]
        assert len(units) == 1, (sym, units)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    with open(FIXTURE, "w") as f:
        json.dump(described(), f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(FIXTURE, len(described()), "rows")
