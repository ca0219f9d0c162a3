"""Engines built from the layout stage compute what the engines of the one-pass mppi_create
computed: one control step per model at its smallest shape (K = 16; H = 20 drone, 32 arm, 64
whole-body and quadrotor), one engine with three vehicles and one with every cost term, against
tests/golden/engine_layout_steps.json -- recorded on an MI355X from the library as it was before
create was split (tools/record_engine_layouts.py --steps).  The kernels are unchanged and draw their
own noise from the configuration's seed, and every sum in them has a fixed order (the suite compares
engines bit for bit elsewhere: tests/test_gpu_specialized.py), so the outputs are compared exactly.

mppi_kernel_info must name the kernels that the capture diagnostics name for the layout's own
geometry (mppi_debug_layout): the layout, not a second derivation, picks the kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_engine_layouts as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return R.load_steps()


def _expected_kernels(L, cfg, w):
    """(rollout, finalize) symbols of a control call's full launches for the layout `w`."""
    full, quiet = C.create_string_buffer(192), C.create_string_buffer(192)
    for name in ("mppi_debug_rollout_kernels", "mppi_debug_finalize_kernels"):
        f = getattr(L, name)
        f.restype, f.argtypes = C.c_int32, [C.POINTER(C.c_int32), C.c_char_p, C.c_char_p, C.c_int32]
    g = (cfg.model, cfg.n_action, cfg.n_horizon, w["L"], w["nch"], w["iters"], w["threads"], cfg.n_vehicles,
         cfg.state_f64, cfg.noise_mode, cfg.store_noise, cfg.cost_terms, int(not w["sigma_diag"]), 0, w["generic"] & 4)
    assert L.mppi_debug_rollout_kernels((C.c_int32 * len(g))(*g), full, quiet, 192) == 0
    roll = full.value.decode()
    g = (cfg.n_action, cfg.n_horizon, w["fin_tsz"], cfg.savgol_window // 2, w["fin_ts"], cfg.savgol_window,
         w["nb"], 0, 0, w["generic"] & 1)
    assert L.mppi_debug_finalize_kernels((C.c_int32 * len(g))(*g), full, quiet, 192) == 0
    return roll, full.value.decode()


@pytest.mark.parametrize("name", list(R.STEP_CASES))
def test_step_equals_the_recording_and_runs_the_layouts_kernels(golden, name):
    e, got = R.run_step(name)
    for k, v in got.items():
        np.testing.assert_array_equal(v, golden[f"{name}.{k}"], err_msg=f"{name}: {k}")
    assert np.isfinite(got["out"]).all() and np.isfinite(got["u_prev"]).all()
    roll, fin = _expected_kernels(e._L, e.cfg, dict(zip(R.WORDS, R.layout(e.cfg))))
    info = e.kernel_info()
    assert info.split("; call: ")[1].split(";")[0] == f"rollout {roll}, finalize {fin}", info
    e.close()
