"""The kernel sources' include graph (CPU only; needs hipcc, runs nothing).

* Every header under csrc/ compiles on its own for gfx950: it includes what it uses.
* The plan unit and the quadrotor rollout unit reach the rollout's helpers (noise, FK, scans, stores)
  without the rollout itself: their preprocessed text holds neither rollout_body nor a launcher.
* build.py's staleness rule sees every header on disk.
"""
import glob
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from quadrotor_manipulator_mppi_amd import build as B  # noqa: E402

HEADERS = sorted(os.path.basename(h) for h in glob.glob(os.path.join(B.CSRC, "*.h")))


def _hipcc():
    try:
        return B.hipcc()
    except RuntimeError:
        return shutil.which("hipcc")


def _device_only(*args):
    cc = _hipcc()
    if not cc:
        pytest.skip("hipcc not found")
    cmd = [cc, f"--offload-arch={B.ARCH}", "-std=c++17", "-I", os.path.join(ROOT, "include"), "--cuda-device-only"] + list(args)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_on_its_own(header):
    r = _device_only("-fsyntax-only", "-x", "hip", os.path.join(B.CSRC, header))
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("unit", ["mppi_plan.hip", "mppi_rollout_quad.hip"])
def test_unit_does_not_include_the_rollout(unit):
    r = _device_only("-E", os.path.join(B.CSRC, unit))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "quad_axis_step" in r.stdout   # (the preprocessed text was read right: both units use the step)
    for name in ("rollout_body", "launch_rollout_k"):
        assert name not in r.stdout, f"{unit} includes {name}"


def test_every_header_is_a_build_dependency():
    assert HEADERS, B.CSRC
    assert set(HEADERS) <= {os.path.basename(h) for h in B.HEADERS}
