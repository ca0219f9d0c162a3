"""The C3 rollout kernels (arm, fp64 state, L = 32: k_rollout_q and k_rollout_s) hold every
kernel-argument scalar they read after the staging barrier in SGPRs from the prologue
(csrc/mppi_rollout.h rollout_body, kRoom).  Compiled here with build.py's flags for the unit to a
listing: after the first s_barrier neither kernel has a scalar load (everything else they read there is
LDS or vector memory, so any s_load would be one from the argument segment), neither uses scratch or
spills an SGPR, and both stay inside their register budgets: 102 SGPRs; 72 VGPRs for the quiet kernel
(7 waves per SIMD), 128 for the full one (4 waves).  Nothing else about the instruction stream is
asserted."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from quadrotor_manipulator_mppi_amd import build as B  # noqa: E402

UNIT = "mppi_rollout_arm_h32.hip"
# <arm, NA 7, one chunk, L 32, fp64 state, ...>: both the one-vehicle and the fleet instantiation
KERNELS = {"_Z11k_rollout_qILi1ELi7ELi1ELi32ELb1E": 72, "_Z11k_rollout_sILi1ELi7ELi1ELi32ELb1E": 128}


def _hipcc():
    try:
        return B.hipcc()
    except RuntimeError:
        return shutil.which("hipcc")


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    cc = _hipcc()
    if not cc:
        pytest.skip("hipcc not found")
    flags = dict(B.SOURCES)[UNIT]
    out = tmp_path_factory.mktemp("c3_listing") / "c3.s"
    cmd = [cc, f"--offload-arch={B.ARCH}", "-std=c++17", "-O3", "-I", os.path.join(ROOT, "include")] + flags + \
          ["--cuda-device-only", "-S", "-o", str(out), os.path.join(B.CSRC, UNIT)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out.read_text()


def _body(text, sym):
    m = re.search(rf"^{re.escape(sym)}:.*?^\.Lfunc_end\d+:", text, re.S | re.M)
    assert m, sym
    return [ln.strip() for ln in m.group(0).splitlines()]


def _meta(text, sym):
    m = re.search(rf"^\s+\.name:\s+{re.escape(sym)}\n(.*?)^\s+\.wavefront_size", text, re.S | re.M)
    assert m, sym
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", m.group(1), re.M)}


def test_c3_kernels_read_no_argument_after_the_staging_barrier(listing):
    syms = sorted(set(re.findall(r"^(_Z1[01]k_rollout_[qs]I\w+):", listing, re.M)))
    seen = {p: 0 for p in KERNELS}
    for sym in syms:
        for prefix, vgprs in KERNELS.items():
            if not sym.startswith(prefix):
                continue
            seen[prefix] += 1
            ops = [ln.split()[0] for ln in _body(listing, sym) if ln and not ln.startswith((";", "."))]
            first = ops.index("s_barrier")
            late = [op for op in ops[first:] if op.startswith(("s_load_", "s_buffer_load_"))]
            assert not late, f"{sym}: {len(late)} scalar loads after the staging barrier"
            assert any(op.startswith("s_load_") for op in ops[:first])   # (the listing was read right)
            md = _meta(listing, sym)
            assert md["private_segment_fixed_size"] == 0 and md["sgpr_spill_count"] == 0 and md["vgpr_spill_count"] == 0, (sym, md)
            assert md["sgpr_count"] <= 102 and md["vgpr_count"] <= vgprs, (sym, md)
    assert all(n == 2 for n in seen.values()), seen   # one vehicle, fleet
