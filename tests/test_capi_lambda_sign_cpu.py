"""The kernels' exponent scale is fp32(-1 / lambda) and the finalize's row factors rely on its sign
(csrc/mppi_finalize.hip fin_body, the bare row factors: exp(coef * (+inf - finite)) must be +0 without a select), so
configuration validation refuses a lambda whose scale is not negative in single precision: infinite,
or so large that -1 / lambda underflows to -0.  Checked through the pure layout stage, without a GPU."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_engine_layouts as R  # noqa: E402
from quadrotor_manipulator_mppi_amd.engine import make_config  # noqa: E402


@pytest.mark.parametrize("lam", [float("inf"), 1e300, 1e46])
def test_a_lambda_whose_fp32_scale_is_not_negative_is_refused(lam):
    ans = R.layout(make_config("arm", n_samples=64, n_horizon=32, lam=lam))
    assert R.refused(ans) and ans[0] == -1 and "underflows single precision" in ans[1], ans


@pytest.mark.parametrize("lam", [0.1, 1e-6, 1e30])
def test_ordinary_lambdas_pass(lam):
    assert not R.refused(R.layout(make_config("arm", n_samples=64, n_horizon=32, lam=lam)))
