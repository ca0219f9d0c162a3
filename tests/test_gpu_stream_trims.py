"""The trimmed instruction streams of a quiet step (csrc/mppi_rollout.h: the quiet body forms no
eta^2, the C3 chain takes its sin / cos ahead of the joints; csrc/mppi_rollout_quad.hip;
csrc/mppi_finalize.hip: the quiet role folds no eta^2) must leave every result as it was.

Every case creates an engine as shipped and one with MPPI_GENERIC_KERNELS=1 (the full rollout and
the kernel of every role on every step) on the same seed and runs batches of 1, 2 and 5 steps, each
followed by one control call.  After each batch u_prev, out, u0, the stats, the costs and
trajectory planes of the batch's last step and get_weighted_noise (READBACK of the last step's
full records) are compared bit for bit, after each call all but the last.  u_prev after a batch
depends on every quiet step's records: rho, eta, the nan flag and the bodies, not eta^2."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOME = [1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0]


def _state(model, V=1, shift=0.0):
    if model == "arm":
        s = [0, 0, 1, 0, 0, 0, 1] + HOME + [0.0] * 7
    elif model == "drone":
        s = [0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    elif model == "quadrotor":
        s = [0.0, 0.0, 1.0, 0.0, 0.0, 0.0] + [0.0] * 6
    else:
        s = [0, 0, 1, 0, 0, 0, 1] + HOME + [0.0] * 10
    s = np.tile(np.array(s, np.float64), (V, 1))
    s[:, 0] += shift
    return s


def _engine(monkeypatch, model, env, tpos=None, **kw):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # read at mppi_create
    e = Engine(make_config(model, device=0, seed=47, **kw))
    for k in env:
        monkeypatch.delenv(k)
    for v in range(e.V):
        if model in ("drone", "quadrotor"):
            e.set_target(tpos or [1.0, 2.0, 3.4], vehicle=v)
        else:
            e.set_target(tpos or [0.1029, 0.4055, 1.6498], [-0.5, -0.5, 0.5, -0.5], vehicle=v)
    e.set_state(_state(model, e.V))
    return e


def _stats(st):
    return np.array([(s.rho, s.eta, s.ess, s.nonfinite) for s in st], np.float64)


def _same(a, b, what, outs=None, readback=False):
    a.synchronize()
    b.synchronize()
    np.testing.assert_array_equal(a.get_u_prev(), b.get_u_prev(), err_msg=what + ": u_prev")
    (oa, ua, sa), (ob, ub, sb) = outs if outs else (a.read_outputs(), b.read_outputs())
    np.testing.assert_array_equal(oa, ob, err_msg=what + ": out")
    np.testing.assert_array_equal(ua, ub, err_msg=what + ": u0")
    np.testing.assert_array_equal(_stats(sa), _stats(sb), err_msg=what + ": stats")
    np.testing.assert_array_equal(a.get_costs(), b.get_costs(), err_msg=what + ": costs")
    np.testing.assert_array_equal(a.get_trajectory(), b.get_trajectory(), err_msg=what + ": trajectory planes")
    if readback:
        (ra, sma), (rb, smb) = a.get_weighted_noise(), b.get_weighted_noise()
        np.testing.assert_array_equal(ra, rb, err_msg=what + ": weighted noise")
        np.testing.assert_array_equal(sma, smb, err_msg=what + ": smoothed weighted noise")


def _batches_and_calls(gen, spec, model):
    """Batches of 1, 2 and 5 steps, a control call after each.  Returns the shipped engine's
    kernel_info after the 5-step batch."""
    info = None
    for i, n in enumerate((1, 2, 5)):
        for e in (gen, spec):
            e.run_steps(n)
        _same(gen, spec, f"{n}-step batch", readback=True)
        info = spec.kernel_info()
        st = _state(model, gen.V, shift=0.01 * (i + 1))
        _same(gen, spec, f"call after the {n}-step batch", (gen.step(st), spec.step(st)))
    return info


def _batch_part(info):
    return info.split("; call:")[0]


ARM64 = dict(n_horizon=32, state_f64=True)
# (model, config, what the quiet rollout's and the quiet finalize's symbols start with)
CASES = [
    ("arm", dict(n_samples=16, **ARM64), "_Z11k_rollout_qILi1ELi7ELi1ELi32ELb1E", 128),      # one record
    ("arm", dict(n_samples=48, **ARM64), "_Z11k_rollout_qILi1ELi7ELi1ELi32ELb1E", 128),      # 3 records
    ("arm", dict(n_samples=272, **ARM64), "_Z11k_rollout_qILi1ELi7ELi1ELi32ELb1E", 128),     # 17: a second row-group round
    ("arm", dict(n_samples=4096, **ARM64), "_Z11k_rollout_qILi1ELi7ELi1ELi32ELb1E", 256),    # C3
    ("arm", dict(n_samples=48, n_horizon=32, state_f64=False), "_Z11k_rollout_qILi1ELi7ELi1ELi32ELb0E", 128),
    ("drone", dict(n_samples=48, n_horizon=32), "_Z11k_rollout_qILi0ELi3ELi1ELi32ELb0E", 128),
    ("quadrotor", dict(n_samples=64, n_horizon=32), "_Z16k_rollout_quad_qI", 128),
    ("wholebody", dict(n_samples=64, n_horizon=64), "_Z11k_rollout_qILi2ELi10ELi1ELi64ELb0ELb1E", 128),
    # the looping quiet kernel: 132 groups on 33 blocks (the automatic layout would give each its own block)
    ("wholebody", dict(n_samples=1056, n_horizon=64, blocks_per_vehicle=33),
     "_Z12k_rollout_qlILi2ELi10ELi1ELi64ELb0ELb1ELb0ELb0E", 128),
    ("wholebody", dict(n_samples=64, n_horizon=64, n_vehicles=3), "_Z11k_rollout_qILi2ELi10ELi1ELi64ELb0ELb0E", 128),
]


@pytest.mark.parametrize("model,kw,quiet,nt", CASES,
                         ids=[f"{m}-K{kw['n_samples']}-V{kw.get('n_vehicles', 1)}-f64{int(kw.get('state_f64', 0))}"
                              for m, kw, _, _ in CASES])
def test_trimmed_streams_match_the_generic_kernels(monkeypatch, model, kw, quiet, nt):
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    gen = _engine(monkeypatch, model, {"MPPI_GENERIC_KERNELS": "1"}, **kw)
    spec = _engine(monkeypatch, model, {}, **kw)
    info = _batches_and_calls(gen, spec, model)
    # the trimmed kernels ran (a silent fall-back to the full ones would compare equal too)
    assert f"quiet rollout {quiet}" in _batch_part(info), info
    assert f"quiet finalize _Z12k_finalize_sILi{nt}ELi2E" in _batch_part(info), info
    assert "k_finalize_s" not in gen.kernel_info() and "quiet rollout none" in _batch_part(gen.kernel_info())
    gen.close()
    spec.close()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_blocks_without_a_finite_cost(monkeypatch, bad):
    """A target position that is NaN (every cost NaN: the records carry the nan flag and rho = inf)
    or infinite (every cost +inf: rho = inf, eta = 0, no flag): no sample of any block has a finite
    cost.  The quiet steps' records must carry the flag and rho through to u_prev as the full ones do."""
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    kw = dict(n_samples=48, **ARM64)
    tpos = [0.1029, bad, 1.6498]
    gen = _engine(monkeypatch, "arm", {"MPPI_GENERIC_KERNELS": "1"}, tpos=tpos, **kw)
    spec = _engine(monkeypatch, "arm", {}, tpos=tpos, **kw)
    info = _batches_and_calls(gen, spec, "arm")
    assert "quiet rollout _Z11k_rollout_qI" in _batch_part(info), info
    assert np.isnan(spec.get_u_prev()).all()
    assert spec.read_outputs()[2][0].nonfinite
    gen.close()
    spec.close()
