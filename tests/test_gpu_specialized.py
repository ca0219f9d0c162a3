"""The finalize's role kernels (csrc/mppi_finalize.hip: k_finalize_s, one role and one table
geometry per instantiation, and the quiet FINAL of a batch's steps before its last) and the
rollout's fixed-block single-group kernel (csrc/mppi_rollout.h: k_rollout_s) must compute exactly
what the kernels of every role and block size (k_finalize, k_rollout) compute.  Every case runs
one engine as shipped and one created with MPPI_GENERIC_KERNELS=1 (k_finalize on every step, the
rollout of every block size) on the same seed through control calls, a 5-step batch (quiet
finalizes, then the full one on the last packet), a control call and a 1-step batch, and compares
bit for bit after each stage; mppi_kernel_info says which kernels ran, so a silent fall-back to
the generic kernels fails here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOME = [1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0]
GENERIC = "_Z10k_finalizeILi"
ROLE = "_Z12k_finalize_sILi"
FINAL, QUIET = 1, 2   # mppi_finalize.hip kRoleFinal, kRoleQuiet


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


def _engine(monkeypatch, model, env, **kw):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # read at mppi_create
    e = Engine(make_config(model, device=0, seed=23, **kw))
    for k in env:
        monkeypatch.delenv(k)
    for v in range(e.V):
        if model in ("drone", "quadrotor"):
            e.set_target([1.0, 2.0, 3.4], vehicle=v)
        else:
            e.set_target([0.1029, 0.4055, 1.6498], [-0.5, -0.5, 0.5, -0.5], vehicle=v)
    e.set_state(_state(model, e.V))
    return e


def _same(a, b, what, outs=None):
    a.synchronize()
    b.synchronize()
    np.testing.assert_array_equal(a.get_u_prev(), b.get_u_prev(), err_msg=what + ": u_prev")
    np.testing.assert_array_equal(a.get_costs(), b.get_costs(), err_msg=what + ": costs")
    np.testing.assert_array_equal(a.get_trajectory(), b.get_trajectory(), err_msg=what + ": trajectory planes")
    (oa, ua, sa), (ob, ub, sb) = outs if outs else (a.read_outputs(), b.read_outputs())
    np.testing.assert_array_equal(oa, ob, err_msg=what + ": out")
    np.testing.assert_array_equal(ua, ub, err_msg=what + ": u0")
    assert [(s.rho, s.eta, s.ess, s.nonfinite) for s in sa] == [(s.rho, s.eta, s.ess, s.nonfinite) for s in sb], \
        what + ": stats"


def _stages(engines, model):
    """Three control calls, a 5-step batch, a control call, a 1-step batch; all engines compared
    with the first after each stage.  Returns every engine's kernel_info after the 5-step batch."""
    ref = engines[0]
    for i in range(3):
        st = _state(model, ref.V, shift=0.01 * i)
        outs = [e.step(st) for e in engines]
        for e, o in zip(engines[1:], outs[1:]):
            _same(ref, e, f"control call {i}", (outs[0], o))
    for e in engines:
        e.run_steps(5)
    for e in engines[1:]:
        _same(ref, e, "5-step batch")
    info = [e.kernel_info() for e in engines]
    st = _state(model, ref.V, shift=0.05)
    outs = [e.step(st) for e in engines]
    for e, o in zip(engines[1:], outs[1:]):
        _same(ref, e, "call after the batch", (outs[0], o))
    for e in engines:
        e.run_steps(1)
    for e in engines[1:]:
        _same(ref, e, "1-step batch")
    for e in engines:   # a one-step batch runs the full finalize, no quiet one
        assert "quiet finalize none" in e.kernel_info(), e.kernel_info()
    return info


# (model, config, table index of the finalize geometry (0: not in the table), finalize block size)
CASES = [
    ("arm", dict(n_samples=64, n_horizon=32, state_f64=True), 1, 128),               # 4 records
    ("arm", dict(n_samples=250, n_horizon=32, state_f64=True), 1, 128),              # partial last block
    ("arm", dict(n_samples=4096, n_horizon=32, state_f64=True), 1, 256),             # the full record chunk
    ("arm", dict(n_samples=64, n_horizon=32, state_f64=False), 1, 128),
    ("drone", dict(n_samples=128, n_horizon=20), 0, 0),                              # H = 20: not in the table
    ("drone", dict(n_samples=256, n_horizon=32), 2, 128),
    ("quadrotor", dict(n_samples=64, n_horizon=32), 3, 128),
    ("wholebody", dict(n_samples=128, n_horizon=64, n_vehicles=1), 4, 128),
    ("wholebody", dict(n_samples=128, n_horizon=64, n_vehicles=2), 4, 128),          # blockIdx.y
    ("arm", dict(n_samples=64, n_horizon=32, state_f64=True, savgol_window=5), 0, 0),   # 5 taps: not in the table
]


def _check_info(info, gid, nt, what):
    batch = info.split("; call:")[0]
    if gid:
        assert f"finalize {ROLE}{nt}ELi{FINAL}ELi{gid}E" in batch, (what, info)
        assert f"quiet finalize {ROLE}{nt}ELi{QUIET}ELi{gid}E" in batch, (what, info)
    else:   # the fall-back: the kernel of every geometry, on every step
        assert f"finalize {GENERIC}" in batch and "quiet finalize none" in batch and ROLE not in info, (what, info)


@pytest.mark.parametrize("model,kw,gid,nt", CASES,
                         ids=[f"{m}-{'-'.join(f'{k}{v}' for k, v in kw.items())}" for m, kw, _, _ in CASES])
def test_role_kernels_match_the_generic_kernel(monkeypatch, model, kw, gid, nt):
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    spec = _engine(monkeypatch, model, {}, **kw)
    gen = _engine(monkeypatch, model, {"MPPI_GENERIC_KERNELS": "1"}, **kw)
    engines = [gen, spec]
    hip = gid == 1 and kw["n_samples"] == 64 and kw["state_f64"] and "savgol_window" not in kw
    if hip:   # the HIP launches make the same choices (finalize_impl)
        engines.append(_engine(monkeypatch, model, {"MPPI_DISPATCH": "hip"}, **kw))
    info = _stages(engines, model)
    assert spec.dispatch_info().startswith("aql;"), spec.dispatch_info()
    _check_info(info[1], gid, nt, "as shipped")
    # the switched engine: no role kernel anywhere, no quiet finalize
    assert ROLE not in info[0] and f"finalize {GENERIC}" in info[0] and "quiet finalize none" in info[0], info[0]
    assert info[0].endswith("; MPPI_GENERIC_KERNELS") and "MPPI_GENERIC_KERNELS" not in info[1], info
    # the rollout: its fixed-block single-group kernel at the flagship shape, never on the switched engine
    assert "k_rollout_s" not in info[0], info[0]
    if kw["n_samples"] == 4096:
        assert info[1].count("rollout _Z11k_rollout_sILi1ELi7ELi1ELi32ELb1ELb1ELb0E") == 2, info[1]
    if gid:   # control calls always run the full FINAL
        assert f"finalize {ROLE}{nt}ELi{FINAL}ELi{gid}E" in spec.kernel_info().split("; call:")[1], spec.kernel_info()
    if hip:
        assert engines[2].dispatch_info().startswith("hip"), engines[2].dispatch_info()
        _check_info(info[2], gid, nt, "HIP launches")
    for e in engines:
        e.close()
