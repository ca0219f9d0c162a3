"""The quiet rollout (csrc/mppi_rollout.h rollout_body QUIET: k_rollout_q, k_rollout_ql;
csrc/mppi_rollout_quad.hip: k_rollout_quad_q) runs on a batch's steps before its last and writes
the block records and nothing else: no trajectory planes, no costs, no handed-over vehicle
constants.  Its records must be bit for bit those of the full kernel, and the batch's last step
must run the full kernel, so that what a batch leaves behind is its last step's.

Every case runs one engine as shipped and one created with MPPI_GENERIC_KERNELS=1 (the full
rollout and the full FINAL on every step) on the same seed through a control call, a 2-step batch,
a 5-step batch, a control call and a 1-step batch, and compares u_prev, costs, trajectory planes
and outputs bit for bit after each stage.  u_prev after a batch depends on every step's records
(the quiet kernels'); the trajectory planes and costs after it are the last step's (the full
kernel's, at the right Philox step).  mppi_kernel_info says which kernels ran, so a silent
fall-back to the full kernel fails here too."""
import numpy as np
import pytest

from noise_stream import MODEL_A, assert_stream

pytestmark = pytest.mark.gpu

HOME = [1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0]
MODEL_ID = {"drone": 0, "arm": 1, "wholebody": 2}
SIG = "EvjjjjiiiPKfPKN4mppi8JointDevENS2_9DevParamsE"


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


def _engine(monkeypatch, model, env, peer=False, **kw):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # read at mppi_create
    e = Engine(make_config(model, device=0, seed=23, **kw))
    for k in env:
        monkeypatch.delenv(k)
    if peer:   # one rank exchanging with itself
        e.peer_connect([e.peer_open()])
        for phase in (0, 1, 2):
            e.peer_probe(phase)
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


def _batch_part(info):
    return info.split("; call:")[0]


def _names_quiet(info):   # any quiet rollout symbol (k_rollout_quad itself starts with "k_rollout_q")
    return any(k in info for k in ("k_rollout_qI", "k_rollout_qlI", "k_rollout_quad_q"))


def _stages(engines, model):
    """Control call, 2-step batch, 5-step batch, control call, 1-step batch; every engine compared
    with the first after each stage.  Returns every engine's kernel_info after the 5-step batch."""
    ref = engines[0]

    def call(shift, what):
        st = _state(model, ref.V, shift=shift)
        outs = [e.step(st) for e in engines]
        for e, o in zip(engines[1:], outs[1:]):
            _same(ref, e, what, (outs[0], o))

    def batch(n):
        c0 = [e.get_step_counter() for e in engines]
        for e in engines:
            e.run_steps(n)
        for e in engines[1:]:
            _same(ref, e, f"{n}-step batch")
        assert [e.get_step_counter() for e in engines] == [c + n for c in c0]

    call(0.0, "control call")
    for e in engines:   # a control call runs no quiet kernel (nor did any batch yet)
        assert not _names_quiet(e.kernel_info()), e.kernel_info()
    batch(2)
    batch(5)
    info = [e.kernel_info() for e in engines]
    call(0.05, "call after the batches")
    batch(1)
    for e in engines:   # a one-step batch runs the full kernels only
        assert "quiet rollout none" in _batch_part(e.kernel_info()), e.kernel_info()
    return info


def _q(model, A, L, f64, vone):    # k_rollout_q: the 512-thread single-group kernel's quiet form
    return f"_Z11k_rollout_qILi{MODEL_ID[model]}ELi{A}ELi1ELi{L}ELb{f64}ELb{vone}ELb0E{SIG}"


def _ql(model, A, L, f64, vone, oneg):   # k_rollout_ql: k_rollout's (any block size, one group or a loop)
    return f"_Z12k_rollout_qlILi{MODEL_ID[model]}ELi{A}ELi1ELi{L}ELb{f64}ELb{vone}ELb0ELb{oneg}E{SIG}"


QUAD_Q = "_Z16k_rollout_quad_qILb1ELb0ELi1ELi512EEvjjjjiiPKfN4mppi9DevParamsE"

# (model, config, the quiet rollout's symbol)
CASES = [
    ("arm", dict(n_samples=64, n_horizon=32, state_f64=True), _q("arm", 7, 32, 1, 1)),
    ("arm", dict(n_samples=250, n_horizon=32, state_f64=True), _q("arm", 7, 32, 1, 1)),     # partial last block
    ("arm", dict(n_samples=4096, n_horizon=32, state_f64=True), _q("arm", 7, 32, 1, 1)),    # C3: 256 blocks
    ("arm", dict(n_samples=64, n_horizon=32, state_f64=False), _q("arm", 7, 32, 0, 1)),
    ("drone", dict(n_samples=256, n_horizon=32), _q("drone", 3, 32, 0, 1)),
    ("quadrotor", dict(n_samples=64, n_horizon=32), QUAD_Q),
    ("wholebody", dict(n_samples=128, n_horizon=64, n_vehicles=1), _q("wholebody", 10, 64, 0, 1)),
    ("wholebody", dict(n_samples=128, n_horizon=64, n_vehicles=2), _q("wholebody", 10, 64, 0, 0)),   # blockIdx.y, vc[v]
    # the looping kernel, 3 blocks x 13 groups of 2 waves (tests/test_gpu_noise_stream.py's override)
    ("wholebody", dict(n_samples=77, n_horizon=64, block_threads=128, blocks_per_vehicle=3),
     _ql("wholebody", 10, 64, 0, 1, 0)),
    # one group per wave at a block size other than 512
    ("arm", dict(n_samples=77, n_horizon=32, state_f64=True, block_threads=128), _ql("arm", 7, 32, 1, 1, 1)),
]


def _id(model, kw):
    return f"{model}-" + "-".join(f"{k}{v}" for k, v in kw.items())


@pytest.mark.parametrize("model,kw,quiet", CASES, ids=[_id(m, kw) for m, kw, _ in CASES])
def test_quiet_rollout_matches_the_full_kernel(monkeypatch, model, kw, quiet):
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    gen = _engine(monkeypatch, model, {"MPPI_GENERIC_KERNELS": "1"}, **kw)
    spec = _engine(monkeypatch, model, {}, **kw)
    engines = [gen, spec]
    hip = model == "arm" and kw["n_samples"] == 64 and kw["state_f64"]
    if hip:   # the HIP launches make the same choice (mppi_run_steps' loop)
        engines.append(_engine(monkeypatch, model, {"MPPI_DISPATCH": "hip"}, **kw))
    info = _stages(engines, model)
    assert spec.dispatch_info().startswith("aql;"), spec.dispatch_info()
    assert f"quiet rollout {quiet}" in _batch_part(info[1]), info[1]
    assert quiet not in info[1].split("; call:")[1], info[1]            # control calls: the full kernel
    assert "quiet rollout none" in _batch_part(info[0]) and not _names_quiet(info[0]), info[0]
    assert info[0].endswith("; MPPI_GENERIC_KERNELS") and "MPPI_GENERIC_KERNELS" not in info[1], info
    if hip:
        assert engines[2].dispatch_info().startswith("hip"), engines[2].dispatch_info()
        assert f"quiet rollout {quiet}" in _batch_part(info[2]), info[2]
    for e in engines:
        e.close()


def test_the_part_switch_keeps_the_full_rollout(monkeypatch):
    """MPPI_GENERIC_KERNELS=quiet_rollout switches this part alone off (A/B of the parts)."""
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    kw = dict(n_samples=64, n_horizon=32, state_f64=True)
    part = _engine(monkeypatch, "arm", {"MPPI_GENERIC_KERNELS": "quiet_rollout"}, **kw)
    spec = _engine(monkeypatch, "arm", {}, **kw)
    info = _stages([part, spec], "arm")
    assert "quiet rollout none" in _batch_part(info[0]) and "quiet finalize _Z12k_finalize_s" in info[0], info[0]
    assert info[0].endswith("; MPPI_GENERIC_KERNELS (in part)"), info[0]
    part.close()
    spec.close()


# Engines and shapes that keep the full rollout on every step: (model, config, peer exchange)
FULL_ONLY = [
    pytest.param("arm", dict(n_samples=64, n_horizon=32, state_f64=True, store_noise=True), False, id="store_noise"),
    pytest.param("wholebody", dict(n_samples=128, n_horizon=64), True, id="peer-1-rank"),
    pytest.param("arm", dict(n_samples=64, n_horizon=32, state_f64=True, cost_terms=("center",)), False,
                 id="XC-cost-term"),
    pytest.param("arm", dict(n_samples=64, n_horizon=48, state_f64=True), False, id="arm-f64-H48-not-instantiated"),
]


@pytest.mark.parametrize("model,kw,peer", FULL_ONLY)
def test_engines_that_keep_the_full_rollout(monkeypatch, model, kw, peer):
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    gen = _engine(monkeypatch, model, {"MPPI_GENERIC_KERNELS": "1"}, peer=peer, **kw)
    spec = _engine(monkeypatch, model, {}, peer=peer, **kw)
    info = _stages([gen, spec], model)
    for i in info:
        assert "quiet rollout none" in _batch_part(i) and not _names_quiet(i), i
    gen.close()
    spec.close()


def test_step_word_across_the_quiet_full_boundary(monkeypatch):
    """A batch's quiet rollouts and its full one take their Philox step from the same word
    (argument + dispatch id >> 1).  An engine as shipped and a store_noise twin (the full kernel
    on every step, noise stored) run a 3-step and a 2-step batch: both counters advance by the
    batch length, the twin's stored noise after the second batch is the stream's at step 4, and
    the warm starts agree bit for bit (every step of both drew the same noise)."""
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    kw = dict(n_samples=77, n_horizon=32, state_f64=True)
    spec = _engine(monkeypatch, "arm", {}, **kw)
    twin = _engine(monkeypatch, "arm", {}, store_noise=True, **kw)
    for n, after in ((3, 3), (2, 5)):
        for e in (spec, twin):
            e.run_steps(n)
            e.synchronize()
            assert e.get_step_counter() == after
    assert "quiet rollout _Z11k_rollout_q" in spec.kernel_info() and "quiet rollout none" in twin.kernel_info()
    sigma = (np.eye(7) * 0.1).astype(np.float32)   # the arm's default Sigma (make_config)
    eps = twin.get_noise()
    assert_stream(eps[0], 23, 4, 0, np.arange(77, dtype=np.int64), 32, MODEL_A["arm"], sigma, what="step 4")
    np.testing.assert_array_equal(spec.get_u_prev(), twin.get_u_prev())
    np.testing.assert_array_equal(spec.get_trajectory(), twin.get_trajectory())
    np.testing.assert_array_equal(spec.get_costs(), twin.get_costs())
    spec.close()
    twin.close()
