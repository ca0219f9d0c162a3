"""The role finalize's lane map (csrc/mppi_finalize.hip fin_body, CPL > 1: several window columns per
lane, one body load for them, a block of NT / CPL threads) must compute bit for bit what k_finalize
computes with one column per lane.  Every case creates an engine as shipped and one with
MPPI_GENERIC_KERNELS=1 on the same seed, runs a 6-step batch (five quiet finalizes, then the full
one) and a control call on each and compares u_prev, out, u0 and the stats after both.  The shapes
are the record counts at which the map changes: one record, fewer records than sequences (3, 6), two
full rows per sequence of the 32-thread block (16), one record more (17), the full chunk of the
one-wave block (256), two waves with 512 records, the window starts
that are no multiple of four columns (drone, quadrotor), blockIdx.y (a fleet), the peer exchange's
FINAL, and a record without a finite cost (nan flag, f = 0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOME = [1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0]
GENERIC = "_Z10k_finalizeILi"
ROLE = "_Z12k_finalize_sILi"
GID = {"arm": 1, "drone": 2, "quadrotor": 3, "wholebody": 4}   # mppi_finalize.hip FinGeo


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
    e = Engine(make_config(model, device=0, seed=31, **kw))
    for k in env:
        monkeypatch.delenv(k)
    for v in range(e.V):
        if model in ("drone", "quadrotor"):
            e.set_target([1.0, 2.0, 3.4], vehicle=v)
        else:
            e.set_target([0.1029, 0.4055, 1.6498], [-0.5, -0.5, 0.5, -0.5], vehicle=v)
    e.set_state(_state(model, e.V))
    return e


def _stats(st):
    return [(s.rho, s.eta, s.ess, s.nonfinite) for s in st]


def _same(a, b, what, outs=None):
    a.synchronize()
    b.synchronize()
    np.testing.assert_array_equal(a.get_u_prev(), b.get_u_prev(), err_msg=what + ": u_prev")
    (oa, ua, sa), (ob, ub, sb) = outs if outs else (a.read_outputs(), b.read_outputs())
    np.testing.assert_array_equal(oa, ob, err_msg=what + ": out")
    np.testing.assert_array_equal(ua, ub, err_msg=what + ": u0")
    assert np.array_equal(np.array(_stats(sa), np.float64), np.array(_stats(sb), np.float64), equal_nan=True), \
        (what + ": stats", _stats(sa), _stats(sb))


def _batch_then_call(ref, e, model):
    for x in (ref, e):
        x.run_steps(6)
    _same(ref, e, "6-step batch")
    st = _state(model, ref.V, shift=0.02)
    _same(ref, e, "control call", (ref.step(st), e.step(st)))


def _nt(nrec):
    return 128 if nrec <= 128 else 256 if nrec <= 256 else 512


# (model, config, records per vehicle)
CASES = [("arm", dict(n_samples=K, n_horizon=32, state_f64=True), K // 16) for K in (16, 48, 256, 272, 4096)] + \
        [(m, dict(n_samples=K, n_horizon=32), K // 16) for m in ("drone", "quadrotor") for K in (48, 4096)] + \
        [("wholebody", dict(n_samples=K, n_horizon=64), n) for K, n in ((48, 6), (8192, 512))] + \
        [("drone", dict(n_samples=1024, n_horizon=32, n_vehicles=3), 64)]


@pytest.mark.parametrize("model,kw,nrec", CASES,
                         ids=[f"{m}-K{kw['n_samples']}-V{kw.get('n_vehicles', 1)}" for m, kw, _ in CASES])
def test_lane_map_matches_the_generic_kernel(monkeypatch, model, kw, nrec):
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    gen = _engine(monkeypatch, model, {"MPPI_GENERIC_KERNELS": "1"}, **kw)
    spec = _engine(monkeypatch, model, {}, **kw)
    _batch_then_call(gen, spec, model)
    info, ginfo = spec.kernel_info(), gen.kernel_info()
    # the record count is what this case is about: the role kernel of its capacity class ran, the
    # switched engine ran none
    assert f"finalize {ROLE}{_nt(nrec)}ELi1ELi{GID[model]}E" in info, info
    assert f"quiet finalize {ROLE}{_nt(nrec)}ELi2ELi{GID[model]}E" in info, info
    assert ROLE not in ginfo and f"finalize {GENERIC}" in ginfo, ginfo
    gen.close()
    spec.close()


def test_peer_final_matches_the_plain_engine(monkeypatch):
    """One rank exchanging with itself (f = exp(0) = 1: the unsharded step exactly), arm, 17 records."""
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    kw = dict(n_samples=272, n_horizon=32, state_f64=True)
    gen = _engine(monkeypatch, "arm", {"MPPI_GENERIC_KERNELS": "1"}, **kw)
    plain = _engine(monkeypatch, "arm", {}, **kw)
    peer = _engine(monkeypatch, "arm", {}, **kw)
    peer.peer_connect([peer.peer_open()])
    for ph in (0, 1, 2):
        peer.peer_probe(ph)
    for x in (gen, plain, peer):
        x.run_steps(6)
    _same(gen, plain, "6-step batch, plain")
    _same(gen, peer, "6-step batch, peer")
    st = _state("arm", shift=0.02)
    og, op, ox = gen.step(st), plain.step(st), peer.step(st)
    _same(gen, plain, "control call, plain", (og, op))
    _same(gen, peer, "control call, peer", (og, ox))
    assert f"finalize {ROLE}128ELi4ELi1E" in peer.kernel_info(), peer.kernel_info()   # kRolePeer, 17 records
    for x in (gen, plain, peer):
        x.close()


@pytest.mark.parametrize("model,K,H", [("drone", 64, 32), ("arm", 272, 32)])
def test_record_without_a_finite_cost(monkeypatch, model, K, H):
    """A NaN in one sample's noise: its rollout block's record carries rho = inf and the nan flag, so the
    fold takes it with f = 0 and the step's update is NaN -- the same bits in both kernels.  A clean
    call first, so the running sums are rescaled past the masked record as well."""
    monkeypatch.delenv("MPPI_DISPATCH", raising=False)
    kw = dict(n_samples=K, n_horizon=H, noise="injected")
    if model == "arm":
        kw["state_f64"] = True
    A = 3 if model == "drone" else 7
    gen = _engine(monkeypatch, model, {"MPPI_GENERIC_KERNELS": "1"}, **kw)
    spec = _engine(monkeypatch, model, {}, **kw)
    noise = np.random.default_rng(7).normal(0.0, 0.3, (1, K, H, A)).astype(np.float32)
    st = _state(model)
    _same(gen, spec, "clean call", (gen.step(st, noise), spec.step(st, noise)))
    noise[0, K - 11, 3, 1] = np.nan   # a sample of the last record
    og, os_ = gen.step(st, noise), spec.step(st, noise)
    _same(gen, spec, "call with a NaN sample", (og, os_))
    assert og[2][0].nonfinite and os_[2][0].nonfinite
    assert np.isnan(spec.get_u_prev()).all()
    assert f"finalize {ROLE}" in spec.kernel_info() and ROLE not in gen.kernel_info()
    gen.close()
    spec.close()
