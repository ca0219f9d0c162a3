"""The aerial manipulator model on the GPU against tests/aerial_oracle.py: k_rollout_aerial, the finalize on
11 dims, the host-formed outputs, k_plan_aerial, the elite readback and the batch paths.  Every bound is that
file's (derived there; nothing here is tuned to what the kernels give); tests/test_aerial_oracle_cpu.py holds
the same inputs to the caps and shows that each planted mistake would fail them.

Each comparison prints its worst err / bound as a JSON row (side = "gpu"): the tolerances' measured slack
(profiles/aerial/gpu_tests.log)."""
import json

import numpy as np
import pytest

import aerial_oracle as A
import noise_stream as NS
import quad_oracle as Q
import softmin_oracle as SO

pytestmark = pytest.mark.gpu


def _log(**row):
    print(json.dumps(dict(side="gpu", **row)))


def _config(case, d, **extra):
    kw = dict(model="aerial", n_samples=case.K, n_horizon=case.H, n_vehicles=case.V, noise="injected", dt=d.cfg.dt,
              quad=d.cfg.quad(case.literal))
    kw.update(extra)
    return kw


def _split(traj):
    """(base (…, 6), q (…, 7), ee (…, 4, 4)) of get_trajectory rows: xyz, rpy, q, EE 4x4."""
    return traj[..., :6], traj[..., 6:13], traj[..., 13:].reshape(*traj.shape[:-1], 4, 4)


def _check_rows(tag, v, ao, traj, S, samples=None):
    base, q, ee = _split(traj)
    r = A.compare(ao, base, q, ee, S, samples)
    _log(case=tag, vehicle=v, pos=round(r.pos, 4), ang=round(r.ang, 4), q=round(r.q, 4), ee=round(r.ee, 4), rot=round(r.rot, 4), S=round(r.S, 4),
         excluded=r.excluded, circular=r.circular)
    assert r.excluded <= A.EXCLUDED_CAP and r.circular <= A.CIRCULAR_CAP, (tag, v, r)
    assert np.isfinite(traj).all() and np.isfinite(S).all(), (tag, v)
    # the channel order: the EE's last row, and its position within the arm's reach of the base's
    assert np.array_equal(ee[..., 3, :], np.broadcast_to(np.float32([0, 0, 0, 1]), ee[..., 3, :].shape)), (tag, v)
    assert r.worst() <= 1.0, (tag, v, r)
    return r


def _fly(case, chain, **extra):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    veh = case.vehicles()
    e = Engine(make_config(**_config(case, veh[0][0], **extra)))
    for v, (d, u, eps) in enumerate(veh):
        e.set_target(np.float32(d.tpos), np.float32(d.tquat), vehicle=v)
    e.set_u_prev(np.stack([u for _, u, _ in veh]))
    out, u0, st = e.step(np.stack([d.state for d, _, _ in veh]), np.stack([eps for _, _, eps in veh]))
    return e, veh, out, u0, st


# ------------------------------------------------------------------------------------- the rollout, by shape
@pytest.mark.parametrize("case", A.CASES, ids=[c.tag for c in A.CASES])
def test_rollout_inside_the_bounds(case, kinova_chain):
    e, veh, out, u0, st = _fly(case, kinova_chain)
    sym = f"k_rollout_aerialILb{int(case.V == 1)}ELb{int(case.literal)}ELi1ELi512E"
    assert sym in e.kernel_info().split("call:")[-1], e.kernel_info()
    traj, S = e.get_trajectory(), e.get_costs()
    assert traj.shape == (case.V, case.K, case.H, 29) and e.traj_channels == 29
    for v, (d, u, eps) in enumerate(veh):
        assert not st[v].nonfinite, (case.tag, v)
        ao = A.rollout(kinova_chain, u, eps, d.state, d.tpos, d.tquat, d.cfg, case.literal)
        _check_rows(case.tag, v, ao, traj[v], S[v])
        if v == 0:   # the case can fail: the WHOLEBODY composition is far outside the bounds on these inputs
            bad = A.emulate(kinova_chain, u, eps, d.state, d.tpos, d.tquat, d.cfg, case.literal, variant="fixed_attitude")
            assert A.compare(ao, bad["base"], bad["q"], bad["ee"], bad["S"]).ee > 1.0
        # the finalize, given the GPU's own costs: S's tolerance does not leak into this check
        lam = float(e.cfg.lambda_)
        red = SO.reduce(S[v], eps, lam, 9, 2, u)
        lay = SO.Layout(R=16, nw=1, iters=1, nb=(case.K + 15) // 16, quad=True)
        bnd = SO.bounds(red, eps, lay)
        raw, sm = e.get_weighted_noise()
        got = dict(w=e.get_weights()[v], w_eps_raw=raw[v], w_eps=sm[v], u_prev=e.get_u_prev()[v], eta=st[v].eta, ess=st[v].ess)
        assert np.float32(st[v].rho) == np.float32(red.rho), (case.tag, v, st[v].rho, red.rho)
        r = SO.ratios(got, red, bnd)
        _log(case=case.tag, vehicle=v, **{"softmin_" + k: round(x, 4) for k, x in r.items()})
        assert max(r.values()) <= 1.0, (case.tag, v, r)
        assert np.array_equal(u0[v], got["u_prev"][0]), (case.tag, v)
        # the outputs: the base's first step under u0 (host-formed) and the joints' qdes, vdes (mppi.py:157-158)
        want, b = Q.first_step_outputs(d.x, d.v, u0[v, :4], d.cfg)
        err = np.abs(out[v, :12] - want)
        _log(case=case.tag, vehicle=v, outputs=round(float(np.max(err / b)), 4))
        assert (err <= b).all(), (case.tag, v, err / b)
        dt = float(np.float32(d.cfg.dt))
        q0, qd0 = np.float32(d.q).astype(np.float64), np.float32(d.qd).astype(np.float64)
        qdes = q0 + u[0, 4:].astype(np.float64) * dt + 0.5 * u0[v, 4:].astype(np.float64) * dt * dt
        vdes = qd0 + u0[v, 4:].astype(np.float64) * dt
        assert np.allclose(out[v, 12:19], qdes, rtol=1e-6, atol=1e-6), (case.tag, v, out[v, 12:19] - qdes)
        assert np.allclose(out[v, 19:26], vdes, rtol=1e-5, atol=1e-6), (case.tag, v, out[v, 19:26] - vdes)
    e.close()


# ------------------------------------------------------------------------------------------- device noise
def test_large_k_philox_four_wave_form(kinova_chain):
    """K = 16400, H = 20: more than 1024 blocks, so 64 rollouts per block on four dynamics waves.  The stored noise
    is the Philox stream of 11 dims, and the first and last 32 samples are the oracle's on that noise."""
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config, philox_normals
    K, H, seed = 16400, 20, 0xA3F1
    d = A.DESIGNS[0]
    case = A.Case("K16400-H20", K, H)
    e = Engine(make_config(**_config(case, d, noise="philox", store_noise=True, seed=seed)))
    u, _ = d.inputs(1, H)
    e.set_target(np.float32(d.tpos), np.float32(d.tquat))
    e.set_u_prev(u[None])
    step = e.get_step_counter()
    out, u0, st = e.step(d.state)
    assert "k_rollout_aerialILb1ELb0ELi4ELi256E" in e.kernel_info().split("call:")[-1], e.kernel_info()
    assert not st[0].nonfinite
    eps = e.get_noise()[0]
    sel = np.r_[0:64, 8160:8224, K - 64:K]
    NS.assert_stream(eps[sel], seed, step, 0, sel, H, 11, np.float32(A.SIGMA), what="aerial stored noise")
    for k0 in (0, K - 64):   # bit for bit what the library's own draw of 11 dims gives (one Philox4x32 + one Philox2x32 call)
        _, z = philox_normals(seed, step, 0, k0, 64, H, 11)
        assert np.array_equal(eps[k0:k0 + 64], z * np.float32(A.SIGMA)), k0
    traj, S = e.get_trajectory()[0], e.get_costs()[0]
    idx = np.r_[0:32, K - 32:K]
    ao = A.rollout(kinova_chain, u, eps[idx], d.state, d.tpos, d.tquat, d.cfg)
    _check_rows(case.tag, 0, ao, traj[idx], S[idx])
    assert np.isfinite(S).all()
    e.close()


def test_block_forms_agree_bit_for_bit():
    """V = 3 runs K = 4096, H = 32 in 256-thread blocks (768 blocks), V = 1 in 512-thread blocks: vehicle 0 draws the same
    noise in both (the stream is keyed by the vehicle), and its costs agree bit for bit."""
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    d = A.DESIGNS[0]
    u, _ = d.inputs(1, 32)
    S = {}
    for V, nt in ((1, 512), (3, 256)):
        e = Engine(make_config(model="aerial", n_samples=4096, n_horizon=32, n_vehicles=V, seed=91, store_trajectory=False))
        for v in range(V):
            e.set_target(np.float32(d.tpos), np.float32(d.tquat), vehicle=v)
        e.set_u_prev(np.broadcast_to(u, (V, 32, 11)).copy())
        e.step(np.broadcast_to(d.state, (V, 26)).copy())
        assert f"k_rollout_aerialILb{int(V == 1)}ELb0ELi1ELi{nt}E" in e.kernel_info().split("call:")[-1], e.kernel_info()
        S[V] = e.get_costs()[0]
        e.close()
    assert np.isfinite(S[1]).all() and np.ptp(S[1]) > 0
    assert np.array_equal(S[1], S[3])


# ----------------------------------------------------------------------------------------------- batching
def test_native_batch_equals_hip_steps(monkeypatch):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    d = A.DESIGNS[1]
    u, _ = d.inputs(1, 32)

    def make(mode):
        if mode:
            monkeypatch.setenv("MPPI_DISPATCH", mode)
        else:
            monkeypatch.delenv("MPPI_DISPATCH", raising=False)
        e = Engine(make_config(model="aerial", n_samples=256, n_horizon=32, seed=17))
        e.set_target(np.float32(d.tpos), np.float32(d.tquat))
        e.set_u_prev(u[None])
        e.set_state(d.state)
        return e

    a = make(None)
    a.run_steps(3)
    a.synchronize()
    assert a.dispatch_info().startswith("aql;"), a.dispatch_info()
    info = a.kernel_info()
    assert "k_rollout_aerial" in info.split(";")[0] and "quiet rollout none" in info, info
    ua = a.get_u_prev()
    h = make("hip")
    for _ in range(3):
        h.step(d.state)
    assert h.dispatch_info().endswith("calls: hip"), h.dispatch_info()
    uh = h.get_u_prev()
    assert np.isfinite(ua).all() and not np.array_equal(ua[0], u)
    assert np.array_equal(ua, uh)
    a.close()
    h.close()


def test_split_phases_and_kernel_timing():
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    d = A.DESIGNS[0]
    u, _ = d.inputs(1, 32)
    e = Engine(make_config(model="aerial", n_samples=256, n_horizon=32, seed=17))
    e.set_target(np.float32(d.tpos), np.float32(d.tquat))
    e.set_u_prev(u[None])
    e.set_state(d.state)
    e.rollout()
    e.finalize()
    out, u0, st = e.read_outputs()
    assert np.isfinite(out).all() and not st[0].nonfinite
    before = e.get_u_prev()
    r, f = e.kernel_timing(5)
    assert 0 < r < 1e4 and 0 < f < 1e4
    assert np.array_equal(e.get_u_prev(), before)
    e.close()


# --------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("name,H,literal", [("tilt_a", 20, False), ("tilt_b", 64, True), ("tilt_b", 33, False)])
def test_plan_against_the_zero_noise_rollout(kinova_chain, name, H, literal):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    d = A.BY_NAME[name]
    u, _ = d.inputs(1, H)
    e = Engine(make_config(model="aerial", n_samples=64, n_horizon=H, dt=d.cfg.dt, quad=d.cfg.quad(literal)))
    e.set_target(np.float32(d.tpos), np.float32(d.tquat))
    e.set_u_prev(u[None])
    e.set_state(d.state)
    p = e.get_plan().vehicle(0)
    ao = A.rollout(kinova_chain, u, np.zeros((1, H, 11), np.float32), d.state, d.tpos, d.tquat, d.cfg, literal)
    assert ao.valid.all()
    assert p.traj.shape == (H, 29)
    _check_rows(f"plan-{name}-H{H}", 0, ao, p.traj[None], np.float32([p.S]))
    perr = np.abs(p.pos_err - ao.pos_err[0])
    ct = np.abs(p.cost_t - ao.cost_t[0]) / ao.b_cost_t[0]
    _log(case=f"plan-{name}-H{H}", pos_err=round(float(perr.max() / A.TOL_PERR_WB), 4), cost_t=round(float(ct.max()), 4))
    assert perr.max() <= A.TOL_PERR_WB and ct.max() <= 1.0
    assert np.allclose(p.ee_path, ao.ee[0, :, :3, 3], rtol=0, atol=float(ao.b_ee.max()))
    e.close()


def test_plan_after_a_step_is_the_plan_of_the_committed_warm_start(kinova_chain):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    case = A.CASES[0]
    e, veh, out, u0, st = _fly(case, kinova_chain)
    d = veh[0][0]
    p1 = e.get_plan().vehicle(0)
    un = e.get_u_prev()
    assert not np.array_equal(un[0], veh[0][1])
    f = Engine(make_config(**_config(case, d)))
    f.set_target(np.float32(d.tpos), np.float32(d.tquat))
    f.set_u_prev(un)
    f.set_state(d.state)
    p2 = f.get_plan().vehicle(0)
    for a, b in ((p1.traj, p2.traj), (p1.cost_t, p2.cost_t), (p1.pos_err, p2.pos_err)):
        assert np.array_equal(a, b)
    assert p1.S == p2.S
    ao = A.rollout(kinova_chain, un[0], np.zeros((1, case.H, 11), np.float32), d.state, d.tpos, d.tquat, d.cfg)
    _check_rows("plan-after-step", 0, ao, p1.traj[None], np.float32([p1.S]))
    e.close()
    f.close()


# ------------------------------------------------------------------------------------------------- elites
def test_elites_are_rows_of_the_trajectory(kinova_chain):
    case = A.Case("K48-H20", 48, 20)
    e, veh, out, u0, st = _fly(case, kinova_chain)
    el = e.get_elites(8)
    S, traj = e.get_costs(), e.get_trajectory()
    assert np.array_equal(el.idx[0], np.argsort(S[0], kind="stable")[:8])
    assert np.array_equal(el.S[0], S[0][el.idx[0]])
    assert el.traj.shape == (1, 8, 20, 29) and np.array_equal(el.traj[0], traj[0][el.idx[0]])
    assert np.array_equal(el.ee_path[0], traj[0][el.idx[0]][..., 13:].reshape(8, 20, 4, 4)[..., :3, 3])
    e.close()


# ------------------------------------------------------------------------------------------------ refusal
def test_scene_engine_is_refused_on_the_device_too():
    from quadrotor_manipulator_mppi_amd import _capi as capi
    from quadrotor_manipulator_mppi_amd.engine import Engine, Scene, make_config
    with pytest.raises(capi.MPPIError, match="AERIAL"):
        Engine(make_config(model="aerial"), scene=Scene(((-1, (0.0, 0.0, 0.0), 0.3),)))
    with pytest.raises(capi.MPPIError, match="AERIAL"):
        Engine(make_config(model="aerial", cost_terms=("target_track",)))


def test_dropin_class_steps(kinova_chain):
    import torch
    from quadrotor_manipulator_mppi_amd.mppi_solver.aerial_mppi import MPPI
    d = A.DESIGNS[0]
    m = MPPI(n_samples=64, n_horizon=20, seed=5)
    m.set_state(d.x, d.v)
    m.update_joint(d.q, d.qd)
    m.target_pose.pose = torch.tensor(d.tpos, dtype=torch.float32)
    m.target_pose.orientation = torch.tensor(d.tquat, dtype=torch.float32)
    x_des, v_des, qdes, vdes = m.compute_control_input()
    assert x_des.shape == (6,) and v_des.shape == (6,) and qdes.shape == (7,) and vdes.shape == (7,)
    want, b = Q.first_step_outputs(d.x, d.v, m.u.numpy()[:4], d.cfg)
    got = np.concatenate([x_des.cpu().numpy(), v_des.cpu().numpy()]).astype(np.float64)
    assert (np.abs(got - want) <= b + 2.0 ** -23 * np.abs(want)).all()   # (the class returns float32 tensors: one more rounding)
    assert m.get_trajectory().shape == (64, 20, 29) and m.get_plan().traj.shape == (20, 29) and m.get_elites(4).idx.shape == (4,)
    assert m.u_prev.shape == (20, 11)
    m._engine.close()   # (its native queue with it: nothing of this file outlives it in the process)
