"""GPU tests of the elite readback (mppi_get_elites, csrc/mppi_elites.hip): the n lowest-cost
samples of the last rollout, selected, sorted and gathered on the device.

The reference is the engine's existing readbacks, never the code under test:
    order = np.argsort(e.get_costs()[v], kind="stable")[:n]
    idx == order, S == get_costs()[v, order], w == get_weights()[v, order],
    traj == get_trajectory()[v, order]
all exact, bit for bit (compared as uint32 words, so NaN payloads and signed zeros count): the
selection and the gather copy values, and w is k_weights' own expression over the same rho and eta.

S_A = 4096 is the share of the costs one stage-A block selects from (csrc/mppi_elites.h
kEliteShare): K <= S_A takes one launch of the selection, K > S_A the two stages.
"""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

S_A = 4096
TPOS, TQUAT = [0.1029, 0.4055, 1.6498], [-0.5, -0.5, 0.5, -0.5]
HOME = [1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0]
RATES = [0.8, -0.5, 0.3, -1.2, 0.4, 0.9, -0.7]
ARM_STATE = np.array([0.1, -0.2, 1.1, 0.0, 0.0, 0.2588190, 0.9659258] + HOME + RATES, np.float64)
WB_STATE = np.array([0.3, -0.1, 1.2, 0.0, 0.0, 0.1305262, 0.9914449] + HOME + [0.5, -0.4, 0.2] + RATES, np.float64)
DRONE_STATE = np.array([0.1, 0.2, 1.0, 0.3, -0.2, 0.1], np.float64)
DRONE_TARGET = [1.0, 2.0, 3.4]
QUAD_STATE = np.array([0.2, -0.1, 2.5, 0.05, -0.08, 0.7, 0.3, 0.2, -0.1, 0.2, -0.1, 0.05], np.float64)


def _engine(model, **kw):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    e = Engine(make_config(model=model, **kw))
    for v in range(e.V):
        if model in ("drone", "quadrotor"):
            e.set_target(DRONE_TARGET, vehicle=v)
        else:
            e.set_target(TPOS, TQUAT, vehicle=v)
    return e


def _state(model, V=1):
    s = {"arm": ARM_STATE, "wholebody": WB_STATE, "drone": DRONE_STATE, "quadrotor": QUAD_STATE}[model]
    return np.tile(s, (V, 1))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0]}"


def _reference(e, traj=True):
    """The existing readbacks, read once per engine state."""
    return e.get_costs(), e.get_weights(), (e.get_trajectory() if traj else None)


def _check(e, n, ref=None, traj=True, w=True, what=""):
    S, W, T = ref if ref is not None else _reference(e, traj)
    el = e.get_elites(n, traj)
    assert el.idx.shape == (e.V, n) and el.idx.dtype == np.int32 and el.S.shape == (e.V, n) and el.w.shape == (e.V, n)
    for v in range(e.V):
        order = np.argsort(S[v], kind="stable")[:n]
        np.testing.assert_array_equal(el.idx[v], order, err_msg=f"{what} vehicle {v}: idx")
        _same_bits(el.S[v], S[v, order], f"{what} vehicle {v}: S")
        if w:
            _same_bits(el.w[v], W[v, order], f"{what} vehicle {v}: w")
        if traj:
            assert el.traj.shape == (e.V, n, e.H, e.traj_channels)
            _same_bits(el.traj[v], T[v, order], f"{what} vehicle {v}: traj")
            pos = T[v, order][..., e.A:].reshape(n, e.H, 4, 4)[..., :3, 3] if T.shape[-1] > 6 else T[v, order][..., :3]
            _same_bits(el.ee_path[v], pos, f"{what} vehicle {v}: ee_path")
        else:
            assert el.traj is None and el.ee_path is None
    return el


# ------------------------------------------------------------------ 1. the arm fixture's shape
def test_arm_fixture_shape():
    """K = 32, H = 32, fp32 state, the fixture's injected noise; n = K is a full sort."""
    g = load_golden("arm_k32_h32_f32.npz")
    e = _engine("arm", n_samples=32, n_horizon=32, state_f64=False, noise="injected")
    e.set_target(g["target_pos"], g["target_quat"])
    e.step(np.concatenate([g["q_full"][:7], g["q_full"][7:], g["v_full"][6:]]), g["s0_noise"])
    ref = _reference(e)
    for n in (1, 5, 32):
        _check(e, n, ref, what=f"n={n}")


# ------------------------------------- 2. K off the wave and the share; across the stage boundary
@pytest.mark.parametrize("model,K,H,n", [("arm", 100, 32, 7), ("drone", 5000, 20, 64), ("drone", S_A, 20, 64),
                                         ("drone", S_A + 1, 20, 64), ("drone", 2 * S_A - 1, 20, 64)])
def test_odd_sample_counts(model, K, H, n):
    """K not a multiple of 64 or of S_A; drone H = 20 has padded rows (hp = 32); S_A, S_A + 1 and
    2 S_A - 1 straddle the one-launch / two-stage boundary (a last share of 1 and of S_A - 1)."""
    e = _engine(model, n_samples=K, n_horizon=H, seed=5)
    e.step(_state(model))
    _check(e, n, what=f"{model} K={K}")


# --------------------------------------------------------------------------------- 3. large K
def test_large_sample_count():
    e = _engine("drone", n_samples=65536, n_horizon=20, seed=6)
    e.step(_state("drone"))
    ref = _reference(e)
    for n in (1, 64):
        _check(e, n, ref, what=f"K=65536 n={n}")


def test_shares_beyond_the_register_cache():
    """K > 256 S_A: the stage-A blocks are capped at 256, so their shares grow past S_A and are read
    again each pass instead of kept in registers, and stage B reads 256 * 64 candidates the same way
    (no planes: 1 M rollouts' trajectories would be 400 MB; the selection does not touch them)."""
    K = 256 * S_A + 4097
    e = _engine("drone", n_samples=K, n_horizon=20, store_trajectory=False, seed=17)
    e.step(_state("drone"))
    ref = _reference(e, traj=False)
    for n in (1, 64):
        _check(e, n, ref, traj=False, what=f"K={K} n={n}")


# -------------------------------------------------------------------------------- 4. row pitch
@pytest.mark.parametrize("H,f64", [(100, True), (256, False)])
def test_arm_row_pitch(H, f64):
    """H = 100: hp = 112; H = 256: k_rollout's four-chunk path, the same plane layout."""
    e = _engine("arm", n_samples=64, n_horizon=H, state_f64=f64, seed=7)
    e.step(_state("arm"))
    _check(e, 16, what=f"arm H={H}")


# ------------------------------------------------------------------ 5., 6. whole-body, quadrotor
def test_wholebody_rows():
    """C = 22 planes into rows of 26: the state, the EE's twelve entries, 0 0 0 1."""
    e = _engine("wholebody", n_samples=128, n_horizon=64, seed=8)
    e.step(_state("wholebody"))
    el = _check(e, 16, what="wholebody")
    assert el.traj.shape[-1] == 26
    np.testing.assert_array_equal(el.traj[..., 22:], np.broadcast_to(np.float32([0, 0, 0, 1]), el.traj[..., 22:].shape))


def test_quadrotor_t_major_planes():
    """(C,H,Kp) planes with Kp = 112."""
    e = _engine("quadrotor", n_samples=100, n_horizon=32, seed=9)
    e.step(_state("quadrotor"))
    _check(e, 9, what="quadrotor")


# ----------------------------------------------------------------------------------- 7. fleets
def test_fleet_every_vehicle_its_own_elites():
    V = 3
    e = _engine("arm", n_samples=64, n_horizon=32, n_vehicles=V, seed=10)
    for v, t in enumerate(([0.1029, 0.4055, 1.6498], [0.3, 0.2, 1.4], [-0.2, 0.5, 1.8])):
        e.set_target(t, TQUAT, vehicle=v)
    e.step(_state("arm", V))
    ref = _reference(e)
    orders = [tuple(np.argsort(ref[0][v], kind="stable")[:8]) for v in range(V)]
    assert len(set(orders)) == V, "the vehicles' elites must differ for the case to mean anything"
    _check(e, 8, ref, what="arm fleet")


def test_fleet_without_stored_trajectories():
    from quadrotor_manipulator_mppi_amd import _capi as capi
    V = 64
    e = _engine("drone", n_samples=64, n_horizon=20, n_vehicles=V, store_trajectory=False, seed=11)
    e.step(_state("drone", V))
    _check(e, 8, traj=False, what="drone fleet")
    with pytest.raises(capi.MPPIError) as err:
        e.get_elites(8, traj=True)
    assert err.value.status == capi.ERR_STATE and "store_trajectory" in str(err.value)
    _check(e, 8, traj=False, what="drone fleet after the refusal")


# ------------------------------------------------------------------------------------- 8. ties
def _pose_of(ee16):
    """(position, quaternion xyzw) of an EE matrix."""
    T = np.asarray(ee16, np.float64).reshape(4, 4)
    R = T[:3, :3]
    w = 0.5 * np.sqrt(max(1e-12, 1.0 + R[0, 0] + R[1, 1] + R[2, 2]))
    q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (4.0 * w)
    return [float(x) for x in T[:3, 3]], [float(q[0]), float(q[1]), float(q[2]), float(w)]


def test_ties_go_by_the_lower_index():
    K, H = 64, 32
    e = _engine("arm", n_samples=K, n_horizon=H, state_f64=True, noise="injected")
    rest = ARM_STATE.copy()
    rest[14:] = 0.0   # at rest, so the zero-noise rollout stays where it is
    zeros = np.zeros((1, K, H, 7), np.float32)
    e.step(rest, zeros)
    S = e.get_costs()
    assert len(np.unique(_bits(S))) == 1, "precondition: one unique cost"
    ref = _reference(e)
    for n in (1, 16, 64):
        el = _check(e, n, ref, what=f"all equal n={n}")
        np.testing.assert_array_equal(el.idx[0], np.arange(n))
    # the target on the resting EE: standing still is the best a sample can do, so the odd (zero
    # noise) samples tie below every even (moving) one
    e.set_target(*_pose_of(ref[2][0, 0, 0, 7:]))
    e.set_u_prev(np.zeros((1, H, 7), np.float32))
    noise = np.random.default_rng(12).normal(0.0, 2.0, (1, K, H, 7)).astype(np.float32)
    noise[:, 1::2] = 0.0
    e.step(rest, noise)
    S = e.get_costs()[0]
    assert len(np.unique(_bits(S[1::2]))) == 1, "precondition: the odd samples' costs are equal"
    assert (S[0::2] > S[1]).all(), "precondition: every even sample is strictly worse"
    ref = _reference(e)
    for n in (1, 16, 32):
        el = _check(e, n, ref, what=f"odd samples tie n={n}")
        np.testing.assert_array_equal(el.idx[0], 1 + 2 * np.arange(n))
    el = _check(e, 40, ref, what="odd samples tie n=40")   # past the tie: the best evens follow
    np.testing.assert_array_equal(el.idx[0, :32], 1 + 2 * np.arange(32))
    assert (el.idx[0, 32:] % 2 == 0).all()


# ------------------------------------------------------------------------------- 9. non-finite
def test_nan_cost_sorts_last():
    g = load_golden("arm_k32_h32_f32.npz")
    noise = g["s0_noise"].copy()
    noise[5, 3, 1] = np.nan
    e = _engine("arm", n_samples=32, n_horizon=32, state_f64=False, noise="injected")
    e.set_target(g["target_pos"], g["target_quat"])
    e.step(np.concatenate([g["q_full"][:7], g["q_full"][7:], g["v_full"][6:]]), noise)
    S = e.get_costs()
    assert np.isnan(S[0, 5]) and np.isnan(S[0]).sum() == 1
    ref = (S, None, None)
    el = _check(e, 31, ref, traj=False, w=False, what="n=31")
    assert 5 not in el.idx[0]
    el = _check(e, 32, ref, traj=False, w=False, what="n=32")
    assert el.idx[0, -1] == 5 and np.isnan(el.S[0, -1])


# ----------------------------------------------------------------------- 10. after a native batch
def test_after_a_batch_the_last_steps_elites():
    """The batch's last step is what all four readbacks see (its steps before ran the quiet kernels,
    which write neither costs nor planes); asked straight after run_steps, the call joins the batch."""
    e = _engine("arm", n_samples=512, n_horizon=32, state_f64=True, seed=13)
    e.set_state(_state("arm"))
    e.run_steps(6)
    e.synchronize()
    info = e.kernel_info().split("; call:")[0]
    assert "quiet rollout none" not in info and "quiet finalize none" not in info, info
    _check(e, 16, what="after run_steps(6)")
    e2 = _engine("arm", n_samples=512, n_horizon=32, state_f64=True, seed=13)
    e2.set_state(_state("arm"))
    e2.run_steps(6)
    el = e2.get_elites(16)   # (nothing synchronised in between)
    ref = _reference(e2)
    order = np.argsort(ref[0][0], kind="stable")[:16]
    np.testing.assert_array_equal(el.idx[0], order)
    _same_bits(el.S[0], ref[0][0, order], "S straight after the batch")
    _same_bits(el.traj[0], ref[2][0, order], "traj straight after the batch")


# -------------------------------------------------------------------------- 11. disturbs nothing
def test_elites_leave_the_engine_undisturbed():
    """get_elites with growing and shrinking n between control calls and around a batch: outputs,
    warm start, costs and planes bit-identical to a twin engine's that never asks."""
    seen = []
    for ask in (False, True):
        e = _engine("arm", n_samples=512, n_horizon=32, state_f64=True, seed=14)
        st = _state("arm")
        rec = []

        def elites(n):
            if ask:
                el = e.get_elites(n)
                assert np.isfinite(el.S).all() and (el.idx >= 0).all() and (el.idx < e.K).all()

        def snap(outs=None):
            e.synchronize()
            out, u0, stats = outs if outs else e.read_outputs()
            rec.append((out.tobytes(), u0.tobytes(), [(s.rho, s.eta, s.ess, s.nonfinite) for s in stats],
                        e.get_u_prev().tobytes(), e.get_costs().tobytes(), e.get_trajectory().tobytes()))

        for n in (4, 64, 4):
            snap(e.step(st))
            elites(n)
        e.run_steps(5)
        elites(64)
        snap()
        elites(4)
        snap(e.step(st))
        seen.append(rec)
    assert len(seen[0]) == len(seen[1]) == 5
    for i, (a, b) in enumerate(zip(*seen)):
        assert a == b, f"stage {i}: the engine that read its elites differs"


# -------------------------------------------------------------------------------- 12. sharded
def test_merge_of_two_shards_equals_one_engine():
    import torch
    from quadrotor_manipulator_mppi_amd.distributed import merge_elites
    kw = dict(n_horizon=32, state_f64=True, seed=15)
    one = _engine("arm", n_samples=512, **kw)
    shards = [_engine("arm", n_samples=256, shard_rank=r, shard_count=2, **kw) for r in range(2)]
    bufs = [torch.zeros(2 * sh.exchange_slot_floats(), device="cuda") for sh in shards]
    for sh, b in zip(shards, bufs):
        sh.bind_exchange(b.data_ptr())
    for e in [one] + shards:
        e.set_state(_state("arm"))
        e.rollout()
        e.synchronize()
    S = one.get_costs()
    assert _bits(np.concatenate([sh.get_costs() for sh in shards], axis=1)).tobytes() == _bits(S).tobytes(), \
        "precondition: the shards' costs are the one engine's, per global sample"
    n = 16
    parts = []
    for r, sh in enumerate(shards):
        el = _check(sh, n, w=False, what=f"shard {r}")
        el.idx = el.idx.astype(np.int64) + r * sh.K
        parts.append(el)
    m = merge_elites(parts, n)
    want = _check(one, n, w=False, what="one engine")
    np.testing.assert_array_equal(m.idx, want.idx)
    _same_bits(m.S, want.S, "merged S")
    _same_bits(m.traj, want.traj, "merged traj")
    _same_bits(m.ee_path, want.ee_path, "merged ee_path")


# ------------------------------------------------------------------------------- 13. drop-ins
def test_dropin_get_elites():
    from quadrotor_manipulator_mppi_amd.mppi_solver.drone_mppi import MPPI as DroneMPPI
    from quadrotor_manipulator_mppi_amd.mppi_solver.mppi import MPPI
    from quadrotor_manipulator_mppi_amd.mppi_solver.quadrotor_mppi import MPPI as QuadMPPI
    g = load_golden("arm_k100_h32_f64.npz")
    arm = MPPI(verbose=False)
    arm.update_joint(g["q_full"], g["v_full"])
    drone = DroneMPPI(n_samples=128, n_timestep=20)
    drone.set_state([0.1, 0.2, 1.0], [0.3, -0.2, 0.1])
    quad = QuadMPPI(n_samples=128)
    quad.set_state(QUAD_STATE[:6], QUAD_STATE[6:])
    for m, C, ee in ((arm, 23, True), (drone, 3, False), (quad, 6, False)):
        m.compute_control_input()
        el = m.get_elites(8)
        H = m._engine.H
        assert el.idx.shape == (8,) and el.S.shape == (8,) and el.w.shape == (8,)
        assert el.traj.shape == (8, H, C) and el.ee_path.shape == (8, H, 3)
        order = np.argsort(m.get_costs(), kind="stable")[:8]
        np.testing.assert_array_equal(el.idx, order)
        last = m.get_trajectory()[order[0], -1]
        _same_bits(el.ee_path[0, -1], last[7:].reshape(4, 4)[:3, 3] if ee else last[:3], "elite 0's last position")


# ------------------------------------------------------------------------ 14. argument errors
def test_argument_errors_leave_the_engine_stepping():
    from quadrotor_manipulator_mppi_amd import _capi as capi
    e = _engine("drone", n_samples=48, n_horizon=20, seed=16)
    e.step(_state("drone"))
    for n in (0, 65, 49, -3):
        with pytest.raises(capi.MPPIError) as err:
            e.get_elites(n)
        assert err.value.status == capi.ERR_INVALID_ARG, n
    out, u0, st = e.step(_state("drone"))
    assert np.isfinite(out).all() and not st[0].nonfinite
    _check(e, 48, what="n = K after the refusals")
