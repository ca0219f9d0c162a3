"""The aerial manipulator model (MPPI_MODEL_AERIAL = 4) at the C-ABI, without a GPU: defaults, dims and
every refusal the header lists, the layout and the launches through the existing debug hooks, the symbols
of every block form in the new unit's code object, the Philox words of 11 dims, the host-formed base outputs
against quad_oracle's step 0, and the Python class's surface.  On the commit before the model these fail:
mppi_config_default(4) leaves a config mppi_debug_layout refuses as ``unknown model 4``."""
import ctypes as C

import numpy as np
import pytest

import quad_oracle as Q
from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd import build as B
from quadrotor_manipulator_mppi_amd.engine import Scene, SelfCollision, DistanceField, make_config

UNIT = "mppi_rollout_aerial.hip"


def _lib():
    L = capi.lib()
    L.mppi_debug_layout.restype = C.c_int32
    L.mppi_debug_layout.argtypes = [C.POINTER(capi.Config), C.POINTER(C.c_int32), C.c_int32]
    L.mppi_debug_step_launches.restype = C.c_int32
    L.mppi_debug_step_launches.argtypes = [C.POINTER(capi.Config), C.POINTER(C.c_int32), C.c_char_p, C.c_int32]
    L.mppi_debug_scene_step_launches.restype = C.c_int32
    L.mppi_debug_scene_step_launches.argtypes = [C.POINTER(capi.Config), C.POINTER(capi.Scene), C.POINTER(C.c_int32), C.c_char_p, C.c_int32]
    L.mppi_debug_field_step_launches.restype = C.c_int32
    L.mppi_debug_field_step_launches.argtypes = [C.POINTER(capi.Config), C.POINTER(capi.Scene), C.POINTER(capi.FieldDesc),
                                                 C.POINTER(C.c_int32), C.c_char_p, C.c_int32, C.POINTER(C.c_uint64)]
    L.mppi_debug_self_step_launches.restype = C.c_int32
    L.mppi_debug_self_step_launches.argtypes = [C.POINTER(capi.Config), C.POINTER(capi.Scene), C.POINTER(capi.FieldDesc),
                                                C.POINTER(capi.SelfCollision), C.POINTER(C.c_int32), C.c_char_p, C.c_int32]
    L.mppi_debug_plan_kernel.restype = C.c_int32
    L.mppi_debug_plan_kernel.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_int32]
    L.mppi_debug_base_outputs.restype = C.c_int32
    L.mppi_debug_base_outputs.argtypes = [C.POINTER(capi.Config), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_double),
                                          C.POINTER(C.c_float)]
    return L


def _layout(cfg):
    L = _lib()
    out = (C.c_int32 * 28)()
    st = L.mppi_debug_layout(C.byref(cfg), out, 28)
    return st, list(out), L.mppi_last_error().decode()


def _launches(cfg, path=1, n=1):
    L = _lib()
    sw = (C.c_int32 * 7)(path, n, 0, 0, 0, 0, 0)
    buf = C.create_string_buffer(8192)
    st = L.mppi_debug_step_launches(C.byref(cfg), sw, buf, len(buf))
    return st, buf.value.decode().splitlines(), L.mppi_last_error().decode()


# ------------------------------------------------------------------------------------------------- config
def test_abi_is_still_10_and_the_struct_has_not_moved():
    L = _lib()
    assert L.mppi_abi_version() == 10 == capi.ABI_VERSION
    s = [C.c_int32() for _ in range(3)]
    L.mppi_struct_sizes(*[C.byref(x) for x in s])
    assert s[0].value == C.sizeof(capi.Config)
    assert capi.MODEL_AERIAL == 4


def test_defaults_and_dims():
    L = _lib()
    c = capi.Config()
    L.mppi_config_default(C.byref(c), capi.MODEL_AERIAL)
    assert (c.model, c.n_samples, c.n_horizon, c.n_action) == (4, 100, 32, 11)
    sig = np.asarray(list(c.sigma), np.float32)[:121].reshape(11, 11)
    assert np.array_equal(sig, np.diag(np.float32([30, 1, 1, 1] + [0.1] * 7)))
    assert (c.savgol_window, c.savgol_order) == (9, 2)
    assert (c.w_stage_pos, c.w_stage_ori, c.w_term_pos, c.w_term_ori) == (50.0, 30.0, 40.0, 30.0)
    assert c.state_f64 == 0 and c.check_reach == 0 and c.cost_terms == 0 and c.shard_count == 1
    assert (c.quad_mass, tuple(c.quad_inertia)) == (np.float32(14.7), tuple(np.float32([1.57, 3.93, 2.59])))
    assert L.mppi_state_dim(C.byref(c)) == 26 and L.mppi_output_dim(C.byref(c)) == 26
    assert L.mppi_traj_channels(C.byref(c)) == 29
    c.n_samples, c.n_horizon = 4096, 32
    assert L.mppi_rollout_bytes(C.byref(c)) == 4096 * 32 * 25 * 4 + 4096 * 4
    cfg = make_config("aerial")
    assert cfg.n_joints > 7 and cfg.n_action == 11
    st, lay, msg = _layout(cfg)
    assert st == capi.OK, msg


def test_state_f64_is_forced_off_as_for_wholebody():
    cfg = make_config("aerial", state_f64=True)
    st, lines, msg = _launches(cfg)
    assert st == capi.OK, msg   # (the engine's copy runs fp32: the launches are those of state_f64 = 0)
    assert lines == _launches(make_config("aerial"))[1]


# ----------------------------------------------------------------------------------------------- refusals
def _refused(cfg, needle):
    st, _, msg = _layout(cfg)
    assert st == capi.ERR_INVALID_ARG, (st, msg)
    assert "AERIAL" in msg and needle in msg, msg


def test_refusals_name_the_model():
    _refused(make_config("aerial", n_action=10, sigma=np.eye(10) * 0.1), "n_action")
    _refused(make_config("aerial", n_horizon=65), "H <= 64")
    for bits in (capi.COST_COVAR, capi.COST_CENTER, capi.COST_JOINT_TRACK, capi.COST_ACTION, capi.COST_JOINT_LIMIT,
                 capi.COST_TARGET_TRACK, capi.COST_TARGET_TRACK | capi.COST_CENTER):
        _refused(make_config("aerial", cost_terms=bits), "cost_terms")
    _refused(make_config("aerial", shard_count=2), "shard")
    _refused(make_config("aerial", quad=dict(quad_mass=0.0)), "mass")
    _refused(make_config("aerial", quad=dict(quad_inertia=(1.0, -1.0, 1.0))), "inertia")
    # the chain checks of the arm models
    cfg = make_config("aerial")
    cfg.n_joints = 0
    st, _, msg = _layout(cfg)
    assert st == capi.ERR_INVALID_ARG and "n_joints" in msg
    cfg = make_config("aerial")
    cfg.joints[cfg.n_joints - 1].axis[0] = 1.0   # no longer a revolute-z chain: not the Kinova table
    _refused(cfg, "Kinova")


def test_scene_field_and_self_engines_are_refused():
    L = _lib()
    cfg = make_config("aerial")
    sw = (C.c_int32 * 7)(1, 1, 0, 0, 0, 0, 0)
    buf = C.create_string_buffer(4096)
    arm = make_config("arm")
    sc = Scene.default(arm).to_c()
    assert L.mppi_debug_scene_step_launches(C.byref(cfg), C.byref(sc), sw, buf, len(buf)) == capi.ERR_INVALID_ARG
    assert "AERIAL" in L.mppi_last_error().decode()
    fd = DistanceField((4, 4, 4), 0.1).to_c()
    assert L.mppi_debug_field_step_launches(C.byref(cfg), C.byref(sc), C.byref(fd), sw, buf, len(buf), None) == capi.ERR_INVALID_ARG
    assert "AERIAL" in L.mppi_last_error().decode()
    sf = SelfCollision.default(arm, Scene.default(arm)).to_c()
    assert L.mppi_debug_self_step_launches(C.byref(cfg), C.byref(sc), None, C.byref(sf), sw, buf, len(buf)) == capi.ERR_INVALID_ARG
    assert "AERIAL" in L.mppi_last_error().decode()
    assert Scene.default(cfg).body == ()   # no placeholder spheres for a model without a scene kernel


# ------------------------------------------------------------------------------------------------- layout
def _lds(H, nwd):
    return 4 * ((H + 1) * (16 * nwd * 11 + 1) + (H + 1) * 11 + 16 * nwd * (H + 1) * 7)


@pytest.mark.parametrize("K,H,V,nb,iters", [
    (100, 32, 1, 7, 1), (16, 32, 1, 1, 1), (17, 20, 1, 2, 1), (48, 64, 2, 3, 1), (4096, 32, 1, 256, 1), (4096, 32, 3, 256, 1),
    (16384, 32, 1, 1024, 1),
    (16400, 20, 1, 257, 4),        # above 1024 blocks: four dynamics waves, 64 rollouts per block
    (16400, 32, 1, 1025, 1),       # ... where their tiles fit: at H = 32 they do not (154 KB)
    (8192, 64, 1, 512, 1)])
def test_layout_words(K, H, V, nb, iters):
    st, w, msg = _layout(make_config("aerial", n_samples=K, n_horizon=H, n_vehicles=V))
    assert st == capi.OK, msg
    threads, L, R, nch, gnb, giters, P, Cc, hp = w[:9]
    assert (gnb, giters, threads) == (nb, iters, 256)
    assert Cc == 25 and hp == (H + 15) // 16 * 16 and P == (4 + 11 * H + 3) // 4 * 4
    assert w[11:18] == [w[11], 2, 1, 7, 4, 26, 26] and w[11] >= 1   # j0 (the folded fixed joints), Kinova, diag Sigma, nq, qoff, dims
    assert _lds(H, iters) <= 128 * 1024
    if iters == 1 and (K + 15) // 16 * V > 1024:
        assert _lds(H, 4) > 128 * 1024


@pytest.mark.parametrize("V,K,H,lit,nwd,nt", [
    (1, 100, 32, 0, 1, 512), (1, 100, 32, 1, 1, 512),          # wide: at most 512 blocks
    (3, 4096, 32, 0, 1, 256), (3, 4096, 32, 1, 1, 256),        # 768 blocks: one dynamics wave in 256 threads
    (1, 16400, 20, 0, 4, 256), (1, 16400, 20, 1, 4, 256),      # four dynamics waves
    (2, 16400, 20, 0, 4, 256), (1, 12000, 64, 1, 1, 256)])
def test_symbols_are_in_the_new_unit(V, K, H, lit, nwd, nt):
    assert UNIT in B.KERNEL_UNITS
    cfg = make_config("aerial", n_samples=K, n_horizon=H, n_vehicles=V, quad=dict(quad_literal_jinv=bool(lit)))
    with open(B.code_object_path(B.LIB, UNIT), "rb") as f:
        blob = f.read()
    want = f"_Z16k_rollout_aerialILb{int(V == 1)}ELb{lit}ELi{nwd}ELi{nt}EEvjjjjiiPKfN4mppi9DevParamsE"
    for path, n in ((1, 1), (0, 3), (2, 3)) + (((3, 1),) if V == 1 else ()):
        st, lines, msg = _launches(cfg, path, n)
        assert st == capi.OK, msg
        rolls = [ln.split() for ln in lines if ln.split()[1] == "rollout"]
        assert rolls and all(r[2] == want for r in rolls), (path, rolls)   # no quiet form: every step the full kernel
        nb = (K + 16 * nwd - 1) // (16 * nwd)
        for r in rolls:
            assert (int(r[4]), int(r[6]), int(r[8])) == (nb, nt, _lds(H, nwd)), r
        fins = [ln.split() for ln in lines if ln.split()[1] == "finalize"]
        assert fins and all(f[2].startswith("_Z10k_finalizeILi16ELi9E") for f in fins), fins   # run-time geometry, 9 taps
    assert (want + ".kd").encode() in blob
    others = [u for u in B.KERNEL_UNITS if u != UNIT and (want + ".kd").encode() in open(B.code_object_path(B.LIB, u), "rb").read()]
    assert not others, others


def test_no_scratch_in_the_new_kernels():
    res = B.kernel_resources(B.code_object_path(B.LIB, UNIT))
    mine = {k: v for k, v in res.items() if "k_rollout_aerial" in k}
    assert len(mine) == 12, sorted(mine)   # V == 1 / V > 1, both quad_literal_jinv values, three block forms
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["vspill"] == 0, (k, v)   # (a scalar spill goes to VGPR lanes: no private segment)
    plan = B.kernel_resources(B.code_object_path(B.LIB, "mppi_plan.hip"))
    pa = {k: v for k, v in plan.items() if "k_plan_aerial" in k}
    assert len(pa) == 2 and all(v["scratch"] == 0 for v in pa.values()), pa


def test_plan_kernel():
    L = _lib()
    buf = C.create_string_buffer(512)
    for lit in (0, 1):
        g = (C.c_int32 * 6)(capi.MODEL_AERIAL, 11, 33, 3, 0, lit)
        assert L.mppi_debug_plan_kernel(g, buf, len(buf)) == capi.OK
        assert buf.value.decode() == f"_Z13k_plan_aerialILb{lit}EEvPKfPKN4mppi8JointDevENS2_10PlanParamsENS2_9DevParamsE grid 3 block 64"
    g = (C.c_int32 * 6)(capi.MODEL_AERIAL, 10, 32, 1, 0, 0)
    assert L.mppi_debug_plan_kernel(g, buf, len(buf)) == capi.ERR_INVALID_ARG


def test_philox_words_of_eleven_dims():
    assert _lib().mppi_philox_words(11) == 6   # one Philox4x32 call and one Philox2x32 call


# ------------------------------------------------------------------------------------------------ outputs
def test_host_formed_base_outputs_and_vehicle_constants():
    L = _lib()
    rng = np.random.default_rng(3)
    for d in (Q.BY_NAME["hover"], Q.BY_NAME["pitch_p120"], Q.BY_NAME["body2"], Q.BY_NAME["drag_near"]):
        q, qd = rng.uniform(-3, 3, 7), rng.uniform(-1, 1, 7)
        state = np.concatenate([d.x, q, d.v, qd]).astype(np.float64)
        u0 = np.concatenate([[Q._f(d.cfg.mass) * Q._f(d.cfg.gravity) * 1.1, 0.3, -0.2, 0.1], rng.normal(0, 1, 7)]).astype(np.float32)
        cfg = make_config("aerial", dt=d.cfg.dt, quad=d.cfg.quad(False))
        out = np.full(12, np.nan)
        vc = np.zeros(44, np.float32)
        st = L.mppi_debug_base_outputs(C.byref(cfg), capi.dptr(state), capi.fptr(u0), capi.dptr(out), capi.fptr(vc))
        assert st == capi.OK, L.mppi_last_error().decode()
        want, b = Q.first_step_outputs(d.x, d.v, u0[:4], d.cfg)
        assert (np.abs(out - want) <= b).all(), (d.name, np.abs(out - want) / b)
        # the same numbers as the QUADROTOR model's own host step, bit for bit
        qcfg = make_config("quadrotor", dt=d.cfg.dt, quad=d.cfg.quad(False))
        qout = np.full(12, np.nan)
        assert L.mppi_debug_base_outputs(C.byref(qcfg), capi.dptr(np.asarray(d.state, np.float64)), capi.fptr(u0[:4].copy()),
                                         capi.dptr(qout), None) == capi.OK
        assert np.array_equal(out, qout)
        # the vehicle constants: xyz / v in 0..2, q / qd at the joints' action dims 4..10, rpy / omega in 11..13
        pos, vel, base = vc[:16], vc[16:32], vc[32:].reshape(3, 4)
        f = np.float32
        assert np.array_equal(pos[:3], f(d.x[:3])) and np.array_equal(pos[11:14], f(d.x[3:])) and np.array_equal(pos[4:11], f(q))
        assert np.array_equal(vel[:3], f(d.v[:3])) and np.array_equal(vel[11:14], f(d.v[3:])) and np.array_equal(vel[4:11], f(qd))
        assert pos[3] == 0 and vel[3] == 0 and not pos[14:].any()
        # base = M_fixed alone: the product of the chain's leading fixed joints, no state in it
        M = np.eye(4)
        for j in range(cfg.n_joints):
            if cfg.joints[j].type != capi.JOINT_FIXED:
                break
            T = np.zeros(16, np.float32)
            L.mppi_joint_origin(C.byref(cfg.joints[j]), capi.fptr(T))
            M = M @ T.reshape(4, 4).astype(np.float64)
        assert np.allclose(base, M[:3], rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------- Python
def test_class_surface():
    import torch
    from quadrotor_manipulator_mppi_amd.mppi_solver._base import SolverBase
    from quadrotor_manipulator_mppi_amd.mppi_solver.aerial_mppi import MPPI
    m = MPPI()
    assert isinstance(m, SolverBase) and m.n_action == 11 and (m.n_samples, m.n_horizon) == (100, 32)
    assert m.u.shape == (11,) and m.u_prev.shape == (32, 11)
    up = m.u_prev.numpy()
    assert np.all(up[:, 0] == np.float32(14.7 * 9.81)) and not up[:, 1:].any()   # warm start at hover thrust
    assert torch.equal(m.sigma, torch.diag(torch.tensor([30.0, 1, 1, 1] + [0.1] * 7)))
    for name in ("set_state", "update_joint", "compute_control_input", "get_plan", "get_elites", "get_trajectory", "get_costs"):
        assert callable(getattr(m, name)), name
    m.set_state([0.1, 0.2, 1.0, 0.3, -0.2, 0.5], [[0.0, 0.1, 0.2], [1.0, 2.0, 3.0]])
    assert m.x_prev.dtype == torch.float32 and m.v_prev.tolist() == [0.0, np.float32(0.1), np.float32(0.2), 1.0, 2.0, 3.0]
    m.update_joint(np.arange(7.0), -np.arange(7.0))
    assert m._q.dtype == np.float32 and m._q.tolist() == list(range(7)) and m._qdot[3] == -3.0
    cfg = m._config((False, 64, 20))
    assert (cfg.model, cfg.n_samples, cfg.n_horizon, cfg.n_action, cfg.cost_terms) == (capi.MODEL_AERIAL, 64, 20, 11, 0)
    assert _layout(cfg)[0] == capi.OK
    hv = MPPI(mass=2.0, gravity=3.71, inertia=(0.1, 0.2, 0.3))
    assert hv.u_prev[0, 0] == np.float32(2.0 * 3.71) and hv._config((False, 8, 8)).quad_mass == 2.0
    for kw in (dict(scene=True), dict(field=DistanceField((4, 4, 4), 0.1)), dict(self_collision=True), dict(track_target=True)):
        with pytest.raises(NotImplementedError, match="aerial manipulator"):
            MPPI(**kw)
    with pytest.raises(RuntimeError):
        m.set_target_trajectory(np.zeros((32, 7)))
