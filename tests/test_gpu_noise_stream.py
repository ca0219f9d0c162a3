"""The fused rollout kernels' device noise against the Philox stream DESIGN.md §4 specifies.

Every accuracy test elsewhere feeds the oracle the noise the GPU drew itself; here the stored noise
of ``k_rollout`` / ``k_rollout_quad`` (``store_noise``) is held, element by element, to
``eps = draw_normals(k_global, t, fleet-wide vehicle, step, seed) Sigma`` as ``O.philox_normals``
restates it in float64 (tests/noise_stream.py: ``expected_eps`` / ``assert_stream``, the tolerance
of ``test_device_philox_matches_restatement`` carried through Sigma).  The five counter arguments
are computed by the kernels themselves (csrc/mppi_noise.h, mppi_rollout.h, mppi_rollout_quad.hip, mppi_device.h):

    kg   = k_off + (g * nw + wid) * R + sub,  g = blockIdx.x + it * nb     (looping kernel)
    t    = t0 + 64 c                                                         (H > 64)
    vkey = blockIdx.y + vehicle_offset
    step = the host's count (HIP launches) or step_arg + (dispatch id >> 1)  (native dispatch)
    k_off = shard_rank * K

and each case below is the smallest shape that exercises one of them; its id names the kernel
instantiation and the launch geometry (nb blocks per vehicle x iters groups per block, restated
from mppi_create by ``noise_stream.geometry`` and asserted against the literal in the case).

For a diagonal Sigma the stored noise is also compared bit for bit with ``z_gpu * diag(Sigma)``
in float32, ``z_gpu`` the ``k_philox`` readback (``engine.philox_normals``) at the same five
arguments: both kernels inline the same ``draw_normals`` and the rollout adds one fp32 multiply.

State, target and warm start do not enter the noise: home state, one target, zero ``u_prev``.
"""
import numpy as np
import pytest
import torch

from noise_stream import MODEL_A, assert_stream, geometry, sigma_matrix

pytestmark = pytest.mark.gpu

SEED = 2**40 + 7          # both key words non-zero
HOME_Q = [1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0]
ARM_TARGET = ([0.1029, 0.4055, 1.6498], [-0.5, -0.5, 0.5, -0.5])
STATE = {"drone": [0.0, 0.0, 1.0, 0.0, 0.0, 0.0],
         "quadrotor": [0.0, 0.0, 3.0, 0.0, 0.0, 0.0] + [0.0] * 6,
         "arm": [0, 0, 1, 0, 0, 0, 1] + HOME_Q + [0.0] * 7,
         "wholebody": [0, 0, 1, 0, 0, 0, 1] + HOME_Q + [0.0] * 10}
SIGMA = {"drone": np.diag([30.0] * 3).astype(np.float32),
         "quadrotor": np.diag([30.0, 1.0, 1.0, 1.0]).astype(np.float32),
         "arm": (np.eye(7) * 0.1).astype(np.float32),
         "wholebody": np.diag([30.0] * 3 + [0.1] * 7).astype(np.float32)}


def _full_sigma(model):
    """Non-diagonal and not symmetric (z Sigma, the row-vector convention, differs from Sigma z):
    the entries of test_gpu_fleet's full-Sigma cases plus one unequal pair."""
    s = SIGMA[model].copy()
    if model == "wholebody":
        s[0, 1] = s[1, 0] = 2.0
        s[4, 5] = s[5, 4] = 0.02
        s[0, 2], s[2, 0] = 1.0, -0.5
    else:
        s[0, 1] = s[1, 0] = 0.02
        s[2, 5], s[5, 2] = 0.03, -0.01
    return s


def _engine(model, K, H, V=1, seed=SEED, sigma=None, **kw):
    from quadrotor_manipulator_mppi_amd.engine import Engine, make_config
    sigma = SIGMA[model] if sigma is None else sigma
    e = Engine(make_config(model=model, n_samples=K, n_horizon=H, n_vehicles=V, seed=seed, sigma=sigma,
                           store_noise=True, store_trajectory=False, **kw))
    for v in range(V):
        if model in ("drone", "quadrotor"):
            e.set_target(np.asarray([1.0, 2.0, 3.4], np.float32), vehicle=v)
        else:
            e.set_target(*ARM_TARGET, vehicle=v)
    e.set_u_prev(np.zeros((V, H, MODEL_A[model]), np.float32))
    e.set_state(np.tile(np.asarray(STATE[model], np.float64), (V, 1)))
    return e


def _hip_step(e):
    """One control step as HIP launches (the step word is the host's count in the kernel argument;
    mppi_step on one vehicle would take the native path, which has its own test below)."""
    e.rollout()
    e.finalize()
    e.synchronize()


def _check(e, model, step, seed=SEED, sigma=None, k0=0, vehicle_offset=0, what=""):
    """All of get_noise() against the specification, vehicle by vehicle; for a diagonal Sigma also
    bit for bit against the k_philox readback times diag(Sigma)."""
    from quadrotor_manipulator_mppi_amd.engine import philox_normals
    sigma = SIGMA[model] if sigma is None else sigma
    A = MODEL_A[model]
    S = sigma_matrix(sigma, A)
    diagonal = not (S - np.diag(np.diag(S))).any()
    eps = e.get_noise()
    assert eps.shape == (e.V, e.K, e.H, A)
    ks = k0 + np.arange(e.K, dtype=np.int64)
    for v in range(e.V):
        veh = vehicle_offset + v
        assert_stream(eps[v], seed, step, veh, ks, e.H, A, sigma, what=f"{what} {model} vehicle {veh} step {step:#x}")
        if diagonal:
            _, z = philox_normals(seed, step & 0xFFFFFFFF, veh, k0, e.K, e.H, A)
            want = z * np.diag(np.asarray(sigma, np.float32))[None, None, :]
            assert want.dtype == np.float32
            same = eps[v] == want
            if not same.all():
                ulp = np.abs(eps[v].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
                print(f"{what} {model} vehicle {veh}: {int((~same).sum())} / {same.size} elements differ from "
                      f"z_gpu * diag(Sigma), max {int(ulp.max())} ulp")
            assert same.all(), f"{what} {model} vehicle {veh}: stored eps != k_philox z * diag(Sigma) bit for bit"
    return eps


def _geom(model, K, H, want, **kw):
    g = geometry(model, K, H, **kw)
    assert (g["nb"], g["iters"]) == want, (g, want)
    return g


# ------------------------------------------------- draw_normals<NA> layout, single-group kernel
@pytest.mark.parametrize("model,K,H,f64,nb_iters", [
    pytest.param("drone", 77, 20, None, (5, 1), id="drone-K77-H20-DRONE_3_NCH1_L32_ONEG-nb5x1"),
    pytest.param("arm", 77, 32, False, (5, 1), id="arm-f32-K77-H32-ARM_7_NCH1_L32_F32_ONEG-nb5x1"),
    pytest.param("arm", 77, 32, True, (5, 1), id="arm-f64-K77-H32-ARM_7_NCH1_L32_F64_ONEG-C3-nb5x1"),
    pytest.param("arm", 77, 48, True, (10, 1), id="arm-f64-K77-H48-ARM_7_NCH1_L64_F64_ONEG-nb10x1"),
    pytest.param("wholebody", 77, 64, None, (10, 1), id="wb-K77-H64-WB_10_NCH1_L64_ONEG-nb10x1"),
    pytest.param("wholebody", 77, 16, None, (5, 1), id="wb-K77-H16-WB_10_NCH1_L32_ONEG-sub-nb5x1"),
    pytest.param("quadrotor", 100, 32, None, (7, 1), id="quad-K100-H32-quad_NWD1-nb7"),
])
def test_single_group_kernels_draw_the_specified_stream(model, K, H, f64, nb_iters):
    """One Philox4x32 call (arm), 4x32 + 2x32 (whole-body), one 2x32 (drone, quadrotor); a partial
    last wave and block (K = 77: 5 rollouts in the last 16-rollout block at L = 32; K = 100: 4 in the
    quadrotor's last 16)."""
    _geom(model, K, H, nb_iters)
    kw = {} if f64 is None else {"state_f64": f64}
    e = _engine(model, K, H, **kw)
    _hip_step(e)
    _check(e, model, 0)
    e.close()


# ----------------------------------------------------------------------- t = t0 + 64 c (H > 64)
@pytest.mark.parametrize("model,H,nch", [
    pytest.param("arm", 100, 2, id="arm-H100-ARM_7_NCH2_L64-nb5x1"),
    pytest.param("arm", 200, 4, id="arm-H200-ARM_7_NCH4_L64-nb5x1"),
    pytest.param("drone", 256, 4, id="drone-H256-DRONE_3_NCH4_L64-nb5x1"),
    pytest.param("wholebody", 128, 2, id="wb-H128-WB_10_NCH2_L64-nb5x1"),
])
def test_horizon_chunks_draw_their_own_steps(model, H, nch):
    """K = 40, 8 rollouts per block, 5 blocks of one group each (NCH > 1 has no single-group
    instantiation: the looping kernel at iters = 1); chunk c draws t = t0 + 64 c."""
    g = _geom(model, 40, H, (5, 1))
    assert g["nch"] == nch and g["L"] == 64
    e = _engine(model, 40, H)
    _hip_step(e)
    _check(e, model, 0)
    e.close()


# ---------------------------------------------------------------------------- looping kernel
@pytest.mark.parametrize("model,H,bt,nbv,nb_iters", [
    pytest.param("wholebody", 64, 128, 3, (3, 13), id="wb-H64-bt128-WB_10_NCH1_L64_loop-nb3x13"),
    pytest.param("arm", 32, 128, 3, (3, 7), id="arm-H32-bt128-ARM_7_NCH1_L32_loop-R2-nb3x7"),
    pytest.param("drone", 20, 128, 3, (3, 7), id="drone-H20-bt128-DRONE_3_NCH1_L32_loop-nb3x7"),
    pytest.param("wholebody", 64, 64, 1, (1, 77), id="wb-H64-bt64-WB_10_NCH1_L64_loop-nb1x77"),
    pytest.param("arm", 32, 64, 1, (1, 39), id="arm-H32-bt64-ARM_7_NCH1_L32_loop-nb1x39"),
    pytest.param("drone", 20, 64, 1, (1, 39), id="drone-H20-bt64-DRONE_3_NCH1_L32_loop-nb1x39"),
])
def test_looping_kernel_draws_every_group(model, H, bt, nbv, nb_iters):
    """K = 77: groups it > 0 are drawn inside the loop with g = blockIdx.x + it * nb (group 0's
    normals come from the prologue); the last group's padding rollouts (k >= K) store nothing."""
    _geom(model, 77, H, nb_iters, block_threads=bt, blocks_per_vehicle=nbv)
    e = _engine(model, 77, H, block_threads=bt, blocks_per_vehicle=nbv)
    _hip_step(e)
    _check(e, model, 0)
    e.close()


def test_quadrotor_four_wave_blocks():
    """V = 2, K = 8200, H = 16: (K + 15) / 16 * V = 1026 > 1024 blocks -> k_rollout_quad<NWD4>, 64
    rollouts per block, 129 blocks per vehicle (the last with 8 rollouts)."""
    g = _geom("quadrotor", 8200, 16, (129, 4), V=2)
    assert g["iters"] == 4
    e = _engine("quadrotor", 8200, 16, V=2)
    _hip_step(e)
    _check(e, "quadrotor", 0)
    e.close()


# ------------------------------------------------------------------------------------- vkey
@pytest.mark.parametrize("model,K,H,offset", [
    pytest.param("wholebody", 40, 64, 0, id="wb-V3-off0-WB_10_NCH1_L64_Vgt1_ONEG-nb5x1"),
    pytest.param("wholebody", 40, 64, 300, id="wb-V3-off300-WB_10_NCH1_L64_Vgt1_ONEG-nb5x1"),
    pytest.param("wholebody", 40, 64, 32765, id="wb-V3-off32765-WB_10_NCH1_L64_Vgt1_ONEG-nb5x1"),
    pytest.param("arm", 40, 32, 0, id="arm-V3-off0-ARM_7_NCH1_L32_Vgt1_ONEG-nb3x1"),
    pytest.param("arm", 40, 32, 300, id="arm-V3-off300-ARM_7_NCH1_L32_Vgt1_ONEG-nb3x1"),
    pytest.param("arm", 40, 32, 32765, id="arm-V3-off32765-ARM_7_NCH1_L32_Vgt1_ONEG-nb3x1"),
    pytest.param("drone", 40, 20, 300, id="drone-V3-off300-DRONE_3_NCH1_L32_Vgt1_ONEG-nb3x1"),
    pytest.param("quadrotor", 40, 32, 300, id="quad-V3-off300-quad_Vgt1_NWD1-nb3"),
])
def test_vehicle_key_is_the_fleet_wide_index(model, K, H, offset):
    """V = 3 (vehicle constants from LDS / vc[v]), vkey = blockIdx.y + vehicle_offset; an offset
    >= 256 reaches the step bits of the Philox2x32 counter word ((veh << 8 | t) ^ (step << 16)),
    32765 + 2 = 32767 is the largest fleet-wide index."""
    _geom(model, K, H, (5, 1) if model == "wholebody" else (3, 1), V=3)
    e = _engine(model, K, H, V=3, vehicle_offset=offset)
    _hip_step(e)
    eps = _check(e, model, 0, vehicle_offset=offset)
    assert not np.array_equal(eps[0], eps[1]) and not np.array_equal(eps[1], eps[2])
    e.close()


# --------------------------------------------------------------------- extended (XC) kernels
@pytest.mark.parametrize("model,K,H,V,full,terms", [
    pytest.param("wholebody", 77, 64, 1, True, 0, id="wb-fullSigma-V1-WB_10_NCH1_L64_XC_loop-nb10x1"),
    pytest.param("wholebody", 77, 64, 3, True, 0, id="wb-fullSigma-V3-WB_10_NCH1_L64_Vgt1_XC_loop-nb10x1"),
    pytest.param("arm", 77, 32, 1, True, 0, id="arm-fullSigma-ARM_7_NCH1_L32_XC_loop-nb5x1"),
    pytest.param("arm", 77, 32, 1, False, ("covar", "center", "action"),
                 id="arm-costterms-diagSigma-ARM_7_NCH1_L32_XC_loop-nb5x1"),
])
def test_extended_kernels_draw_the_specified_stream(model, K, H, V, full, terms):
    """The XC instantiation (no single-group variant: the looping kernel at iters = 1): the full
    z Sigma product in the row-vector convention (a Sigma that is not symmetric), and the diagonal
    path inside the extended kernel (extra cost terms)."""
    _geom(model, K, H, (10, 1) if model == "wholebody" else (5, 1), V=V)
    sigma = _full_sigma(model) if full else SIGMA[model]
    e = _engine(model, K, H, V=V, sigma=sigma, cost_terms=terms)
    _hip_step(e)
    _check(e, model, 0, sigma=sigma)
    e.close()


# --------------------------------------------------------------------------------- seed halves
@pytest.mark.parametrize("model,K,H", [("drone", 77, 20), ("arm", 77, 32), ("wholebody", 77, 64),
                                       ("quadrotor", 100, 32)])
def test_both_seed_halves_key_the_stream(model, K, H):
    """seed = 2^40 + 7 (low and high key words non-zero), and a seed that differs only in the high
    half: each on its own stream, the two different."""
    got = []
    for seed in (2**40 + 7, 2**41 + 7):
        e = _engine(model, K, H, seed=seed)
        _hip_step(e)
        got.append(_check(e, model, 0, seed=seed))
        e.close()
    assert not np.array_equal(got[0], got[1]), "the high seed half must change the noise"
    assert float(np.mean(got[0] == got[1])) < 1e-3


# ------------------------------------------------------------------------- k_off (shard offsets)
@pytest.mark.parametrize("model,K,H,rank,count", [
    pytest.param("arm", 40, 32, 1, 2, id="arm-K40-rank1of2-k_off40"),
    pytest.param("arm", 40, 32, 7, 8, id="arm-K40-rank7of8-k_off280"),
    pytest.param("wholebody", 264, 64, 248, 249, id="wb-K264-rank248of249-k-crosses-2pow16"),
    pytest.param("drone", 4096, 20, 4096, 4097, id="drone-K4096-rank4096of4097-k_off2pow24"),
    pytest.param("drone", 65536, 20, 32767, 32769, id="drone-K65536-rank32767of32769-k-below-2pow31"),
    pytest.param("drone", 65536, 20, 32768, 32769, id="drone-K65536-rank32768of32769-k_off2pow31"),
    pytest.param("drone", 65536, 20, 65535, 65536, id="drone-K65536-rank65535of65536-k-ends-at-2pow32-1"),
])
def test_shard_offset_enters_the_sample_counter(model, K, H, rank, count):
    """A shard's rollout alone (its exchange slot in a zeroed buffer; no finalize): sample k of
    shard r draws with k_global = r * K + k as one 32-bit word.  Geometries: arm K=40 H=32 nb3x1,
    whole-body K=264 H=64 nb33x1, drone K=4096 H=20 nb256x1 (single-group kernels), drone K=65536
    H=20 nb1024x4 (looping kernel)."""
    want = {40: (3, 1), 264: (33, 1), 4096: (256, 1), 65536: (1024, 4)}[K]
    _geom(model, K, H, want)
    e = _engine(model, K, H, shard_rank=rank, shard_count=count)
    buf = torch.zeros(count * e.exchange_slot_floats(), device="cuda")
    e.bind_exchange(buf.data_ptr())
    e.rollout()
    e.synchronize()
    _check(e, model, 0, k0=rank * K)
    e.close()
    del buf


# ------------------------------------------------------------------ step counter, HIP launches
@pytest.mark.parametrize("model,K,H", [("arm", 77, 32), ("quadrotor", 100, 32)])
def test_step_counter_hip_launch_path(model, K, H):
    """rollout() + finalize() through HIP launches (the step word is the host's count, passed as
    the kernel argument): steps 0, 1, 2 on a fresh engine, then 0xFFFFFFFE, 0xFFFFFFFF and 0 across
    the 32-bit wrap."""
    e = _engine(model, K, H)
    for start in (0, 0xFFFFFFFE):
        if start:
            e.set_step_counter(start)
        for i in range(3):
            step = (start + i) & 0xFFFFFFFF
            assert e.get_step_counter() == step
            e.rollout()
            e.finalize()
            e.synchronize()
            _check(e, model, step, what=f"HIP launch {i} from {start:#x}:")
            assert e.get_step_counter() == (step + 1) & 0xFFFFFFFF
    e.close()


# ---------------------------------------------------------------- step counter, native dispatch
@pytest.mark.parametrize("model,K,H,kw", [
    pytest.param("arm", 77, 32, {"state_f64": True}, id="arm-f64-K77-H32"),
    pytest.param("wholebody", 77, 64, {}, id="wb-K77-H64"),
    pytest.param("quadrotor", 100, 32, {}, id="quad-K100-H32"),
])
def test_step_counter_native_dispatch_path(model, K, H, kw):
    """Native batches and control calls (AQL packets): the kernel takes the step as
    step_arg + (dispatch id >> 1).  The host's count (get_step_counter) and the device's
    arithmetic (the stored noise) are independent; both must follow the specification through
    batches, calls, a counter set by the caller and the 32-bit wrap."""
    e = _engine(model, K, H, **kw)

    def expect(next_step, what):
        assert e.get_step_counter() == next_step & 0xFFFFFFFF, (what, e.get_step_counter(), next_step)
        _check(e, model, (next_step - 1) & 0xFFFFFFFF, what=what)

    e.run_steps(5)
    e.synchronize()
    assert e.dispatch_info().startswith("aql;"), e.dispatch_info()
    expect(5, "run_steps(5):")
    e.step()
    assert "calls: aql" in e.dispatch_info(), e.dispatch_info()
    expect(6, "step() after the batch:")
    e.step()
    expect(7, "second step():")
    e.run_steps(3)
    e.synchronize()
    expect(10, "run_steps(3):")
    e.step()
    expect(11, "step() after the second batch:")
    e.set_step_counter(0xFFFFFFFE)
    assert e.get_step_counter() == 0xFFFFFFFE
    e.run_steps(3)
    e.synchronize()
    expect(1, "run_steps(3) across the wrap:")       # steps 0xFFFFFFFE, 0xFFFFFFFF, 0
    e.step()
    expect(2, "step() after the wrap:")
    assert e.dispatch_info().startswith("aql;") and "calls: aql" in e.dispatch_info(), e.dispatch_info()
    e.close()
