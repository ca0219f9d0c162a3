"""CPU side of the noise-stream pin (tests/noise_stream.py, tests/test_gpu_noise_stream.py):

* the checker rejects each counter mistake the GPU cases are meant to catch (synthetic "GPU" noise
  made from the specification with one argument wrong);
* the float64 restatement stays finite and self-consistent at the extremes the GPU cases use
  (k up to 2^32 - 1, step 0xFFFFFFFF, vehicle 32767);
* mppi_create refuses shard layouts the 32-bit sample counter cannot address.
No GPU calls."""
import ctypes as C

import numpy as np
import pytest

from noise_stream import assert_stream, expected_eps, geometry, reference_normals, stream_tolerance
from oracle import mppi_oracle as O

SEED = 2**40 + 7
ARM_SIG = np.eye(7, dtype=np.float32) * 0.1
WB_SIG = np.diag([30.0] * 3 + [0.1] * 7).astype(np.float32)
WB_FULL = WB_SIG.copy()
WB_FULL[0, 1] = WB_FULL[1, 0] = 2.0
WB_FULL[4, 5] = WB_FULL[5, 4] = 0.02
WB_FULL[0, 2], WB_FULL[2, 0] = 1.0, -0.5      # not symmetric: z Sigma differs from Sigma z

K, H, STEP, VEH = 77, 32, 5, 2
KS = np.arange(K)


def _fake(**wrong):
    """The specification's noise as float32 (what a correct kernel stores), one argument replaced."""
    a = dict(seed=SEED, step=STEP, vehicle=VEH, k_global=KS, H=H, A=7, sigma=ARM_SIG)
    a.update(wrong)
    return expected_eps(**a).astype(np.float32)


def _check(eps, **over):
    a = dict(seed=SEED, step=STEP, vehicle=VEH, k_global=KS, H=H, A=7, sigma=ARM_SIG)
    a.update(over)
    assert_stream(eps, what="synthetic", **a)


def test_checker_accepts_the_specification():
    _check(_fake())
    # and the whole tolerance band of the hardware Box-Muller, not a hair more
    z = reference_normals(SEED, STEP, VEH, KS, H, 7)
    tol = stream_tolerance(z, ARM_SIG)
    want = expected_eps(SEED, STEP, VEH, KS, H, 7, ARM_SIG)
    _check(want + 0.99 * tol)
    with pytest.raises(AssertionError):
        _check(want + 1.5 * tol)
    one = want.copy()
    one[K - 1, H - 1, 6] += 1.5 * tol[K - 1, H - 1, 6]      # a single element: nothing is subsampled
    with pytest.raises(AssertionError):
        _check(one)
    with pytest.raises(AssertionError):
        _check(want[:, :, :6])                               # shape


# the looping launch of the GPU cases: block_threads=128, blocks_per_vehicle=3, arm K=77 H=32
_G = geometry("arm", K, H, block_threads=128, blocks_per_vehicle=3)
_PER_IT = _G["nb"] * _G["nw"] * _G["R"]      # rollouts one loop iteration of the whole grid covers


@pytest.mark.parametrize("name,wrong", [
    ("step + 1", dict(step=STEP + 1)),
    ("vehicle ^ 1", dict(vehicle=VEH ^ 1)),
    ("k shifted by one", dict(k_global=KS + 1)),
    ("k masked to 13 bits", dict(k_global=(KS + 8190) & 0x1FFF)),
    ("groups it > 0 redraw group 0 (the prologue's normals)", dict(k_global=KS % _PER_IT)),
    ("seed high half cleared", dict(seed=SEED & 0xFFFFFFFF)),
])
def test_checker_rejects_a_wrong_counter(name, wrong):
    over = {}
    if name.startswith("k masked"):      # the shard's samples straddle 2^13
        over = dict(k_global=KS + 8190)
    assert _G["iters"] == 7 and _PER_IT == 12
    with pytest.raises(AssertionError, match="off the Philox stream"):
        _check(_fake(**wrong), **over)


def test_checker_rejects_a_repeated_chunk():
    """t >= 64 drawn as t - 64 (the second 64-step chunk repeating the first)."""
    Hl = 100
    eps = _fake(H=Hl, k_global=KS[:8])
    _check(eps, H=Hl, k_global=KS[:8])
    eps[:, 64:] = eps[:, :Hl - 64]
    with pytest.raises(AssertionError, match="off the Philox stream"):
        _check(eps, H=Hl, k_global=KS[:8])


def test_checker_rejects_a_transposed_sigma():
    a = dict(seed=SEED, step=STEP, vehicle=VEH, k_global=KS[:16], H=16, A=10)
    good = expected_eps(sigma=WB_FULL, **a).astype(np.float32)
    assert_stream(good, sigma=WB_FULL, **a)
    with pytest.raises(AssertionError, match="off the Philox stream"):
        assert_stream(expected_eps(sigma=WB_FULL.T, **a).astype(np.float32), sigma=WB_FULL, **a)


def test_wrong_counters_leave_almost_nothing_within_tolerance():
    """The bar is far from marginal: under each wrong counter at most 0.1 % of the elements stay
    within the tolerance (unrelated normals; expected ~1e-4 of them by chance)."""
    z = reference_normals(SEED, STEP, VEH, KS, H, 7)
    want, tol = z @ ARM_SIG.astype(np.float64), stream_tolerance(z, ARM_SIG)
    for wrong in (dict(step=STEP + 1), dict(vehicle=VEH ^ 1), dict(k_global=KS + 1), dict(seed=SEED & 0xFFFFFFFF)):
        inside = np.abs(_fake(**wrong) - want) <= tol
        assert inside.mean() < 1e-3, (wrong, inside.mean())


@pytest.mark.parametrize("A", [3, 4, 7, 10])
def test_oracle_at_the_extremes(A):
    """k up to 2^32 - 1, step 0xFFFFFFFF, vehicle 32767: finite, within Box-Muller's range (the
    18-bit radius grid cuts the tail at 5.13 sigma), equal to the same draw taken one sample at a
    time, and distinct from the neighbouring counters (no word wraps into another)."""
    ks = np.array([0, 2**16 - 1, 2**16, 2**24, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1])
    step, veh, Hh = 0xFFFFFFFF, 32767, 8
    raw, z = O.philox_normals(SEED, step, veh, ks, Hh, A)
    assert z.shape == (len(ks), Hh, A) and np.isfinite(z).all() and np.abs(z).max() < 5.2
    for i, k in enumerate(ks):
        raw1, z1 = O.philox_normals(SEED, step, veh, np.array([k]), Hh, A)
        assert np.array_equal(raw1[0], raw[i]) and np.array_equal(z1[0], z[i])
    flat = raw.reshape(len(ks), -1)
    assert len({r.tobytes() for r in flat}) == len(ks), "samples must draw distinct words"
    for other in (dict(step=0), dict(step=0xFFFFFFFE), dict(veh=32766), dict(veh=0)):
        raw2, _ = O.philox_normals(SEED, other.get("step", step), other.get("veh", veh), ks, Hh, A)
        assert not (raw2 == raw).all(axis=-1).any(), other
    e = expected_eps(SEED, step, veh, ks, Hh, A, np.full(A, 0.5, np.float32))
    assert e.dtype == np.float64 and np.isfinite(e).all()
    # the step word is 32 bits: 2^32 + s is step s
    assert np.array_equal(expected_eps(SEED, 2**32 + 1, veh, ks, Hh, A, np.ones(A, np.float32)),
                          expected_eps(SEED, 1, veh, ks, Hh, A, np.ones(A, np.float32)))


def test_geometry_restatement_of_the_issue_cases():
    """The launch geometries the GPU cases name (csrc/mppi_engine.cpp, mppi_create)."""
    g = geometry("wholebody", 77, 64, block_threads=128, blocks_per_vehicle=3)
    assert (g["groups"], g["nb"], g["iters"]) == (39, 3, 13)
    g = geometry("arm", 77, 32, block_threads=128, blocks_per_vehicle=3)
    assert (g["R"], g["groups"], g["nb"], g["iters"]) == (2, 20, 3, 7)
    g = geometry("arm", 77, 32)
    assert (g["nb"], g["iters"]) == (5, 1)
    g = geometry("quadrotor", 8200, 16, V=2)
    assert (g["nb"], g["iters"]) == (129, 4)
    assert geometry("quadrotor", 100, 32)["iters"] == 1


def _create_status(**kw):
    from quadrotor_manipulator_mppi_amd import _capi as capi
    from quadrotor_manipulator_mppi_amd.engine import make_config
    L = capi.lib()
    cfg = make_config(store_trajectory=False, **kw)
    h = C.c_void_p()
    st = L.mppi_create(C.byref(cfg), C.byref(h))
    msg = L.mppi_last_error().decode(errors="replace") if st != capi.OK else ""
    if st == capi.OK:
        L.mppi_destroy(h)
    return st, msg


def test_shard_layout_beyond_the_32_bit_sample_counter_is_refused():
    """k_global = shard_rank * K + k is one 32-bit Philox counter word: shard_count * K > 2^32 is
    refused at create with MPPI_ERR_INVALID_ARG (a high shard would redraw shard 0's noise);
    exactly 2^32 samples are addressable and pass validation (without a GPU the create then fails
    later, on the device, with another status)."""
    from quadrotor_manipulator_mppi_amd import _capi as capi
    for kw in (dict(model="drone", n_samples=65536, n_horizon=20, shard_rank=65536, shard_count=65537),
               dict(model="drone", n_samples=65536, n_horizon=20, shard_rank=0, shard_count=65537),
               dict(model="drone", n_samples=2**30, n_horizon=20, shard_rank=4, shard_count=5)):
        st, msg = _create_status(**kw)
        assert st == capi.ERR_INVALID_ARG, (kw, st, msg)
        assert "32-bit sample counter" in msg and "2^32" in msg, msg
    st, msg = _create_status(model="drone", n_samples=65536, n_horizon=20, shard_rank=65535, shard_count=65536)
    assert "32-bit sample counter" not in msg, msg
    assert st != capi.ERR_INVALID_ARG, (st, msg)
