"""The device noise stream as DESIGN.md §4 specifies it, and the checker that holds stored
rollout noise to it (shared by tests/test_gpu_noise_stream.py and tests/test_noise_stream_cpu.py).

Specification: eps[k, t, :] = z[k, t, :] Sigma (row vector), z = draw_normals(k_global, t,
fleet-wide vehicle, control step, seed), restated in float64 by ``O.philox_normals``.

Tolerance, from the project's own bar on the hardware Box-Muller
(``test_gpu_parity.test_device_philox_matches_restatement``: rtol 2e-5, atol 2e-5 on z, the same
inlined ``draw_normals`` the rollout kernels call): every normal may be off by
2e-5 + 2e-5 |z_a|, and eps_b = sum_a z_a Sigma_ab carries that through |Sigma_ab|:

    |eps_b - (z Sigma)_b| <= sum_a (2e-5 + 2e-5 |z_a|) |Sigma_ab|

which for a diagonal Sigma is (2e-5 + 2e-5 |z_a|) sigma_a.  The fp32 product and sum add a few
1e-7 relative, far inside it.  A wrong counter word gives unrelated normals (error O(sigma)).
"""
import numpy as np

from oracle import mppi_oracle as O

Z_RTOL = 2e-5
Z_ATOL = 2e-5
MODEL_A = {"drone": 3, "quadrotor": 4, "arm": 7, "wholebody": 10}


def sigma_matrix(sigma, A):
    """Sigma as the (A, A) float64 image of the float32 matrix the engine holds."""
    s = np.asarray(sigma, np.float32)
    if s.ndim == 1:
        s = np.diag(s)
    assert s.shape == (A, A), s.shape
    return s.astype(np.float64)


def reference_normals(seed, step, vehicle, k_global, H, A):
    _, z = O.philox_normals(int(seed), int(step) & 0xFFFFFFFF, int(vehicle), np.asarray(k_global, np.int64), H, A)
    return z.astype(np.float64)


def expected_eps(seed, step, vehicle, k_global, H, A, sigma):
    """(len(k_global), H, A) float64: z_ref @ Sigma (= z_ref * diag for a diagonal Sigma, exactly:
    the other terms are zeros)."""
    return reference_normals(seed, step, vehicle, k_global, H, A) @ sigma_matrix(sigma, A)


def stream_tolerance(z_ref, sigma):
    A = z_ref.shape[-1]
    return (Z_ATOL + Z_RTOL * np.abs(z_ref)) @ np.abs(sigma_matrix(sigma, A))


def assert_stream(eps_gpu, seed, step, vehicle, k_global, H, A, sigma, what=""):
    """Every element of ``eps_gpu`` (len(k_global), H, A) against the specification."""
    eps = np.asarray(eps_gpu, np.float64)
    z = reference_normals(seed, step, vehicle, k_global, H, A)
    want = z @ sigma_matrix(sigma, A)
    assert eps.shape == want.shape, (what, eps.shape, want.shape)
    assert np.isfinite(eps).all(), f"{what}: non-finite noise"
    err = np.abs(eps - want)
    bad = err > stream_tolerance(z, sigma)
    if bad.any():
        k, t, a = np.argwhere(bad)[0]
        raise AssertionError(
            f"{what}: {int(bad.sum())} / {bad.size} elements off the Philox stream "
            f"(seed {seed:#x}, step {int(step) & 0xFFFFFFFF:#x}, vehicle {vehicle}); first at local k={k} "
            f"(global {int(np.asarray(k_global)[k])}), t={t}, a={a}: got {eps[k, t, a]:.7g}, want {want[k, t, a]:.7g}; "
            f"rollouts with an element off: {int(bad.any(axis=(1, 2)).sum())} / {bad.shape[0]}, "
            f"steps t with one: {np.flatnonzero(bad.any(axis=(0, 2)))[:8].tolist()}")


def geometry(model, K, H, V=1, block_threads=0, blocks_per_vehicle=0):
    """The rollout launch geometry mppi_create derives (csrc/mppi_layout.cpp, geometry), restated
    (tests/test_capi_layout_cpu.py holds it to the library over a sweep):
    lane segment L, 64-step chunks nch, rollouts per wave R, waves per block nw, rollout groups,
    blocks per vehicle nb and groups per block iters (iters == 1 with nch == 1 and the common
    kernel: the single-group instantiation; else the looping one)."""
    L = 64 if H > 32 else 32
    nch = (H + 63) // 64
    assert nch in (1, 2, 4), H
    if model == "quadrotor":
        iters = 1 if (K + 15) // 16 * V <= 1024 else 4
        return dict(L=L, nch=nch, R=16, nw=iters, groups=None, nb=(K + 16 * iters - 1) // (16 * iters), iters=iters)
    R = 64 // L
    nw = (block_threads or 512) // 64
    groups = (K + nw * R - 1) // (nw * R)
    nb = blocks_per_vehicle
    if nb <= 0:
        nb = groups if groups * V <= 512 else min(max(1, groups // 2), max(1, 1024 // V))
    nb = min(nb, groups)
    iters = (groups + nb - 1) // nb
    iters = min(iters, max(1, 4096 // ((nw * R + 3) & ~3)))
    nb = (groups + iters - 1) // iters
    return dict(L=L, nch=nch, R=R, nw=nw, groups=groups, nb=nb, iters=iters)
