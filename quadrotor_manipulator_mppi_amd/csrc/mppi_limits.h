// mppi_limits.h -- the rotor limits of a bounded engine (mppi_create_limits): bounds lo[4] <= hi[4] on action
// dims 0..3 of the QUADROTOR and AERIAL models (thrust, tau_x, tau_y, tau_z) and the arithmetic of one clamped
// control.  Shared by the bounded rollouts (mppi_rollout_quad.hip; mppi_rollout_aerial.h, built in mppi_limits.hip),
// the bounded plan kernels (mppi_plan_air.h, likewise) and the host replay (mppi_limits_apply), so it compiles as
// HIP and as plain C++.
//
// The device buffer: kLimitsW floats, lo[0..3] then hi[0..3]; -inf / +inf leave a side open.
//
// For u = u_prev[t][a] and the draw eps, every operation one fp32 operation, none fused with a neighbour:
//     a0   = fl(u + eps)
//     v'   = min(max(a0, lo), hi)
//     eps' = (a0 == v') ? eps : fl(v' - u)                          the effective noise
//     c    = (a0 == v') ? a0  : min(max(fl(u + eps'), lo), hi)      the control the dynamics integrate
// An unsaturated draw is untouched bit for bit (eps' = eps, c = a0).  For a saturated one fl(u + eps') can miss
// the bound by an ulp, so c takes the clamp once more: c lies in [lo, hi] always.  Since the clamp is the
// identity on an unsaturated a0, c = min(max(fl(u + eps'), lo), hi) in both cases: what the dynamics wave
// applies to the sum of the two LDS operands it already reads (limits_clamp).
#pragma once
#include <math.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define MPPI_LIM_FN __host__ __device__ __forceinline__
#else
#define MPPI_LIM_FN inline
#endif

namespace mppi {

constexpr int kLimitsN = 4;              // the bounded dims: thrust, tau_x, tau_y, tau_z
constexpr int kLimitsW = 2 * kLimitsN;   // lo[4], hi[4]

// min(max(x, lo), hi) for lo <= hi, neither NaN (one v_med3_f32 on the device); a NaN x comes out as lo
MPPI_LIM_FN float limits_clamp(float x, float lo, float hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fmed3f(x, lo, hi);
#else
    return fminf(fmaxf(x, lo), hi);
#endif
}

// The four lines above: the effective noise into eps_eff, the control into ctl.
MPPI_LIM_FN void limits_apply(float u, float eps, float lo, float hi, float& eps_eff, float& ctl) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float a0 = u + eps;
    const float v = limits_clamp(a0, lo, hi);
    const bool same = a0 == v;
    const float e = same ? eps : v - u;
    eps_eff = e;
    ctl = same ? a0 : limits_clamp(u + e, lo, hi);
}

// the control of an effective noise (limits_apply's last line on what it left in the noise tile)
MPPI_LIM_FN float limits_control(float u, float eps_eff, float lo, float hi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return limits_clamp(u + eps_eff, lo, hi);
}

}  // namespace mppi
