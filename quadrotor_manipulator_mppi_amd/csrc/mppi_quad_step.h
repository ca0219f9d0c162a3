// mppi_quad_step.h -- one step of the 6-DoF quadrotor dynamics for one axis lane, shared by
// k_rollout_quad (mppi_rollout_quad.hip) and the plan kernel (mppi_plan.hip).  Four lanes per
// rollout: lane j < 3 owns axis j (position, velocity, Euler angle j, body rate j), lane 3 follows
// axis 2; quad_perm DPP broadcasts hand each lane the other axes' values.
#pragma once
#include "mppi_fk.h"   // sincos_joint

namespace {

// lane SRC of every 4-lane group, to all four (DPP quad_perm [SRC, SRC, SRC, SRC])
template <int SRC>
__device__ __forceinline__ float qbc(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), SRC * 0x55, 0xF, 0xF, false));
}
// per-lane select by a wave-uniform lane mask (m-lanes take b): a ternary on the lane's
// axis index compiled to divergent branches around each formula
__device__ __forceinline__ float lane_sel(float a, float b, uint64_t m) {
    float r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(m));
    return r;
}
constexpr uint64_t kM0 = 0x1111111111111111ull, kM1 = 0x2222222222222222ull;   // lanes of axis 0 / 1
constexpr uint64_t kM2 = 0xCCCCCCCCCCCCCCCCull;                                  // axis 2 (and lane 3)

// Step t of this lane's axis under thrust thr and this axis' torque tau (v = u + eps,
// drone_mppi.py:144): (pj, ej, vj, wj) = position, Euler angle, world velocity, body rate.
// Constants of the lane: gj = g's component, ij = 1 / I_jj, a0 = J's column 0 entry (1 on axis 0),
// (ox0, oy0, oz0) = the measured body rates (FIRST).  LIT: mppi_config.quad_literal_jinv.
template <bool LIT, bool FIRST>
__device__ __forceinline__ void quad_axis_step(float& pj, float& ej, float& vj, float& wj, const float thr,
                                               const float tau, const float dt, const float im, const float kd,
                                               const float gj, const float ij, const float a0, const float ox0,
                                               const float oy0, const float oz0) {
    // body rate: omega_t = omega_{t-1} + dt * (I^-1 tau_t) (drone_mppi.py:65,72)
    wj = wj + dt * (ij * tau);
    // attitude of the previous step: sin/cos of this lane's angle, the others by DPP
    float sj, cj;
    sincos_joint(ej, sj, cj);
    const float sr = qbc<0>(sj), cr = qbc<0>(cj), sp = qbc<1>(sj), cp = qbc<1>(cj);
    const float sy = qbc<2>(sj), cy = qbc<2>(cj);
    // step 0 integrates the measured rates (drone_mppi.py:69), later steps omega_t
    const float ox = FIRST ? ox0 : qbc<0>(wj), oy = FIRST ? oy0 : qbc<1>(wj), oz = FIRST ? oz0 : qbc<2>(wj);
    // Euler rates of this lane's axis: J(rpy) omega (drone.py:114-124), or inv(J) omega
    // for t >= 1 in the literal mode (drone_mppi.py:73-75)
    float dj;
    if (LIT && !FIRST) {
        const float d0 = ox - sp * oz;
        const float d1 = cr * oy + (sr * cp) * oz;
        const float d2 = (cr * cp) * oz - sr * oy;
        dj = lane_sel(lane_sel(d2, d1, kM1), d0, kM0);
    } else {
        // row j of J as (A_j, B_j, C_j): (1, s_r t, c_r t), (0, c_r, -s_r), (0, s_r/c_p, c_r/c_p)
        // with t = s_p / c_p: B and C of rows 0 and 2 are (s_r, c_r) times f = (s_p or 1) / c_p
        const float ic = __builtin_amdgcn_rcpf(cp);   // one v_rcp_f32 (<= 1 ulp) for tan and 1/cos
        const float f = ic * lane_sel(1.0f, sp, kM0);
        const float Bj = lane_sel(sr * f, cr, kM1), Cj = lane_sel(cr * f, -sr, kM1);
        dj = fmaf(Cj, oz, fmaf(Bj, oy, a0 * ox));
    }
    float en = ej + dt * dj;
    if (!FIRST) en = en - 6.283185307179586f * __builtin_rintf(en * 0.15915494309189535f);   // atan2(sin, cos) (:76)
    // translational: v_t = v_{t-1} + dt (g + (R f - kd v_{t-1}) / m), f = (0, 0, thrust),
    // R(rpy_{t-1}) (drone.py:126-154); p_t = p_{t-1} + dt v
    // column 2 of R: (c_y s_p c_r + s_y s_r, s_y s_p c_r - c_y s_r, c_p c_r) as
    // P_j (s_p c_r) + Q_j s_r for rows 0, 1
    const float Pj = lane_sel(sy, cy, kM0), Qj = lane_sel(-cy, sy, kM0);
    const float rj = lane_sel(fmaf(Pj, sp * cr, Qj * sr), cp * cr, kM2);
    const float aj = gj + im * (rj * thr - kd * vj);
    const float nv = vj + dt * aj;
    pj = pj + dt * (FIRST ? vj : nv);   // step 0 moves with the measured velocity (:70)
    vj = nv;
    ej = en;
}

}  // namespace
