// mppi_plan_air.h -- the plan kernels of the two airframe models (QUADROTOR: k_plan_quad; AERIAL: k_plan_aerial) and
// their bounded forms (k_plan_quad_b, k_plan_aerial_b), shared by mppi_plan.hip (the plain kernels' unit) and
// mppi_limits.hip (the bounded ones'): each unit instantiates its own kernels.
#pragma once
#include <type_traits>

#include "mppi_fk.h"
#include "mppi_integrator.h"   // seg_scan_f32_multi
#include "mppi_quad_step.h"
#include "mppi_aerial.h"
#include "mppi_limits.h"

// QUADROTOR: lanes 0..3 of the block's one wave are the vehicle's axis lanes (mppi_quad_step.h);
// the other lanes only help stage u_prev.
// LIM (k_plan_quad_b, k_plan_aerial_b; an engine of mppi_create_limits): the rows' rotor dims are staged clamped
// (mppi_limits.h limits_apply with eps = 0): the plan of the clamped warm start.
__device__ __forceinline__ float plan_limit(const float u, const int a, const float* __restrict__ lim) {
    float e, c;
    limits_apply(u, 0.0f, lim[a], lim[kLimitsN + a], e, c);
    return c;
}

template <bool LIT, bool LIM>
__device__ __forceinline__ void plan_quad_body(const float* __restrict__ u_prev, const PlanParams& pp, const DevParams& pk,
                                               const float* __restrict__ lim) {
    constexpr int kQA = 4;
    __shared__ float u_t[(64 + 1) * kQA];   // (a spare row: the step loads one row ahead)
    const DevParams& p = pk;
    const int v = blockIdx.x, lane = threadIdx.x, H = p.H;
    const float* up = u_prev + (size_t)v * H * kQA;
    for (int i = lane; i < (64 + 1) * kQA; i += 64) {
        float x = (i < H * kQA) ? ld_dev(up + i) : 0.0f;
        if constexpr (LIM) x = (i < H * kQA) ? plan_limit(x, i & 3, lim) : x;
        u_t[i] = x;
    }
    lds_barrier();
    if (lane >= 4) return;
    const VehicleConst& vc = pp.vc[v];
    const int j = lane & 3, jj = j < 3 ? j : 2;
    const float dt = p.dt, im = p.q_inv_m, kd = p.q_kd;
    const float gj = (j >= 2) ? -p.q_g : 0.0f;      // g = (0, 0, -q_g)
    const float ij = p.q_iinv[jj], tg = vc.tpos[jj];
    const float* const trow = pp.ttab ? pp.ttab + (size_t)v * H * 12 + jj : nullptr;   // a tracking engine's rows
    float pj = vc.pos0f[jj], ej = vc.pos0f[3 + jj], vj = vc.vel0f[jj], wj = vc.vel0f[3 + jj];
    const float ox0 = vc.vel0f[3], oy0 = vc.vel0f[4], oz0 = vc.vel0f[5];
    const float a0 = (j == 0) ? 1.0f : 0.0f;
    float* const planes = pp.traj + (size_t)v * p.C * H;
    float S = 0.0f;
    auto step = [&](const int t, auto first_c) {
        constexpr bool FIRST = decltype(first_c)::value;
        const float thr = u_t[t * kQA], tau = u_t[t * kQA + 1 + jj];
        quad_axis_step<LIT, FIRST>(pj, ej, vj, wj, thr, tau, dt, im, kd, gj, ij, a0, ox0, oy0, oz0);
        if (j < 3) {
            planes[(size_t)j * H + t] = pj;
            planes[(size_t)(3 + j) * H + t] = ej;
        }
        // squared and L1 position error over the three axes (drone_mppi.py:87-107)
        const float dd = pj - (trow ? trow[(size_t)t * 12] : tg), d2 = dd * dd, d1 = fabsf(dd);
        const float x = qbc<0>(d2) + qbc<1>(d2) + qbc<2>(d2);
        const float e1 = qbc<0>(d1) + qbc<1>(d1) + qbc<2>(d1);
        const float c = ((t == H - 1) ? p.w_tp : p.w_sp) * x;
        S += c;
        if (j == 0) {
            pp.cost_t[(size_t)v * H + t] = c;
            pp.pos_err[(size_t)v * H + t] = e1;
        }
    };
    step(0, std::true_type{});
    for (int t = 1; t < H; ++t) step(t, std::false_type{});
    if (j == 0) pp.S[v] = S;
}

template <bool LIT>
__global__ void __launch_bounds__(64) k_plan_quad(const float* __restrict__ u_prev, const PlanParams pp,
                                                  const DevParams pk) {
    plan_quad_body<LIT, false>(u_prev, pp, pk, nullptr);
}
template <bool LIT>
__global__ void __launch_bounds__(64) k_plan_quad_b(const float* __restrict__ u_prev, const float* __restrict__ lim,
                                                    const PlanParams pp, const DevParams pk) {
    plan_quad_body<LIT, true>(u_prev, pp, pk, lim);
}

// AERIAL: one wave per vehicle.  Lanes 0..3 step the base through the quadrotor's step as k_plan_quad does and
// leave (p, rpy)(t) in LDS; then lane = t integrates the joints, runs the chain in the base frame, composes it
// with the base pose of its row and costs the end effector (mppi_aerial.h: the rollout kernel's own functions).
template <bool LIT, bool LIM>
__device__ __forceinline__ void plan_aerial_body(const float* __restrict__ u_prev, const JointDev* __restrict__ jtab,
                                                 const PlanParams& pp, const DevParams& pk, const float* __restrict__ lim) {
    constexpr int kA = kAerialA, kNQ = kAerialNq, kPW = kAerialPoseW;
    __shared__ float u_t[(64 + 1) * kA];   // (a spare row: the step loads one row ahead)
    __shared__ float pose[64 * kPW];
    const DevParams& p = pk;
    const int v = blockIdx.x, lane = threadIdx.x, H = p.H;
    const float* up = u_prev + (size_t)v * H * kA;
    for (int i = lane; i < (64 + 1) * kA; i += 64) {
        float x = (i < H * kA) ? ld_dev(up + i) : 0.0f;
        if constexpr (LIM) x = (i < H * kA && i % kA < kLimitsN) ? plan_limit(x, i % kA, lim) : x;
        u_t[i] = x;
    }
    lds_barrier();
    const VehicleConst& vc = pp.vc[v];
    if (lane < 4) {
        const int j = lane & 3, jj = j < 3 ? j : 2;
        const float dt = p.dt, im = p.q_inv_m, kd = p.q_kd;
        const float gj = (j >= 2) ? -p.q_g : 0.0f;      // g = (0, 0, -q_g)
        const float ij = p.q_iinv[jj];
        float pj = vc.pos0f[jj], ej = vc.pos0f[11 + jj], vj = vc.vel0f[jj], wj = vc.vel0f[11 + jj];
        const float ox0 = vc.vel0f[11], oy0 = vc.vel0f[12], oz0 = vc.vel0f[13];
        const float a0 = (j == 0) ? 1.0f : 0.0f;
        auto step = [&](const int t, auto first_c) {
            constexpr bool FIRST = decltype(first_c)::value;
            const float thr = u_t[t * kA], tau = u_t[t * kA + 1 + jj];
            quad_axis_step<LIT, FIRST>(pj, ej, vj, wj, thr, tau, dt, im, kd, gj, ij, a0, ox0, oy0, oz0);
            pose[t * kPW + jj] = pj;
            pose[t * kPW + 3 + jj] = ej;
        };
        step(0, std::true_type{});
        for (int t = 1; t < H; ++t) step(t, std::false_type{});
    }
    lds_barrier();
    const int t = lane;
    const bool val = t < H;
    const int tc = val ? t : H - 1;
    float acc[kNQ], q[kNQ];
#pragma unroll
    for (int a = 0; a < kNQ; ++a) acc[a] = val ? u_t[tc * kA + 4 + a] : 0.0f;
    aerial_joints(acc, lane, p.dt, 0.5f * p.dt2, vc.pos0f + 4, vc.vel0f + 4, q);
    AerialChain ch;
    aerial_chain_load(ch, jtab, p.j0);
    Mat34 T, E;
    aerial_arm_fk(T, vc.base, ch, q);
    const float pb[3] = {pose[tc * kPW], pose[tc * kPW + 1], pose[tc * kPW + 2]};
    const float eb[3] = {pose[tc * kPW + 3], pose[tc * kPW + 4], pose[tc * kPW + 5]};
    aerial_compose(E, T, pb, eb);
    const bool term = (t == H - 1);
    const float cost = pose_cost(E, vc, term ? p.w_tp : p.w_sp, term ? p.w_to : p.w_so);
    const float perr = fabsf(E.m[3] - vc.tpos[0]) + fabsf(E.m[7] - vc.tpos[1]) + fabsf(E.m[11] - vc.tpos[2]);
    if (val) {
        float* const planes = pp.traj + (size_t)v * p.C * H;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            planes[(size_t)a * H + t] = pb[a];
            planes[(size_t)(3 + a) * H + t] = eb[a];
        }
#pragma unroll
        for (int a = 0; a < kNQ; ++a) planes[(size_t)(6 + a) * H + t] = q[a];
#pragma unroll
        for (int i = 0; i < 12; ++i) planes[(size_t)(6 + kNQ + i) * H + t] = E.m[i];
        pp.cost_t[(size_t)v * H + t] = cost;
        pp.pos_err[(size_t)v * H + t] = perr;
    }
    const float S = wave_fold_all(val ? cost : 0.0f, OpAdd());
    if (lane == 0) pp.S[v] = S;
}

template <bool LIT>
__global__ void __launch_bounds__(64) k_plan_aerial(const float* __restrict__ u_prev, const JointDev* __restrict__ jtab,
                                                    const PlanParams pp, const DevParams pk) {
    plan_aerial_body<LIT, false>(u_prev, jtab, pp, pk, nullptr);
}
template <bool LIT>
__global__ void __launch_bounds__(64) k_plan_aerial_b(const float* __restrict__ u_prev, const JointDev* __restrict__ jtab,
                                                      const float* __restrict__ lim, const PlanParams pp, const DevParams pk) {
    plan_aerial_body<LIT, true>(u_prev, jtab, pp, pk, lim);
}

