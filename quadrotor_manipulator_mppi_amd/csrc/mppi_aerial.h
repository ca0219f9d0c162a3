// mppi_aerial.h -- what the aerial manipulator's rollout (mppi_rollout_aerial.hip) and its plan kernel
// (mppi_plan.hip k_plan_aerial) share beyond the quadrotor step (mppi_quad_step.h) and the FK helpers
// (mppi_fk.h): the joints' double integrator of one rollout with lane = horizon step, the Kinova chain in
// the base frame, and the composition of that chain with the base pose of the row.
//
//   EE(k,t) = [Rz(yaw) Ry(pitch) Rx(roll) | p](k,t) * M_fixed * chain(q(k,t))
//
// (rotation convention: drone.py:126-154 = transformation_matrix.py:148-187).  The coupling is kinematic
// only: the base steps by the QUADROTOR recurrence under mppi_config.quad_mass / quad_inertia as the user
// sets them for the loaded vehicle, and arm motion does not react on the base.
#pragma once
#include "mppi_fk.h"
#include "mppi_integrator.h"

namespace {

// The chain's run-time constants: the translations of the seven joint origins (the Kinova fast path's
// rotations are compile-time signed permutations, mppi_dev.h kKinova), wave-uniform.
struct AerialChain { float o[kAerialNq][3]; };
__device__ __forceinline__ void aerial_chain_load(AerialChain& c, const JointDev* __restrict__ joints, const int j0) {
#pragma unroll
    for (int j = 0; j < kAerialNq; ++j) {
        c.o[j][0] = uniform_f32(joints[j0 + j].O[3]);
        c.o[j][1] = uniform_f32(joints[j0 + j].O[7]);
        c.o[j][2] = uniform_f32(joints[j0 + j].O[11]);
    }
}

// Joint angles q[j](t) of one rollout, lane = t: the double integrator of standard_normal_noise.py:32-50
// on the joint accelerations acc[j] (0 in the lanes past H), as k_rollout's scan form integrates the
// whole-body model's joints -- two fp32 DPP scans over the 64 lanes, the measured angle added last.
__device__ __forceinline__ void aerial_joints(const float (&acc)[kAerialNq], const int lane, const float dt, const float dt2h,
                                              const float* pos0f, const float* vel0f, float (&q)[kAerialNq]) {
#pragma clang fp contract(off)
    float c1[kAerialNq], c2[kAerialNq];
#pragma unroll
    for (int a = 0; a < kAerialNq; ++a) c1[a] = acc[a] * dt;
    seg_scan_f32_multi<64, kAerialNq>(c1);
#pragma unroll
    for (int a = 0; a < kAerialNq; ++a) {
        const float v0 = uniform_f32(vel0f[a]);
        const float h2 = acc[a] * dt2h;
        const float velf = c1[a] + v0;
        float prev = dpp_f32<0x138, 0xF>(velf);     // wave_shr:1
        if (lane == 0) prev = v0;
        c2[a] = prev * dt + h2;
    }
    seg_scan_f32_multi<64, kAerialNq>(c2);
#pragma unroll
    for (int a = 0; a < kAerialNq; ++a) q[a] = c2[a] + uniform_f32(pos0f[a]);
}

// T = M_fixed * chain(q): the arm in the base frame (the Kinova fast path of the ARM kernels).
template <int J>
__device__ __forceinline__ void aerial_joint(Mat34& T, const AerialChain& c, const float q) {
    const float O[12] = {0.0f, 0.0f, 0.0f, c.o[J][0], 0.0f, 0.0f, 0.0f, c.o[J][1], 0.0f, 0.0f, 0.0f, c.o[J][2]};
    kin_joint<J>(T, O, q);
}
__device__ __forceinline__ void aerial_arm_fk(Mat34& T, const float* base12, const AerialChain& c, const float (&q)[kAerialNq]) {
#pragma unroll
    for (int i = 0; i < 12; ++i) T.m[i] = uniform_f32(base12[i]);
    aerial_joint<0>(T, c, q[0]);
    aerial_joint<1>(T, c, q[1]);
    aerial_joint<2>(T, c, q[2]);
    aerial_joint<3>(T, c, q[3]);
    aerial_joint<4>(T, c, q[4]);
    aerial_joint<5>(T, c, q[5]);
    aerial_joint<6>(T, c, q[6]);
}

// E = [Rz(e2) Ry(e1) Rx(e0) | p] * T, with the three sin / cos pairs formed here (sincos_joint, fp32 angle).
__device__ __forceinline__ void aerial_compose(Mat34& E, const Mat34& T, const float (&p)[3], const float (&e)[3]) {
    float sr, cr, sp, cp, sy, cy;
    sincos_joint(e[0], sr, cr);
    sincos_joint(e[1], sp, cp);
    sincos_joint(e[2], sy, cy);
    const float R[9] = {cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
                        sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                        -sp,     cp * sr,                cp * cr};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float r0 = R[3 * i], r1 = R[3 * i + 1], r2 = R[3 * i + 2];
#pragma unroll
        for (int j = 0; j < 4; ++j) E.m[4 * i + j] = r0 * T.m[j] + r1 * T.m[4 + j] + r2 * T.m[8 + j];
        E.m[4 * i + 3] += p[i];
    }
}

}  // namespace
