// mppi_fk.h -- forward kinematics and the pose cost of one (k, t): the transform helpers, the joints'
// sin / cos, the Kinova joint step and the cost against a fixed or a per-step target.  Shared by the
// rollout kernels, the quadrotor step (sincos_joint) and the plan kernel (mppi_plan.hip).
#pragma once
#include "mppi_device.h"

namespace {

// ---------------------------------------------------------------- FK helpers
struct Mat34 { float m[12]; };   // rows 0..2 of a homogeneous transform

// T <- T * [O3 | o]  (O a constant joint origin, uniform across the wave)
__device__ __forceinline__ void mul_affine(Mat34& T, const float* O) {
    Mat34 r;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float t0 = T.m[4 * i], t1 = T.m[4 * i + 1], t2 = T.m[4 * i + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) r.m[4 * i + j] = t0 * O[j] + t1 * O[4 + j] + t2 * O[8 + j];
        r.m[4 * i + 3] = t0 * O[3] + t1 * O[7] + t2 * O[11] + T.m[4 * i + 3];
    }
    T = r;
}

// T <- T * Rot(axis, q) for a revolute joint (Rodrigues, transformation_matrix.py:68-93)
__device__ __forceinline__ void mul_revolute(Mat34& T, const JointDev& J, float c, float s) {
    const float omc = 1.0f - c;
    if (J.axis_z) {   // R = [[c,-s,0],[s,c,0],[0,0,c+(1-c)]]
        const float r22 = c + omc;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float a0 = T.m[4 * i], a1 = T.m[4 * i + 1];
            T.m[4 * i] = a0 * c + a1 * s;
            T.m[4 * i + 1] = a1 * c - a0 * s;
            T.m[4 * i + 2] = T.m[4 * i + 2] * r22;
        }
        return;
    }
    const float vx = J.ax[0], vy = J.ax[1], vz = J.ax[2];
    float R[9];
    R[0] = c + J.axx[0] * omc; R[1] = J.axx[1] * omc - vz * s; R[2] = J.axx[2] * omc + vy * s;
    R[3] = J.axx[3] * omc + vz * s; R[4] = c + J.axx[4] * omc; R[5] = J.axx[5] * omc - vx * s;
    R[6] = J.axx[6] * omc - vy * s; R[7] = J.axx[7] * omc + vx * s; R[8] = c + J.axx[8] * omc;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float a0 = T.m[4 * i], a1 = T.m[4 * i + 1], a2 = T.m[4 * i + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) T.m[4 * i + j] = a0 * R[j] + a1 * R[3 + j] + a2 * R[6 + j];
    }
}

// T <- T * Slide(axis * q) (transformation_matrix.py:38-55)
__device__ __forceinline__ void mul_prismatic(Mat34& T, const JointDev& J, float q) {
    const float d0 = J.ax[0] * q, d1 = J.ax[1] * q, d2 = J.ax[2] * q;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        T.m[4 * i + 3] += T.m[4 * i] * d0 + T.m[4 * i + 1] * d1 + T.m[4 * i + 2] * d2;
}

// sin/cos of a joint angle.  The reference evaluates them in the state dtype
// (fp32, or fp64 when update_joint got float64 arrays, mppi.py:197) and rounds
// into the fp32 transform (transformation_matrix.py:68-93).  Here: reduce the angle to
// f in [-1/2, 1/2] revolutions in the angle's own precision, then the hardware
// v_sin_f32 / v_cos_f32 of 2 pi f (2 transcendentals + 4 ops; a Cody-Waite reduction
// with minimax polynomials is ~25, ocml sincosf ~130 with a Payne-Hanek branch).
// Measured on MI355X over random angles in [-3 pi, 3 pi]
// (tools/microbench7.hip, profiles/r01/sincos_accuracy.txt): max error 1.8e-7 (fp64
// angle) and 2.6e-7 (fp32 angle) absolute, vs 9e-8 for the polynomials -- 1e2 below the
// trajectory tolerances.
__device__ __forceinline__ void sincos_joint(double q, float& s, float& c) {
    const double r = q * 0.15915494309189533577;
    const float f = (float)(r - rint(r));
    s = __builtin_amdgcn_sinf(f);
    c = __builtin_amdgcn_cosf(f);
}

// fp32 state (torch.sin of a float32 tensor): 1/2pi = C_HI + C_LO, the fractional
// revolution by two FMAs.
__device__ __forceinline__ void sincos_joint(float q, float& s, float& c) {
    const float n = __builtin_rintf(q * 0.15915494309189535f);
    float f = fmaf(q, 0.15915494309189535f, -n);
    f = fmaf(q, 6.4206382e-09f, f);
    s = __builtin_amdgcn_sinf(f);
    c = __builtin_amdgcn_cosf(f);
}

// One Kinova joint: T <- T * [P | o] * Rz(q), P a signed permutation fixed at
// compile time (kKinova, mppi_dev.h): the rotation part is register renaming and
// negation (source modifiers), the translation only its nonzero components.
// (PRE: the angle's sin and cos are given, else formed here, between the origin and the rotation)
template <int J, bool PRE, typename QT>
__device__ __forceinline__ void kin_joint_x(Mat34& T, const float* O, QT q, float s, float c) {
    constexpr KinOrigin k = kKinova[J];
    Mat34 r;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float tr = T.m[4 * i + 3];
        if (k.tmask & 1) tr = fmaf(T.m[4 * i + 0], O[3], tr);
        if (k.tmask & 2) tr = fmaf(T.m[4 * i + 1], O[7], tr);
        if (k.tmask & 4) tr = fmaf(T.m[4 * i + 2], O[11], tr);
#pragma unroll
        for (int j = 0; j < 3; ++j) r.m[4 * i + j] = (k.s[j] > 0) ? T.m[4 * i + k.p[j]] : -T.m[4 * i + k.p[j]];
        r.m[4 * i + 3] = tr;
    }
    if constexpr (!PRE) sincos_joint(q, s, c);
    // Rodrigues about z (transformation_matrix.py:68-93).  Its R22 = fl(c + fl(1 - c)) is
    // 1 or 1 - 2^-24 (a rounding tie of 1 - c for some c < -1/2); the fast path takes 1,
    // as it takes the origins' pi/2 rotations exactly (<= 6e-8 relative).
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float a0 = r.m[4 * i], a1 = r.m[4 * i + 1];
        T.m[4 * i] = a0 * c + a1 * s;
        T.m[4 * i + 1] = a1 * c - a0 * s;
        T.m[4 * i + 2] = r.m[4 * i + 2];   // R22 = fl(c + fl(1 - c)) taken as 1
        T.m[4 * i + 3] = r.m[4 * i + 3];
    }
}
template <int J, typename QT>
__device__ __forceinline__ void kin_joint(Mat34& T, const float* O, QT q) {
    kin_joint_x<J, false>(T, O, q, 0.0f, 0.0f);
}
template <int J>
__device__ __forceinline__ void kin_joint_sc(Mat34& T, const float* O, const float s, const float c) {
    kin_joint_x<J, true>(T, O, 0.0f, s, c);
}

// atan2 with octant reduction and a degree-8 odd minimax polynomial on [0,1]
// (SLEEF atanf coefficients): ~25 ops, <= 3.5 ulp (ocml atan2f: 45 ops).
__device__ __forceinline__ float atan2_fast(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    float rc = __builtin_amdgcn_rcpf(mx);
    rc = rc * fmaf(-mx, rc, 2.0f);
    const float a = (mx > 0.0f) ? mn * rc : 0.0f;
    const float t = a * a;
    float u = 0.00282363896258175373077393f;
    u = fmaf(u, t, -0.0159569028764963150024414f);
    u = fmaf(u, t, 0.0425049886107444763183594f);
    u = fmaf(u, t, -0.0748900920152664184570312f);
    u = fmaf(u, t, 0.106347933411598205566406f);
    u = fmaf(u, t, -0.142027363181114196777344f);
    u = fmaf(u, t, 0.199926957488059997558594f);
    u = fmaf(u, t, -0.333331018686294555664062f);
    float r = fmaf(a * t, u, a);
    if (ay > ax) r = 1.57079632679489661923f - r;
    if (__builtin_signbit(x)) r = 3.14159265358979323846f - r;
    return __builtin_copysignf(r, y);
}

// Pose cost of one (k,t): w_pos*||p - p*|| + w_ori*||eulerZYX(R^T R*)||
// (pose_cost.py:24-63; rotation_conversions.py:277-319; inv(R) of the
// orthonormal FK rotation taken as R^T).
__device__ __forceinline__ float pose_cost(const Mat34& T, const VehicleConst& vc, float wp, float wo) {
    const float dx = T.m[3] - vc.tpos[0], dy = T.m[7] - vc.tpos[1], dz = T.m[11] - vc.tpos[2];
    const float cp = __builtin_amdgcn_sqrtf(dx * dx + dy * dy + dz * dz);
    const float* tR = vc.tR;
    const float r00 = T.m[0] * tR[0] + T.m[4] * tR[3] + T.m[8] * tR[6];
    const float r10 = T.m[1] * tR[0] + T.m[5] * tR[3] + T.m[9] * tR[6];
    const float r20 = T.m[2] * tR[0] + T.m[6] * tR[3] + T.m[10] * tR[6];
    const float r21 = T.m[2] * tR[1] + T.m[6] * tR[4] + T.m[10] * tR[7];
    const float r22 = T.m[2] * tR[2] + T.m[6] * tR[5] + T.m[10] * tR[8];
    const float yaw = atan2_fast(r10, r00);
    const float pitch = asinf(fminf(fmaxf(-r20, -1.0f), 1.0f));
    const float roll = atan2_fast(r21, r22);
    const float co = __builtin_amdgcn_sqrtf(yaw * yaw + pitch * pitch + roll * roll);
    return wp * cp + wo * co;
}

// The same cost against a target row (p*, R* row-major) the lane holds in registers: the tracking
// kernels (rollout_body TRK, k_plan).  pose_cost restated, not lifted: the fixed-target kernels'
// code stays as it is.
__device__ __forceinline__ float pose_cost_row(const Mat34& T, const float (&g)[12], float wp, float wo) {
    const float dx = T.m[3] - g[0], dy = T.m[7] - g[1], dz = T.m[11] - g[2];
    const float cp = __builtin_amdgcn_sqrtf(dx * dx + dy * dy + dz * dz);
    const float r00 = T.m[0] * g[3] + T.m[4] * g[6] + T.m[8] * g[9];
    const float r10 = T.m[1] * g[3] + T.m[5] * g[6] + T.m[9] * g[9];
    const float r20 = T.m[2] * g[3] + T.m[6] * g[6] + T.m[10] * g[9];
    const float r21 = T.m[2] * g[4] + T.m[6] * g[7] + T.m[10] * g[10];
    const float r22 = T.m[2] * g[5] + T.m[6] * g[8] + T.m[10] * g[11];
    const float yaw = atan2_fast(r10, r00);
    const float pitch = asinf(fminf(fmaxf(-r20, -1.0f), 1.0f));
    const float roll = atan2_fast(r21, r22);
    const float co = __builtin_amdgcn_sqrtf(yaw * yaw + pitch * pitch + roll * roll);
    return wp * cp + wo * co;
}
// A row of the target table (V, H, 12: p*(3) then R*(9), 48 B) as three 16 B loads; DRONE reads p* only.
template <bool POS_ONLY>
__device__ __forceinline__ void load_target_row(const float* row, float (&g)[12]) {
    const float4* r4 = reinterpret_cast<const float4*>(row);
    const float4 a = r4[0];
    g[0] = a.x; g[1] = a.y; g[2] = a.z; g[3] = a.w;
    if constexpr (!POS_ONLY) {
        const float4 b = r4[1], c = r4[2];
        g[4] = b.x; g[5] = b.y; g[6] = b.z; g[7] = b.w;
        g[8] = c.x; g[9] = c.y; g[10] = c.z; g[11] = c.w;
    }
}

}  // namespace
