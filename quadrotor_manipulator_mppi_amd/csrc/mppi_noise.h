// mppi_noise.h -- the device noise: Philox4x32-10 / Philox2x32-10 and the Box-Muller that makes standard
// normals of their words (noise).  Shared by the rollout kernels, the quadrotor rollout
// and the Philox readback kernel (mppi_rollout_drone.hip).
#pragma once
#include "mppi_device.h"
#include "mppi_diag.h"

namespace {

// ------------------------------------------------------------------- Philox
// a ^ b ^ k in one VALU op: gfx950's v_bitop3_b32 with truth table 0x96 (three-input
// XOR).  The compiler emits two v_xor_b32 for it (there is no v_xor3 on gfx950).
__device__ __forceinline__ uint32_t xor3_sk(uint32_t a, uint32_t b, uint32_t k) {
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "s"(k));
    return r;
}

__device__ __forceinline__ void philox10(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3,
                                         uint32_t k0, uint32_t k1) {
    k0 = __builtin_amdgcn_readfirstlane(k0);   // the key is wave-uniform: keep it scalar
    k1 = __builtin_amdgcn_readfirstlane(k1);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {   // key schedule in place (opaque scalar adds): hoisting 18 round keys
                   // would spill SGPRs in the rollout kernel
            asm volatile("s_add_u32 %0, %0, 0x9e3779b9" : "+s"(k0) :: "scc");
            asm volatile("s_add_u32 %0, %0, 0xbb67ae85" : "+s"(k1) :: "scc");
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;   // one v_mad_u64_u32 each
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = xor3_sk((uint32_t)(p1 >> 32), c1, k0), n2 = xor3_sk((uint32_t)(p0 >> 32), c3, k1);
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    }
}

// One standard-normal pair per 32-bit Philox word (Box-Muller on the hardware
// transcendental units: v_log_f32 (log2), v_sqrt_f32, v_sin_f32 / v_cos_f32 with the
// argument in revolutions).  The radius takes the top 18 bits, u1 = (w>>14 + 1/2) 2^-18,
// the angle the low 14, u2 = ((w & 0x3fff) + 1/2) 2^-14 (midpoint grids: the radial CDF
// is off by <= 2^-19, the angle's midpoint rule by O(2^-28); the tail is cut at 5.1
// sigma, mass 3e-7).  One Philox4x32-10 call thus yields 8 normals: the 7 arm dims take
// one call and the 10 whole-body dims two (two words per pair took 2 and 3).
__device__ __forceinline__ void box_muller32(uint32_t w, float& z0, float& z1) {
    if (MPPI_KO & 32) { z0 = __uint_as_float((w & 0x3FFFFFu) | 0x3F800000u); z1 = z0 - 1.5f; return; }
    const float u1 = ((float)(w >> 14) + 0.5f) * 3.814697265625e-6f;      // 2^-18
    const float u2 = ((float)(w & 0x3FFFu) + 0.5f) * 6.103515625e-5f;     // 2^-14
    // -2 ln u1 lies in [1.3e-6, 26.3] (u1 >= 2^-19): the bare v_sqrt_f32 (1 ulp) needs none
    // of the denormal scaling and correction steps __builtin_sqrtf adds (~12 VALU)
    const float r = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
    z0 = r * __builtin_amdgcn_cosf(u2);
    z1 = r * __builtin_amdgcn_sinf(u2);
}

// Philox2x32-10 (Salmon et al., SC'11; Random123's philox2x32): one 32x32 -> 64 multiply
// per round instead of two, for the draws that need at most 2 words.
__device__ __forceinline__ void philox2x10(uint32_t& c0, uint32_t& c1, uint32_t k) {
    k = __builtin_amdgcn_readfirstlane(k);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) asm volatile("s_add_u32 %0, %0, 0x9e3779b9" : "+s"(k) :: "scc");
        const uint64_t p = (uint64_t)0xD256D193u * c0;   // one v_mad_u64_u32
        const uint32_t n0 = xor3_sk((uint32_t)(p >> 32), c1, k);
        c1 = (uint32_t)p;
        c0 = n0;
    }
}

// The key of the Philox2x32 draws: the 64-bit seed folded to 32 bits, plus the control
// step times the golden ratio (a bijection of the step for a fixed seed).
__host__ __device__ __forceinline__ uint32_t philox2_key(uint32_t seed_lo, uint32_t seed_hi, uint32_t step) {
    return (seed_lo ^ (seed_hi * 0x85EBCA6Bu)) + step * 0x9E3779B9u;
}
// Its second counter word: (veh<<8 | t) ^ (step<<16) (t < 256 = MPPI_MAX_HORIZON).  The step
// in the counter as well as in the key: two seeds whose folded 32-bit keys meet at some pair
// of steps still draw different words unless the steps are equal too.  The uniform part
// (veh<<8 ^ step<<16) is one scalar value, so the lane pays one OR, as before.
__host__ __device__ __forceinline__ uint32_t philox2_ctr1(uint32_t veh, uint32_t t, uint32_t step) {
    return t | ((veh << 8) ^ (step << 16));
}

// Standard normals z[a], a < NA, of sample kg at step t (noise):
//   * normals 8j .. 8j+7 (j < NA/8): Philox4x32-10 call j, counter (kg, t, veh<<8 | j, step),
//     key (seed lo, seed hi); word i gives the pair (8j+2i, 8j+2i+1);
//   * the r = NA mod 8 left over: r <= 4 -> one Philox2x32-10 call, counter
//     (kg, philox2_ctr1(veh, t, step)), key philox2_key(seed, step), its words giving pairs 8J.., 8J+2..
//     (J = NA/8); r >= 5 -> Philox4x32-10 call J as above.
// (the whole-body's 10 dims: one 4x32 call + one 2x32 call, 30 multiplies instead of 40)
// The draw in two halves (the rollout overlaps them with LDS latency, k_rollout): the
// Philox words of one (k, t) -- word 4j + i of call j, then the Philox2x32 words -- and the
// normals Box-Muller makes of them.
template <int NA>
constexpr int draw_words() {
    return 4 * (NA / 8 + ((NA % 8) >= 5 ? 1 : 0)) + (((NA % 8) >= 1 && (NA % 8) <= 4) ? 2 : 0);
}
template <int NA>
__device__ __forceinline__ void draw_philox(uint32_t (&w)[draw_words<NA>()], uint32_t kg, uint32_t t, uint32_t veh,
                                            uint32_t step, uint32_t s0, uint32_t s1) {
    constexpr int J = NA / 8, REM = NA % 8;
    constexpr int N4 = J + (REM >= 5 ? 1 : 0);   // Philox4x32 calls
#pragma unroll
    for (int j = 0; j < N4; ++j) {
        w[4 * j] = kg; w[4 * j + 1] = t; w[4 * j + 2] = (veh << 8) | (uint32_t)j; w[4 * j + 3] = step;
        if (!(MPPI_KO & 2)) philox10(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3], s0, s1);
    }
    if constexpr (REM >= 1 && REM <= 4) {
        w[4 * N4] = kg; w[4 * N4 + 1] = philox2_ctr1(veh, t, step);
        if (!(MPPI_KO & 2)) philox2x10(w[4 * N4], w[4 * N4 + 1], philox2_key(s0, s1, step));
    }
}
template <int NA>
__device__ __forceinline__ void draw_box_muller(const uint32_t (&w)[draw_words<NA>()], float (&z)[NA]) {
#pragma unroll
    for (int i = 0; 2 * i < NA; ++i) {   // word i gives normals 2i, 2i + 1 (both layouts above)
        float a, b;
        box_muller32(w[i], a, b);
        z[2 * i] = a;
        if (2 * i + 1 < NA) z[2 * i + 1] = b;
    }
}
template <int NA>
__device__ __forceinline__ void draw_normals(float (&z)[NA], uint32_t kg, uint32_t t, uint32_t veh,
                                             uint32_t step, uint32_t s0, uint32_t s1) {
    uint32_t w[draw_words<NA>()];
    draw_philox<NA>(w, kg, t, veh, step, s0, s1);
    draw_box_muller<NA>(w, z);
}

// Philox words one (k, t) draw consumes (the raw layout of k_philox / oracle.philox_normals)
__host__ __device__ constexpr int philox_words(int NA) {
    return 4 * (NA / 8) + ((NA % 8) == 0 ? 0 : (NA % 8) <= 4 ? 2 : 4);
}

}  // namespace
