// mppi_integrator.h -- the double integrator's cumsums over the horizon: the DPP segment scans (H > 64,
// and the plan kernel) and the LDS-transposed integrator of the one-chunk kernels, with the wave
// priority helper of the rollout's phases.
#pragma once
#include "mppi_device.h"
#include "mppi_diag.h"

namespace {

// s_setprio takes an immediate: min(r, 3) for a wave-uniform r
__device__ __forceinline__ void set_wave_prio(int r) {
    if (r >= 3) __builtin_amdgcn_s_setprio(3);
    else if (r == 2) __builtin_amdgcn_s_setprio(2);
    else if (r == 1) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}

}  // namespace

// Inclusive fp32 segment sum (cost reduction; order-insensitive at tolerance).
template <int L>
__device__ __forceinline__ float seg_scan_f32(float x) {
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x111, 0xF, 0xF, true));
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x112, 0xF, 0xF, true));
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x114, 0xF, 0xF, true));
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x118, 0xF, 0xF, true));
    if (L >= 32) x += dpp_f32<0x142, 0xA>(x);
    if (L >= 64) x += dpp_f32<0x143, 0xC>(x);
    return x;
}

// The min of an L-lane segment (L = 32, 64) in every lane of it: the four in-row levels of
// wave_fold_all, then the row-pair swap (rows 0-1, 2-3: the 32-lane halves) and, for L = 64, the
// half swap.  Symmetric pairings: every lane of a segment ends with the same bits.
template <int L>
__device__ __forceinline__ float seg_min_f32(float x) {
    static_assert(L == 32 || L == 64, "segments of 32 or 64 lanes");
    x = fminf(x, dpp_all<0xB1>(x));
    x = fminf(x, dpp_all<0x4E>(x));
    x = fminf(x, dpp_all<0x141>(x));
    x = fminf(x, dpp_all<0x140>(x));
    {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
        x = fminf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
    if constexpr (L == 64) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
        x = fminf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
    return x;
}

// fp32 inclusive scans of NA independent dims inside L-lane segments, step-major
// (the DPP wait states of one dim are filled by the others).  Each step is one
// v_add_f32_dpp: x + dpp(x), where out-of-row sources read 0 (row_shr with
// bound_ctrl) or rows outside row_mask add 0 (row_bcast), so no zeroing moves.
template <int L, int NA>
__device__ __forceinline__ void seg_scan_f32_multi(float (&x)[NA]) {
    if (MPPI_KO & 1) return;
#define MPPI_SCAN_STEP(CTRL, RM, BC)                                                    \
    _Pragma("unroll") for (int a = 0; a < NA; ++a) x[a] += __int_as_float(             \
        __builtin_amdgcn_update_dpp(0, __float_as_int(x[a]), CTRL, RM, 0xF, BC));
    MPPI_SCAN_STEP(0x111, 0xF, true)
    MPPI_SCAN_STEP(0x112, 0xF, true)
    MPPI_SCAN_STEP(0x114, 0xF, true)
    MPPI_SCAN_STEP(0x118, 0xF, true)
#undef MPPI_SCAN_STEP
    // row_bcast steps as in-place v_add_f32_dpp: rows outside row_mask keep x (the
    // compiler's DPP combiner would zero a temporary and add instead).  s_nop 1 covers
    // the VALU-write -> DPP-read hazard the asm hides from the hazard recognizer.
    if (L >= 32) {
#pragma unroll
        for (int a = 0; a < NA; ++a)
            asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf" : "+v"(x[a]));
    }
    if (L >= 64) {
#pragma unroll
        for (int a = 0; a < NA; ++a)
            asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf" : "+v"(x[a]));
    }
}

// Value of segment s's lane l, as a wave-uniform (scalar) quantity.
template <int R>
__device__ __forceinline__ float seg_pick(float x, int sub, int l_in_seg, int L) {
    float r = read_lane_f32(x, l_in_seg);
#pragma unroll
    for (int s = 1; s < R; ++s) r = (sub == s) ? read_lane_f32(x, s * L + l_in_seg) : r;
    return r;
}

// ---------------------------------------------------------------------------
// Integrator in the transposed domain (NCH == 1).  The two cumsums of
// standard_normal_noise.py:41-48 as DPP scans cost 13 DPP ops per dim and lane
// (row_shr 1/2/4/8, row_bcast 15/31, wave_shr 1).  Instead the wave writes its
// controls to its LDS slot (row = lane = (segment, t), pitch P = NA rounded up to odd,
// so the transposed reads are bank-conflict free) and re-reads them with lane =
// (series = (segment, dim), chunk of CL consecutive t).  Each lane integrates its chunk
// sequentially (4 full-rate ops per element), the chunks of a series combine by an
// affine exclusive scan over CPS consecutive lanes (2 log2 CPS + 2 DPP moves), and the
// position increments go back through LDS to lane = t.  For a chunk starting at
// velocity V and position P (relative to q0, q0dot), element i:
//   dq(i) = P + lp(i) + (i + 1) dt V,   lp(i) = sum_{j <= i} (lv(j) dt + a_j dt^2 / 2),
//   lv(j) = sum_{m < j} a_m dt;   combine(L then R) : V = V_L + V_R,
//   P = P_L + P_R + n_R dt V_L  (n_R elements in R).
// q0dot enters as (t + 1) dt q0dot.  fp32 throughout (the old scans were fp32 too); the
// increments stay ~1e-10 from the reference's double-accumulated cumsums.
template <int L, int NA>
struct IntegGeom {
    static constexpr int R = 64 / L;
    static constexpr int S = R * NA;   // series per wave
    static constexpr int CPS = (S <= 4) ? 16 : (S <= 8) ? 8 : (S <= 16) ? 4 : (S <= 32) ? 2 : 1;
    static constexpr int CL = L / CPS;   // elements per chunk
    static constexpr int P = NA | 1;     // LDS row pitch (odd)
    static_assert(S * CPS <= 64 && CPS <= L, "integrator lane map");
};

// floats per wave slot in LDS: the block-combine deposit (4 + NCH*64*NA) and, for
// NCH == 1, the integrator's 64 x P transposition buffer
template <int NA, int NCH, int L>
constexpr int wave_slot_floats() {
    return (NCH == 1 && 64 * IntegGeom<L, NA>::P > 4 + NCH * 64 * NA) ? 64 * IntegGeom<L, NA>::P
                                                                     : 4 + NCH * 64 * NA;
}

template <int CTRL>
__device__ __forceinline__ float row_shr_f32(float x) {   // out-of-row sources read 0
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}

// inc[a] (lane = segment*L + t) = q(t) - q0 for the controls act[a] of this lane
template <int L, int NA>
__device__ __forceinline__ void integrate_lds(const float (&act)[NA], float* xw, const int lane, const float dt,
                                              const float dt2h, const float* vel0f, float (&inc)[NA]) {
    using G = IntegGeom<L, NA>;
    constexpr int P = G::P, CPS = G::CPS, CL = G::CL, S = G::S;
#pragma unroll
    for (int a = 0; a < NA; ++a) xw[lane * P + a] = act[a];
    wave_lds_handoff();
    const int sr = lane / CPS, ch = lane & (CPS - 1);
    const bool on = sr < S;
    const int seg = sr / NA, a = sr - seg * NA;
    const int rb = on ? (seg * L + ch * CL) * P + a : 0;
    float lv = 0.0f, lp = 0.0f, loc[CL];
#pragma unroll
    for (int i = 0; i < CL; ++i) {
        const float x = xw[rb + i * P];
        lp += fmaf(lv, dt, x * dt2h);
        lv = fmaf(x, dt, lv);
        loc[i] = lp;
    }
    // inclusive affine scan over the series' chunks (consecutive lanes of one DPP row)
    float V = lv, Q = lp;
#define MPPI_ISCAN(D, CTRL)                                                                if (CPS > D) {                                                                             const float vs = row_shr_f32<CTRL>(V), qs = row_shr_f32<CTRL>(Q);                       if (ch >= D) { Q = Q + fmaf((float)(D * CL) * dt, vs, qs); V = V + vs; }            }
    MPPI_ISCAN(1, 0x111)
    MPPI_ISCAN(2, 0x112)
    MPPI_ISCAN(4, 0x114)
    MPPI_ISCAN(8, 0x118)
#undef MPPI_ISCAN
    float Vx = row_shr_f32<0x111>(V), Qx = row_shr_f32<0x111>(Q);   // exclusive: previous chunk's
    if (ch == 0) { Vx = 0.0f; Qx = 0.0f; }
    const float v0 = on ? vel0f[a] : 0.0f;
    const float q0 = fmaf((float)(ch * CL) * dt, v0, Qx);   // chunk start incl. the q0dot drift
    const float vb = dt * (Vx + v0);
    wave_lds_handoff();
    if (on) {
#pragma unroll
        for (int i = 0; i < CL; ++i) xw[rb + i * P] = fmaf((float)(i + 1), vb, q0 + loc[i]);
    }
    wave_lds_handoff();
#pragma unroll
    for (int a2 = 0; a2 < NA; ++a2) inc[a2] = xw[lane * P + a2];
}
