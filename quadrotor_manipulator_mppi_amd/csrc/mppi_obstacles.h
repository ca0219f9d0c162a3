// mppi_obstacles.h -- the sphere scene of an obstacle-avoiding engine (mppi_create_scene): the layout of
// its device buffer and the arithmetic of one (body sphere, obstacle) pair.  Shared by the scene rollout
// (mppi_rollout.h rollout_body OBS), the plan kernel (mppi_plan.hip) and the host (mppi_layout.cpp fills
// the buffer, tools/obstacle_host_check.cpp replays it), so it compiles as HIP and as plain C++.
//
// The scene buffer, in 4-byte words:
//   body table (engine-wide, kSceneBodyW words)
//     [0] n_body   [1] w_obs   [2] margin   [3] penalty   [4] clearance offset (words from the base)
//     [5] plan-clearance offset   [6] K   [7] spare
//     [kSceneRng + s], s = 0 .. kSceneSlots: the first sphere of frame slot s (the last word: n_body).
//         Slot 0 is the base transform times the folded leading fixed joints (DevParams::j0), slot
//         1 + j the frame after chain joint j0 + j; the spheres are sorted by slot.
//     [kSceneSph + 4 b]: sphere b's offset in its slot's frame (3) and radius
//   one block per vehicle (kSceneObsW words): [0] n obstacles, [1..3] spare, then n rows of 8:
//     centre (3), radius, velocity (3), spare
//   the per-sample clearances (V, K) and the plan's clearances (V, H), each 256 B aligned
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define MPPI_OBS_FN __host__ __device__ __forceinline__
#else
#define MPPI_OBS_FN inline
#endif

namespace mppi {

constexpr int kSceneMaxObs = 16, kSceneMaxBody = 16;
constexpr int kSceneSlots = 16 + 1;                       // the base and MPPI_MAX_JOINTS joint frames
constexpr int kSceneRng = 8;                              // kSceneSlots + 1 words
constexpr int kSceneSph = 28;                             // 16-byte aligned
constexpr int kSceneBodyW = kSceneSph + 4 * kSceneMaxBody;   // 92
constexpr int kSceneObsW = 4 + 8 * kSceneMaxObs;          // 132
constexpr int kSceneLdsW = kSceneBodyW + kSceneObsW;      // what a block stages: 224 words
static_assert(kSceneRng + kSceneSlots + 1 <= kSceneSph, "the slot ranges end before the spheres");
static_assert(kSceneLdsW % 4 == 0 && kSceneLdsW <= 270, "the staged scene keeps the dynamic LDS base 16 B aligned");
constexpr inline int64_t scene_align(int64_t words) { return (words + 63) & ~int64_t(63); }
constexpr inline int64_t scene_clr_off(int V) { return scene_align(kSceneBodyW + (int64_t)V * kSceneObsW); }
constexpr inline int64_t scene_plan_off(int V, int K) { return scene_clr_off(V) + scene_align((int64_t)V * K); }
constexpr inline int64_t scene_words(int V, int K, int H) { return scene_plan_off(V, K) + scene_align((int64_t)V * H); }

// an integer word of the buffer, kept wave-uniform on the device (it bounds the loops below)
MPPI_OBS_FN int scene_int(const float* w) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readfirstlane(__float_as_int(*w));
#else
    int32_t i;
    memcpy(&i, w, sizeof(i));
    return i;
#endif
}
MPPI_OBS_FN float scene_sqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(x);
#else
    return sqrtf(x);
#endif
}

// One pair: body sphere centre (cx, cy, cz), radius rb; obstacle row ob (8 words) at its row-t centre
// c + vel * tau, tau = (t + 1) dt.  g = d - r_b - r_o; the hinge sum and the running min clearance.
MPPI_OBS_FN void obs_pair(float cx, float cy, float cz, float rb, const float* ob, float tau, float margin,
                          float& hinge, float& gmin) {
    const float dx = cx - fmaf(ob[4], tau, ob[0]), dy = cy - fmaf(ob[5], tau, ob[1]), dz = cz - fmaf(ob[6], tau, ob[2]);
    const float d = scene_sqrt(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
    const float g = (d - rb) - ob[3];
    hinge += fmaxf(0.0f, margin - g);
    gmin = fminf(gmin, g);
}

// The spheres of frame slot `slot` against the vehicle's obstacles: T = rows 0..2 of the frame's world
// transform (row-major 3x4), body = the body table, veh = the vehicle's block.
MPPI_OBS_FN void obs_frame(const float* T, const float* body, const float* veh, int slot, float tau,
                           float& hinge, float& gmin) {
    const int b0 = scene_int(body + kSceneRng + slot), b1 = scene_int(body + kSceneRng + slot + 1);
    const int n = scene_int(veh);
    const float margin = body[2];
    for (int b = b0; b < b1; ++b) {
        const float* s = body + kSceneSph + 4 * b;
        const float cx = fmaf(T[0], s[0], fmaf(T[1], s[1], fmaf(T[2], s[2], T[3])));
        const float cy = fmaf(T[4], s[0], fmaf(T[5], s[1], fmaf(T[6], s[2], T[7])));
        const float cz = fmaf(T[8], s[0], fmaf(T[9], s[1], fmaf(T[10], s[2], T[11])));
        for (int o = 0; o < n; ++o) obs_pair(cx, cy, cz, s[3], veh + 4 + 8 * o, tau, margin, hinge, gmin);
    }
}

// The step's term from the two accumulators: w_obs * hinge sum + penalty once when anything touches.
MPPI_OBS_FN float obs_step_cost(const float* body, float hinge, float gmin) {
    return fmaf(body[1], hinge, gmin < 0.0f ? body[3] : 0.0f);
}

}  // namespace mppi
