// mppi_self.h -- the self-collision pairs of a self engine (mppi_create_scene_self): the layout of the
// pair region behind its scene buffer and the arithmetic of one (body sphere, body sphere) pair.  Shared
// by the self rollout (mppi_rollout.h rollout_body SLF), the plan kernel (mppi_plan.hip) and the host
// (mppi_layout.cpp validates and fills the region, tools/self_collision_host_check.cpp replays it), so it
// compiles as HIP and as plain C++.
//
// A self engine's scene buffer is a scene engine's (mppi_obstacles.h: scene_words(V, K, H) words, every
// offset as it is there) with the pair region appended; body-table word [kSelfWord] -- spare, 0 on every
// other engine -- holds the region's word offset, so the kernels need no pointer of their own.
// The region, in 4-byte words:
//   header and tables (kSelfHdrW words, wave-uniform: the kernels stage them in LDS beside the scene)
//     [0] n_pairs   [1] w_self   [2] margin   [3] penalty   [4] n_members
//     [5] self-clearance offset (words from the scene buffer's base)   [6] plan self-clearance offset   [7] spare
//     [kSelfMem + b], b = 0 .. 15: the member index of body sphere b (its position in the body table's
//         sorted order), -1 for a sphere in no pair.  A member is a sphere that appears in at least one
//         pair; members are numbered in sorted order, at most kSelfMaxMembers.
//     [kSelfPair + 3 i]: pair i = (member of a, member of b, r_a + r_b)
//   the per-sample self clearances (V, K) and the plan's (V, H), each 256 B aligned
//
// The centre column.  A member's centre is formed in the chain walk at its own frame and needed when its
// partner's frame has arrived, so it has to outlive the frame.  Each lane keeps its members' centres in
// an LDS column of its own: word (3 m + axis) * pitch + lane's index, pitch = the block's threads --
// consecutive lanes hit consecutive banks, and a lane reads only what it wrote itself, so there is no
// barrier.  After the chain of a (k, t) a wave-uniform loop over the pairs reads six words per pair.
#pragma once
#include "mppi_field.h"

namespace mppi {

constexpr int kSelfMaxPairs = 32, kSelfMaxMembers = 16;
constexpr int kSelfWord = 7;                                  // the body table's word with the region's offset
constexpr int kSelfMem = 8;
constexpr int kSelfPair = kSelfMem + kSceneMaxBody;           // 24
constexpr int kSelfHdrW = kSelfPair + 3 * kSelfMaxPairs;      // 120
static_assert(kSelfMaxMembers <= kSceneMaxBody, "a member is a body sphere");
constexpr inline int64_t self_off(int V, int K, int H) { return scene_words(V, K, H); }
constexpr inline int64_t self_clr_off(int V, int K, int H) { return self_off(V, K, H) + scene_align(kSelfHdrW); }
constexpr inline int64_t self_plan_off(int V, int K, int H) { return self_clr_off(V, K, H) + scene_align((int64_t)V * K); }
// the whole scene buffer of a self engine
constexpr inline int64_t self_words(int V, int K, int H) { return self_plan_off(V, K, H) + scene_align((int64_t)V * H); }

// The dynamic LDS of a self rollout block in bytes (mppi_rollout_launch.h launch_rollout_self asserts
// the same figure from the kernels' own constants): the warm start, eight wave slots, three staged runs
// (costs, clearances, self clearances) and the centre column.  A = the action width.
constexpr inline int64_t self_dyn_lds(int A, int H, int threads, int iters, int members) {
    const int nch = (H + 63) / 64, L = H > 32 ? 64 : 32, R = 64 / L, P = A | 1;
    const int slot = (nch == 1 && 64 * P > 4 + 64 * A) ? 64 * P : 4 + nch * 64 * A;
    const int run = iters * (((threads / 64) * R + 3) & ~3);
    return 4 * (int64_t)(((H * A + 3) & ~3) + 8 * slot + 3 * run + 3 * members * threads);
}
// what a self block may use: the figure that needs no raised limit on either dispatch path, and the
// CU's own (a 64-thread block of the longest horizons lies between the two)
constexpr int kSelfLdsTarget = 64 * 1024, kSelfLdsMax = 160 * 1024;
// an upper bound of the self kernels' static LDS (3920 B; mppi_rollout_launch.h asserts it)
constexpr int kSelfStaticLds = 4096;

// obs_frame / obs_frame_field with the member store: each sphere of the slot against the vehicle's
// obstacles and (FLD, where set) the field, exactly as there -- the same operations in the same order,
// so a self engine's obstacle term and clearances equal a scene engine's bit for bit -- and a member's
// centre into the lane's column (col = the column's base plus the lane's index).  Restated, not shared,
// for the reason given at obs_frame_field.  Keep the three in step.
template <bool FLD>
MPPI_OBS_FN void obs_frame_self(const float* T, const float* body, const float* veh, int slot, float tau,
                                const float* fhdr, const float* cells, const float* slf, float* col, int pitch,
                                float& hinge, float& gmin) {
    const int b0 = scene_int(body + kSceneRng + slot), b1 = scene_int(body + kSceneRng + slot + 1);
    const int n = scene_int(veh);
    const bool set = FLD && scene_int(fhdr + 7) != 0;
    const float margin = body[2];
    for (int b = b0; b < b1; ++b) {
        const float* s = body + kSceneSph + 4 * b;
        const float cx = fmaf(T[0], s[0], fmaf(T[1], s[1], fmaf(T[2], s[2], T[3])));
        const float cy = fmaf(T[4], s[0], fmaf(T[5], s[1], fmaf(T[6], s[2], T[7])));
        const float cz = fmaf(T[8], s[0], fmaf(T[9], s[1], fmaf(T[10], s[2], T[11])));
        for (int o = 0; o < n; ++o) obs_pair(cx, cy, cz, s[3], veh + 4 + 8 * o, tau, margin, hinge, gmin);
        if (set) {
            const float g = field_sample(fhdr, cells, cx, cy, cz) - s[3];
            hinge += fmaxf(0.0f, margin - g);
            gmin = fminf(gmin, g);
        }
        const int m = scene_int(slf + kSelfMem + b);
        if (m >= 0) {
            float* const c = col + 3 * m * pitch;
            c[0] = cx; c[pitch] = cy; c[2 * pitch] = cz;
        }
    }
}

// The pairs of one (k, t), after its chain: g_ab = |c_a - c_b| - (r_a + r_b) from the lane's column; the
// hinge sum and the min clearance.
MPPI_OBS_FN void self_pairs(const float* slf, const float* col, int pitch, float& hinge, float& gmin) {
    const int n = scene_int(slf);
    const float margin = slf[2];
    for (int i = 0; i < n; ++i) {
        const float* r = slf + kSelfPair + 3 * i;
        const float* const ca = col + 3 * scene_int(r) * pitch;
        const float* const cb = col + 3 * scene_int(r + 1) * pitch;
        const float dx = ca[0] - cb[0], dy = ca[pitch] - cb[pitch], dz = ca[2 * pitch] - cb[2 * pitch];
        const float g = scene_sqrt(fmaf(dx, dx, fmaf(dy, dy, dz * dz))) - r[2];
        hinge += fmaxf(0.0f, margin - g);
        gmin = fminf(gmin, g);
    }
}

// The step's term from the two accumulators: w_self * hinge sum + penalty once when any pair touches.
MPPI_OBS_FN float self_step_cost(const float* slf, float hinge, float gmin) {
    return fmaf(slf[1], hinge, gmin < 0.0f ? slf[3] : 0.0f);
}

}  // namespace mppi
