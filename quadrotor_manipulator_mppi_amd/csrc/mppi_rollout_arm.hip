// mppi_rollout_arm.hip -- arm rollout kernels, fp64 state (the ROS node feeds float64 arrays, mppi.py:196-200).
// H <= 32 (one 32-lane segment per rollout) lives in mppi_rollout_arm_h32.hip (its own scheduler).
#include "mppi_rollout_launch.h"

extern "C" int mppi_launch_rollout_arm64(const DevParams* p, int threads, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    // (dispatch_geom's geometries, the H <= 32 one from its own unit)
    if (p->nch == 1 && p->L == 32) return mppi_launch_rollout_arm64_h32(p, threads, stream);
    return pick_geom<false>(*p, [&](auto nch, auto l) {
        return launch_rollout_t<MPPI_MODEL_ARM, 7, nch(), l(), true>(*p, threads, s);
    });
}
// the tracking kernels (k_rollout_tt; MPPI_COST_TARGET_TRACK), the H <= 32 one from its own unit
extern "C" int mppi_launch_rollout_arm64_tt(const DevParams* p, const float* ttab, int threads, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    if (p->nch == 1 && p->L == 32) return mppi_launch_rollout_arm64_h32_tt(p, ttab, threads, stream);
    return pick_geom<false>(*p, [&](auto nch, auto l) {
        return launch_rollout_tt<MPPI_MODEL_ARM, 7, nch(), l(), true>(*p, ttab, threads, s);
    });
}
// the field kernels (k_rollout_df; mppi_create_scene_field), the H <= 32 one from its own unit.  Ahead of the
// scene launcher on purpose: kernels are emitted in this order, and the scene kernels stay the unit's
// last, as in the builds before the field (the code object's last kernel has no alignment fill behind it).
extern "C" int mppi_launch_rollout_arm64_df(const DevParams* p, const float* ttab, float* scene, const float* field, int threads, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    if (p->nch == 1 && p->L == 32) return mppi_launch_rollout_arm64_h32_df(p, ttab, scene, field, threads, stream);
    return pick_geom<false>(*p, [&](auto nch, auto l) {
        return launch_rollout_df<MPPI_MODEL_ARM, 7, nch(), l(), true>(*p, ttab, scene, field, threads, s);
    });
}
// the scene kernels (k_rollout_ob; mppi_create_scene), the H <= 32 one from its own unit
extern "C" int mppi_launch_rollout_arm64_ob(const DevParams* p, const float* ttab, float* scene, int threads, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    if (p->nch == 1 && p->L == 32) return mppi_launch_rollout_arm64_h32_ob(p, ttab, scene, threads, stream);
    return pick_geom<false>(*p, [&](auto nch, auto l) {
        return launch_rollout_ob<MPPI_MODEL_ARM, 7, nch(), l(), true>(*p, ttab, scene, threads, s);
    });
}
