// mppi_rollout_wb.hip -- whole-body rollout kernels.
#include "mppi_rollout_launch.h"

extern "C" int mppi_launch_rollout_wb(const DevParams* p, int threads, void* stream) {
    return dispatch_geom<MPPI_MODEL_WHOLEBODY, 10, false>(*p, threads, (hipStream_t)stream);
}
// the tracking kernels (k_rollout_tt; MPPI_COST_TARGET_TRACK)
extern "C" int mppi_launch_rollout_wb_tt(const DevParams* p, const float* ttab, int threads, void* stream) {
    return dispatch_geom_tt<MPPI_MODEL_WHOLEBODY, 10, false>(*p, ttab, threads, (hipStream_t)stream);
}
// the scene kernels (k_rollout_ob; mppi_create_scene)
extern "C" int mppi_launch_rollout_wb_ob(const DevParams* p, const float* ttab, float* scene, int threads, void* stream) {
    return dispatch_geom_ob<MPPI_MODEL_WHOLEBODY, 10, false>(*p, ttab, scene, threads, (hipStream_t)stream);
}
// the field kernels (k_rollout_df; mppi_create_scene_field)
extern "C" int mppi_launch_rollout_wb_df(const DevParams* p, const float* ttab, float* scene, const float* field, int threads, void* stream) {
    return dispatch_geom_df<MPPI_MODEL_WHOLEBODY, 10, false>(*p, ttab, scene, field, threads, (hipStream_t)stream);
}
