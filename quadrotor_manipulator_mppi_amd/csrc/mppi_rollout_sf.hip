// mppi_rollout_sf.hip -- the self-collision rollout kernels of a field engine (k_rollout_sf;
// mppi_create_scene_self with a field): ARM fp64 and fp32 state and WHOLEBODY, every geometry of the ladder.
#include "mppi_rollout_launch.h"

extern "C" int mppi_launch_rollout_self_field(const DevParams* p, const float* ttab, float* scene, const float* field, int members,
                                              int threads, void* stream) {
    if (!field) return -1;
    return dispatch_self<true>(*p, ttab, scene, field, members, threads, (hipStream_t)stream);
}
