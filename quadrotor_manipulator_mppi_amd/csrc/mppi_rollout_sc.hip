// mppi_rollout_sc.hip -- the self-collision rollout kernels of a scene engine (k_rollout_sc;
// mppi_create_scene_self without a field): ARM fp64 and fp32 state and WHOLEBODY, every geometry of the
// ladder.  The kernels of an engine with a field (k_rollout_sf) are mppi_rollout_sf.hip's.
#include "mppi_rollout_launch.h"

// The self launch: members = the spheres that appear in a pair (the centre column's rows; 0 with an
// empty pair list).  field non-null: the field kernels' unit.
extern "C" int mppi_launch_rollout_self(const DevParams* p, const float* ttab, float* scene, const float* field, int members,
                                        int threads, void* stream) {
    if (field) return mppi_launch_rollout_self_field(p, ttab, scene, field, members, threads, stream);
    return dispatch_self<false>(*p, ttab, scene, nullptr, members, threads, (hipStream_t)stream);
}
