// mppi_limits.hip -- the bounded kernels (an engine of mppi_create_limits; mppi_limits.h) that share a body with a
// kernel of another unit: k_rollout_aerial_b (mppi_rollout_aerial.h) and the bounded plans k_plan_quad_b and
// k_plan_aerial_b (mppi_plan_air.h).  A unit of their own: the plain kernels' code objects hold what they held.
// (k_rollout_quad_b and k_rollout_quad_tt_b live beside the kernels whose body they share, in mppi_rollout_quad.hip.)
#include "mppi_rollout_aerial.h"
#include "mppi_plan_air.h"

extern "C" int mppi_launch_rollout_aerial_b(const DevParams* p, const float* lim, int threads, void* stream) {
    (void)threads;   // block size chosen in launch_aerial
    return lim ? launch_aerial<true>(p, lim, stream) : -1;
}

// The bounded plans' launch: QUADROTOR and AERIAL, lim = the limits buffer; a block per vehicle, one wave.
extern "C" int mppi_launch_plan_b(const DevParams* p, const PlanParams* pp, const float* lim, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    if (!lim || p->H < 1 || p->H > 64 || p->V < 1 || pp->scene) return -1;
    const dim3 grid(p->V), block(64);
    if (p->model == MPPI_MODEL_QUADROTOR && p->A == 4)
        return pick<true, false>(p->q_literal_jinv != 0, [&](auto lit) {
            return go(k_plan_quad_b<lit()>, grid, block, 0, s, p->u_prev, lim, *pp, *p);
        });
    if (p->model == MPPI_MODEL_AERIAL && p->A == kAerialA && !pp->ttab)
        return pick<true, false>(p->q_literal_jinv != 0, [&](auto lit) {
            return go(k_plan_aerial_b<lit()>, grid, block, 0, s, p->u_prev, p->joints, lim, *pp, *p);
        });
    return -1;
}
