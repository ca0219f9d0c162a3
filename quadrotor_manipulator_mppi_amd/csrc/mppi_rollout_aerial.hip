// mppi_rollout_aerial.hip -- gfx950 rollout kernel of the aerial manipulator (MPPI_MODEL_AERIAL): the
// 6-DoF quadrotor of mppi_rollout_quad.hip carrying the Kinova arm of k_rollout.
//
// Action (thrust, tau_x, tau_y, tau_z, qdd_0..6), v = u_prev + eps on all 11 dims.  Per sample k:
//   base    the recurrence at the head of mppi_rollout_quad.hip (step 0 and t >= 1 forms, wrap,
//           quad_literal_jinv) through quad_axis_step as it stands, on dims 0..3;
//   arm     the joint double integrator of standard_normal_noise.py:32-50, as k_rollout integrates the
//           whole-body model's joints, on dims 4..10;
//   EE      at row t (the state after t + 1 steps)
//             EE(k,t) = [Rz(yaw) Ry(pitch) Rx(roll) | p](k,t) * M_fixed * chain(q(k,t))
//           with that row's base state (drone.py:126-154 = transformation_matrix.py:148-187);
//   cost    the pose cost of pose_cost.py:24-63 (mppi_fk.h pose_cost; stage weights for t < H - 1, terminal
//           at H - 1), S_k = sum_t.
// The coupling is kinematic only: quad_mass and quad_inertia are the loaded vehicle's as the user sets
// them, and arm motion does not react on the base.
//
// The base's dynamics are serial in t; everything else is not.  A block owns 16 rollouts per dynamics wave:
//   1. all waves draw the (16 x H x 11) noise tile (one Philox4x32 and one Philox2x32 call per (k, t)) and
//      load u_prev into LDS;
//   2. wave 0 steps the 16 rollouts through t as k_rollout_quad does, four lanes per rollout, and leaves
//      (p, rpy)(r, t) in an LDS pose tile as it goes -- no trajectory store and no cost on the serial chain;
//      meanwhile the block's other waves (idle in k_rollout_quad) run what does not depend on the base, a
//      rollout at a time with lane = t: the joint integrator, the joints' trajectory stores and the chain
//      FK in the base frame, which they keep in registers;
//   3. after one barrier those waves read the pose tile, form the attitude's three sin / cos pairs (off the
//      serial chain), compose, cost, store the base and EE planes and reduce S_k over the lanes;
//   4. after a second barrier wave 0 forms the block's online-softmin record in k_rollout's format for 11
//      dims, so k_finalize combines it unchanged.
// Block forms (DevParams::iters = dynamics waves per block), as k_rollout_quad's and for its reasons: one
// dynamics wave in 512 threads while the grid is at most 512 blocks (7 helper waves: 3 rollouts each at the
// most), one in 256 (3 helper waves, 6 rollouts each at the most), and four in 256 above 1024 blocks where
// the tiles of 64 rollouts fit (mppi_dev.h aerial_lds_floats).  The four-wave form has no helper wave:
// each wave runs phases 2 and 3 for its own 16 rollouts in turn (two-phase).
//
// Trajectory planes are k-major, (V, C, K, hp) with hp = H rounded up to 16, as k_rollout's: every plane
// store is issued with lane = t for one sample, so one instruction writes the sample's whole row, pad
// lanes t in [H, hp) included (they hold the ballistic continuation: zero acceleration, the last pose),
// in whole 64 B runs.  Channels: xyz, rpy, q, EE rows 0..2.  Samples past K are not costed or stored;
// their dynamics lanes replicate sample K - 1 and their weight is 0.
#include "mppi_rollout_aerial.h"

extern "C" int mppi_launch_rollout_aerial(const DevParams* p, int threads, void* stream) {
    (void)threads;   // block size chosen in launch_aerial
    return launch_aerial<false>(p, nullptr, stream);
}
