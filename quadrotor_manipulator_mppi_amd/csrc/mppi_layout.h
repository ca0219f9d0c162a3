// mppi_layout.h -- everything mppi_create derives from a configuration before it touches the
// device (mppi_layout.cpp), with the error function and the host math it is built from.  No HIP:
// the layout of any configuration can be computed, and checked, on a machine without a GPU
// (mppi_debug_layout; tests/test_capi_layout_cpu.py).  Internal: not part of the public ABI.
#pragma once
#include <vector>

#include "mppi_dev.h"
#include "mppi_obstacles.h"
#include "mppi_field.h"
#include "mppi_limits.h"
#include "mppi_self.h"
#include "mppi_edt.h"
#include "mppi_depth.h"

// mppi_engine::generic with every part switched back (MPPI_GENERIC_KERNELS=1)
constexpr int kGenericAll = 15;

namespace mppi_host {

// ------------------------------------------------------------- errors (mppi_host_math.cpp)
// Sets the calling thread's mppi_last_error string and returns st.
mppi_status fail(mppi_status st, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// ------------------------------------------- reference fp32 builders (mppi_host_math.cpp)
int nq_of(const mppi_config& c);
mppi_status validate(const mppi_config& c);
void rpy_to_R(float r, float p, float y, float* R);
void joint_origin(const mppi_joint& j, float* T16);
void unit_axis(const mppi_joint& j, float* a);
void base_from_xyzquat(const double* b, bool f64, float* T16);
void quat_xyzw_to_R(const float* q, float* R);
void euler_zyx(const float* m, float* ypr);
int savgol_taps(int window, int order, float* c);
void bake_joint(const mppi_joint& j, mppi::JointDev& d);
void mul34(const float* A, const float* B, float* C);
void fk_consts(const mppi_joint* joints, int nj, float* O16s, float* axes);
void host_fk_c(const mppi_joint* joints, int nj, const float* O16s, const float* axes, const double* q,
               const double* xyzquat, bool f64, float* out16);
void host_fk(const mppi_joint* joints, int nj, const double* q, const double* xyzquat, bool f64, float* out16);

// ------------------------------------------------------------ layout (mppi_layout.cpp)
// The engine's sizes, launch geometry, baked tables and kernel parameters.  The launch geometry (L,
// R, nch, nb, iters), P, hp, j0, chain_fast, sigma_diag and sdiag are dp's; dp and fp are zeroed
// (padding included) and then filled in every member that is not a device pointer -- those, and
// ovl_n, dbg and the per-launch members, mppi_create and the step set.
struct EngineLayout {
    mppi_config cfg;                    // as given, but WHOLEBODY without state_f64
    int K = 0, H = 0, A = 0, V = 0, nq = 0, qoff = 0, state_dim = 0, out_dim = 0, C = 0, threads = 0;
    int64_t out_bytes = 0;              // the mapped output buffer (off_xerr + 16)
    mppi::DevParams dp;
    mppi::FinParams fp;
    float sg_taps[mppi::kMaxW];
    float fixedM[12];                   // product of the leading fixed joints (folded into base)
    mppi::JointDev joints[mppi::kMaxJ]; // the baked chain table
    std::vector<float> sinv, gamma_t;   // cost_terms: Sigma^-1 (A,A) and gamma^t (H), else empty
    bool has_scene = false;             // mppi_create_scene: the scene kernels; its body table (kSceneBodyW words)
    std::vector<float> scene_body;
    bool has_field = false;             // mppi_create_scene_field (with has_scene): the field kernels; its descriptor
    mppi_field_desc field{};
    bool has_self = false;              // mppi_create_scene_self (with has_scene): the self kernels; the pair region's
    std::vector<float> self_region;     // header and tables (kSelfHdrW words) and the spheres that appear in a pair
    int self_members = -1;              // (the centre column's rows; -1: not a self engine)
    bool has_limits = false;            // mppi_create_limits: the bounded kernels; the bounds as last set (mppi_limits.h)
    mppi_limits limits{};
    int auto_threads = 512;             // the block of a configuration with block_threads = 0 (a self engine: self_layout)
    int fin_ts = 1, fin_tsz = 8;        // finalize t-slices
    int generic = 0;                    // MPPI_GENERIC_KERNELS=1 (tests, A/B): the kernels as before the role and
                                        // fixed-block ones.  Bits: 1 the finalize of every role with run-time
                                        // geometry, 2 the full FINAL on every step, 4 the rollout of every block
                                        // size, 8 the full rollout on every step ("finalize", "quiet",
                                        // "rollout", "quiet_rollout" set one of them; 1 sets all: kGenericAll)
};
// Reads MPPI_FIN_TSZ, MPPI_NO_KINOVA_PATH and MPPI_GENERIC_KERNELS, the switches that change the
// layout.  `c` has passed validate(); a configuration past a limit fails with its status and message.
mppi_status layout_of(const mppi_config& c, EngineLayout& l);

// ------------------------------------------------- the sphere scene (mppi_layout.cpp; mppi_obstacles.h)
// scene_validate: the errors of mppi_create_scene, for a configuration that passed validate().
// scene_body_table: the engine-wide part of the scene buffer (kSceneBodyW words) for a layout: the
// spheres on frames before the first unfolded joint (l.dp.j0) re-expressed in the folded frame (in
// double), all of them sorted by frame slot (stable), the slots' ranges, the weights and the offsets
// of the clearance outputs.  order (n_body ints, may be null): sorted position -> the caller's index.
// obstacles_validate / obstacles_fill: the errors of mppi_set_obstacles and one vehicle's block
// (kSceneObsW words) from the caller's arrays.
mppi_status scene_validate(const mppi_config& c, const mppi_scene& s);
void scene_body_table(const EngineLayout& l, const mppi_scene& s, float* table, int* order);
mppi_status obstacles_validate(int n_vehicles, int vehicle, int n, const float* center, const float* radius, const float* vel);
void obstacles_fill(float* block, int n, const float* center, const float* radius, const float* vel);
// ------------------------------------------------- rotor limits (mppi_layout.cpp; mppi_limits.h)
// limits_values_validate: the errors of mppi_set_limits' bounds (a NaN, lo > hi; the message names the dim).
// limits_validate: those of mppi_create_limits, for a configuration that passed validate(): the models whose
// outputs the finalize forms (named), a shard, then the bounds.
mppi_status limits_values_validate(const mppi_limits* lim);
mppi_status limits_validate(const mppi_config& c, const mppi_limits* lim);
// ------------------------------------------------- the distance field (mppi_layout.cpp; mppi_field.h)
// field_validate: the descriptor's errors of mppi_create_scene_field (the model's are scene_validate's).
// field_data_validate: those of mppi_set_distance_field's arrays (either may be null).
// field_header: the kFieldHdrW header words for a descriptor, an origin and the set flag.
// field_pack: d (nz, ny, nx) into the x-pair cells (2 * nvox words).
inline int64_t field_voxels(const mppi_field_desc& f) { return (int64_t)f.dims[0] * f.dims[1] * f.dims[2]; }
mppi_status field_validate(const mppi_field_desc* f);
// the whole of mppi_create_scene_field's argument check after validate(): the scene (null: the default one,
// returned in `use`) through scene_validate -- which refuses QUADROTOR -- then the descriptor
mppi_status field_engine_validate(const mppi_config& c, const mppi_scene* scene, const mppi_field_desc* f, mppi_scene& use);
mppi_status field_data_validate(const mppi_field_desc& f, const float* origin3, const float* d_zyx);
void field_header(const mppi_field_desc& f, const float* origin3, bool set, float* hdr);
void field_pack(const mppi_field_desc& f, const float* d_zyx, float* cells);
// ------------------------------------------------- self-collision pairs (mppi_layout.cpp; mppi_self.h)
// self_validate: the errors of mppi_create_scene_self's pair list, for a configuration and a scene that
// passed validate() and scene_validate(); every message names the pair.
// self_sep: the non-fixed chain joints between two frames (0: a rigid pair).
// self_table: the region's header and tables (kSelfHdrW words) for a layout -- the caller's sphere indices
// mapped through the body table's sort order (order: sorted position -> the caller's index, as
// scene_body_table returns it); returns the number of members.
// self_layout: layout_of for a self engine with that many members -- with block_threads = 0 the largest
// block of 256, 128, 64 threads whose LDS stays within kSelfLdsTarget (64 where none does); an explicit
// block the kernels cannot serve is refused with a message.
// self_engine_validate: the whole of mppi_create_scene_self's argument check after validate().
mppi_status self_validate(const mppi_config& c, const mppi_scene& s, const mppi_self_collision* sc);
int self_sep(const mppi_config& c, int frame_a, int frame_b);
int self_table(const EngineLayout& l, const mppi_scene& s, const mppi_self_collision& sc, const int* order, float* region);
int self_member_count(const mppi_self_collision& sc);
mppi_status self_layout(const mppi_config& c, int members, EngineLayout& l);
mppi_status self_engine_validate(const mppi_config& c, const mppi_scene* scene, const mppi_field_desc* f,
                                 const mppi_self_collision* sc, mppi_scene& use);
// ------------------------------------------------- occupancy grids (mppi_layout.cpp; mppi_edt.h)
// occupancy_validate: the errors of mppi_set_occupancy's arguments (origin3 may be null).
// occupancy_field: the host twin of the device transform (mppi_edt.hip) -- the same definition and the
// same inline for the value (mppi_edt.h edt_value), separable, in int32 squared distances: occ (nz, ny, nx)
// into d (nz, ny, nx) for a descriptor that passed field_validate.
mppi_status occupancy_validate(const float* origin3, const uint8_t* occ_zyx, float max_dist);
void occupancy_field(const mppi_field_desc& f, const uint8_t* occ_zyx, float max_dist, float* d_zyx);
// ------------------------------------------------- depth images (mppi_layout.cpp; mppi_depth.h)
// depth_validate: the errors of mppi_integrate_depth's view and image for a field of this descriptor.
// depth_params: the kernels' parameters of a validated view -- the reciprocals and the rotation, formed
// once here for both twins; the pointers are the caller's.
// depth_integrate: the host twin of k_depth_carve and k_depth_mark through the same inlines (p.depth and
// p.occ are host arrays); every node holds 0 or 1 afterwards.
// shift_validate: the errors of mppi_shift_map's arguments; the moved origin in origin_out.
// map_shift: the host twin of k_map_shift (p.src and p.occ host arrays).
mppi_status depth_validate(const mppi_field_desc& f, const mppi_depth_view* view, const float* depth_hw);
void depth_params(const mppi_field_desc& f, const mppi_depth_view& view, mppi::DepthParams& p);
void depth_integrate(const mppi::DepthParams& p);
mppi_status shift_validate(const mppi_field_desc& f, const int32_t* shift_xyz, float max_dist, mppi::ShiftParams& p, float* origin_out);
void map_shift(const mppi::ShiftParams& p);
// the MPPI_GENERIC_KERNELS bits (EngineLayout::generic) and what they set in dp and fp
void set_generic(EngineLayout& l, int generic);

// mapped output buffer layout (h_out): outputs, u0, stats, then the tagged records of a read step
// (k_finalize): per vehicle, 2 per dim -- (o1, u0, seq), (o2, nan flag, seq) -- and one
// (rho, eta, ess, seq), 16 B each, each written by ONE store; the host polls their tags and takes
// the values from the records themselves
inline size_t off_u0(const EngineLayout* l) { return ((size_t)l->V * l->out_dim * sizeof(double) + 15) & ~size_t(15); }
inline size_t off_stats(const EngineLayout* l) {
    return (off_u0(l) + (size_t)l->V * l->A * sizeof(float) + 15) & ~size_t(15);
}
inline size_t off_flags(const EngineLayout* l) { return off_stats(l) + (size_t)l->V * 16; }
inline size_t rec_count(const EngineLayout* l) { return (size_t)l->V * (2 * l->A + 1); }
// the peer exchange's sticky timeout word (16 B after the records): the step tag of a finalize
// block that gave a step up, written by that block, cleared only by the host (mppi_peer_reset)
inline size_t off_xerr(const EngineLayout* l) { return off_flags(l) + rec_count(l) * 16; }

// Trajectory planes: k_rollout rows (one rollout's H steps) are padded to 64 B, hp = H
// rounded up to 16 floats, and written whole.  With H = 100 the unpadded rows left partial
// 64 B sectors at both ends of every wave store, which the write-through stores hand to HBM
// as masked writes: arm K=4096 rollout 20.3 us at H = 100 vs 13.4 at H = 128
// (profiles/r02/ab_traj_row_pitch.txt).  k_rollout_quad writes t-major (C,H,Kp) planes,
// its rows (one step's K samples) padded the same way: Kp = K rounded up to 16.
inline int traj_pitch(const EngineLayout* l) {
    return l->cfg.model == MPPI_MODEL_QUADROTOR ? (l->K + 15) & ~15 : (l->H + 15) & ~15;
}
inline size_t traj_floats(const EngineLayout* l) {   // all vehicles' planes
    const size_t plane = l->cfg.model == MPPI_MODEL_QUADROTOR ? (size_t)traj_pitch(l) * l->H
                                                               : (size_t)l->K * traj_pitch(l);
    return (size_t)l->V * l->C * plane;
}

}  // namespace mppi_host
