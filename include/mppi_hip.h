/*
 * mppi_hip.h -- C-ABI of the MI355X-native MPPI rollout engine (libmppi_hip.so).
 *
 * Drop-in boundary for the mav_mppi control step.  The
 * reference has no native FFI: its hot path is the Python methods below, and a
 * host binding (ctypes, quadrotor_manipulator_mppi_amd/_capi.py) replaces the
 * torch op sequence each entry point stands for:
 *
 *   mppi_create         <- MPPI.__init__            mppi_solver/mppi.py:28-93,
 *                                                   mppi_solver/drone_mppi.py:8-37
 *   mppi_set_state      <- MPPI.update_joint        mppi.py:196-200 (arm),
 *                          MPPI.set_state           drone_mppi.py:179-183 (drone)
 *   mppi_set_target     <- target_pose / target     mppi.py:70-72, drone_mppi.py:141
 *   mppi_rollout        <- sampling + rollout + FK + cost + softmin partials
 *                          mppi.py:129-143 / drone_mppi.py:142-156
 *                          (standard_normal_noise.py:22-50, urdf_fk.py:79-108,
 *                           urdfparser.py:122-163, pose_cost.py:24-63)
 *   mppi_finalize       <- weighted noise + SavGol + control update
 *                          mppi.py:144-158 / drone_mppi.py:157-169
 *                          (mppi.py:173-193, svg_filter.py:13-90)
 *   mppi_read_outputs   <- the (qdes, vdes) / (x, v) returned by
 *                          compute_control_input (mppi.py:161-169 incl. the
 *                          check_reach host FK at :95-120; drone_mppi.py:175)
 *   mppi_step           <- MPPI.compute_control_input as one call
 *   mppi_get_*          <- the reference's intermediate tensors (noise,
 *                          q_samples/trajectory, S, weights, w_eps, u_prev),
 *                          returned in the reference's own layouts
 *
 * Conventions: plain pointers and sizes, no torch types.  Host pointers unless
 * a name says d_ (device).  Every call returns mppi_status (0 = ok); on error
 * mppi_last_error() returns a thread-local message.  Calls on one engine must be
 * serialised by the caller (the Python wrapper holds a lock).
 */
#ifndef MPPI_HIP_H
#define MPPI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPPI_ABI_VERSION 10
#define MPPI_COMM_ID_BYTES 128  /* ncclUniqueId */
#define MPPI_PEER_HANDLE_BYTES 64  /* hipIpcMemHandle_t */
#define MPPI_MAX_ACTION 16
#define MPPI_MAX_JOINTS 16
#define MPPI_MAX_HORIZON 256
#define MPPI_MAX_SAVGOL 31

typedef enum {
    MPPI_OK = 0,
    MPPI_ERR_INVALID_ARG = -1,
    MPPI_ERR_HIP = -2,
    MPPI_ERR_NONFINITE = -3,
    MPPI_ERR_STATE = -4,
    MPPI_ERR_COMM = -5,
    MPPI_ERR_PEER_TIMEOUT = -6  /* mppi_synchronize: a peer-exchange step was given up since the last
                                   mppi_peer_reset (the engine itself is fine; see mppi_peer_status) */
} mppi_status;

/* Rollout models.  A = action dimension. */
typedef enum {
    MPPI_MODEL_DRONE = 0,     /* xyz double integrator, squared position cost      (A=3)  drone_mppi.py   */
    MPPI_MODEL_ARM = 1,       /* joint double integrator + FK chain + pose cost    (A=nq) mppi.py         */
    MPPI_MODEL_WHOLEBODY = 2, /* drone xyz + arm joints, mobile-base FK, pose cost (A=3+nq) SURVEY A16    */
    MPPI_MODEL_QUADROTOR = 3, /* 6-DoF rigid-body quadrotor: thrust + body torques, Euler-angle attitude,
                               * squared position cost (A=4, H <= 64).  The model the reference ships
                               * commented out (drone_mppi.py:57-83, drone.py:114-154) */
    MPPI_MODEL_AERIAL = 4     /* aerial manipulator: the QUADROTOR's rigid body carrying the Kinova arm
                               * (A = 4 + nq = 11, H <= 64).  Action (thrust, tau_xyz, qdd_0..6); the base
                               * steps by the QUADROTOR recurrence on dims 0..3, the joints by the ARM's
                               * double integrator on dims 4..10; the pose cost is taken at
                               *   EE(k,t) = [Rz(yaw) Ry(pitch) Rx(roll) | p](k,t) M_fixed chain(q(k,t))
                               * with the attitude and position of that row of the rollout.  The coupling is
                               * kinematic only: quad_mass and quad_inertia are the loaded vehicle's as the
                               * user sets them, and arm motion does not react on the base.  The chain is the
                               * Kinova table of the ARM kernels (leading fixed joints, then seven revolute-z
                               * joints).  Not available on this model (MPPI_ERR_INVALID_ARG, AERIAL named
                               * in mppi_last_error): scenes, fields and self-collision, every cost_terms
                               * bit (target tracking included), shard_count > 1 */
} mppi_model;

typedef enum {
    MPPI_NOISE_PHILOX = 0,    /* device counter-based Philox4x32-10 + Box-Muller (production)          */
    MPPI_NOISE_INJECTED = 1   /* caller supplies eps (K,H,A) per step (parity: reference randn noise)  */
} mppi_noise_mode;

typedef enum {
    MPPI_JOINT_FIXED = 0,
    MPPI_JOINT_REVOLUTE = 1,
    MPPI_JOINT_PRISMATIC = 2,
    MPPI_JOINT_FLOATING = 3   /* free-flyer root of the dynamics model only (mppi_link)            */
} mppi_joint_type;

/* One entry of the active joint chain (urdfparser.py:133-161). xyz/rpy/axis as
 * the URDF floats (rounded to fp32 like torch.tensor(jt.origin.xyz)). */
typedef struct {
    int32_t type;       /* mppi_joint_type                                   */
    int32_t q_index;    /* index into the arm joint vector, -1 if not actuated */
    float xyz[3];
    float rpy[3];
    float axis[3];      /* raw URDF axis; normalised like transformation_matrix.py:63-66 */
    int32_t has_axis;   /* 0 -> (1,0,0) as urdfparser.py:140-143              */
} mppi_joint;

typedef struct {
    int32_t model;            /* mppi_model                                                     */
    int32_t n_vehicles;       /* V independent controllers batched in one launch (config C5)    */
    int32_t n_samples;        /* K samples owned by THIS engine (one shard)                      */
    int32_t n_horizon;        /* H                                                              */
    int32_t n_action;         /* A (3 drone, nq arm, 3+nq whole-body, 4 quadrotor, 4+nq aerial) */
    double dt;                /* 0.01 (mppi.py:42, drone_mppi.py:18); a Python float there       */
    double lambda_;           /* 0.1  (mppi.py:75, drone_mppi.py:33)                             */
    float sigma[MPPI_MAX_ACTION * MPPI_MAX_ACTION]; /* Sigma (A x A, row-major), eps = z^T Sigma */
    /* cost weights: pose (stage pos, stage ori, terminal pos, terminal ori) = 50,30,40,30
     * (cost_manager.py:25-28); drone uses w_stage_pos=100, w_term_pos=20 (drone_mppi.py:92,104) */
    float w_stage_pos, w_stage_ori, w_term_pos, w_term_ori;
    int32_t n_joints;
    mppi_joint joints[MPPI_MAX_JOINTS];
    int32_t savgol_window;    /* 5 drone, 9 arm (drone_mppi.py:160, mppi.py:149)                */
    int32_t savgol_order;     /* 2                                                              */
    int32_t noise_mode;       /* mppi_noise_mode                                                */
    uint64_t seed;            /* Philox key                                                     */
    int32_t device;           /* HIP device ordinal                                             */
    int32_t shard_rank;       /* sample sharding: this engine owns global samples               */
    int32_t shard_count;      /*   [rank*K, (rank+1)*K); partials exchanged by the caller.      */
                              /*   shard_count * n_samples <= 2^32: the noise stream counts the  */
                              /*   global sample in 32 bits (more: MPPI_ERR_INVALID_ARG)         */
    int32_t state_f64;        /* reproduce the reference's fp64 promotion of an fp64 arm state  */
    int32_t store_trajectory; /* write the trajectory buffer (q / p and EE 3x4 per (k,t)); after */
                              /*   a batch it holds the LAST step's (mppi_run_steps)            */
    int32_t store_noise;      /* write eps (K,H,A) (debug / parity readback)                    */
    int32_t check_reach;      /* host FK at qdes, L1 position error < reach_tol (mppi.py:95-120)*/
    float reach_tol;          /* 0.005                                                          */
    int32_t blocks_per_vehicle; /* rollout grid.x; 0 = auto                                     */
    int32_t block_threads;      /* rollout block size (multiple of 64); 0 = auto                */
    /* The CostManager terms the reference ships disabled (cost_manager.py:83-87), for the
     * ARM and WHOLEBODY models; summed after the pose terms in the reference's order
     * (covar, centering, joint tracking, action, joint limit).  Defaults = the reference's
     * weights (cost_manager.py:21-43, joint_space_cost.py:16,71-80). */
    int32_t cost_terms;         /* MPPI_COST_* bits; 0 = pose cost only, as the reference runs  */
    float w_covar;              /* covar_cost.py:20-25, scaled by lambda*(1-alpha)      (0.1)   */
    float cost_alpha;           /* cost_manager.py:22                                   (0.1)   */
    float cost_gamma;           /* per-step discount gamma^t of the joint/action terms  (0.98)  */
    float w_center;             /* joint_space_cost.py:19-27                            (1.0)   */
    float w_joint_track;        /* joint_space_cost.py:30-38 (target: mppi_set_joint_trajectory; zeros as mppi.py:134) */
    float w_action;             /* action_cost.py:14-24 on the perturbed controls v     (0.01)  */
    float joint_limit_penalty;  /* joint_space_cost.py:68-86                            (1e10)  */
    float q_center[MPPI_MAX_JOINTS];   /* centering target per arm joint                         */
    float q_lower[MPPI_MAX_JOINTS];    /* joint limits                                           */
    float q_upper[MPPI_MAX_JOINTS];
    /* MPPI_MODEL_QUADROTOR rigid body (drone.urdf:15-16; g and kd are undefined in the
     * commented reference loop, drone_mppi.py:64-79): */
    float quad_mass;            /* 14.7 kg                                                      */
    float quad_inertia[3];      /* diagonal body inertia 1.57, 3.93, 2.59                       */
    float quad_kd;              /* linear drag coefficient kd (0)                               */
    float quad_gravity;         /* g = (0, 0, -quad_gravity), 9.81                              */
    int32_t quad_literal_jinv;  /* 1: steps t >= 1 integrate rpy += dt inv(J(rpy)) omega exactly as
                                 * the commented loop (drone_mppi.py:73-76); 0 (default): J at
                                 * every step (J maps body rates to Euler rates, drone.py:114-124) */
    int32_t vehicle_offset;     /* fleet-wide index of this engine's vehicle 0 (vehicle sharding, config C5:
                                 * each GPU runs V of the fleet's vehicles).  The device noise is keyed by
                                 * the fleet-wide index, so an engine over vehicles [o, o+V) draws exactly
                                 * what one engine over the whole fleet draws for them.  0..32767-V */
} mppi_config;

typedef enum {
    MPPI_COST_COVAR = 1,
    MPPI_COST_CENTER = 2,
    MPPI_COST_JOINT_TRACK = 4,
    MPPI_COST_ACTION = 8,
    MPPI_COST_JOINT_LIMIT = 16,
    /* Not a CostManager term: the pose target moves along the horizon (mppi_set_target_trajectory).
     * Accepted on every model but AERIAL (which takes no cost_terms bit); bits 1..16 stay ARM / WHOLEBODY only. */
    MPPI_COST_TARGET_TRACK = 32
} mppi_cost_term;

/* Per-vehicle statistics of the last finalised step. */
typedef struct {
    float rho;          /* min_k S_k                                        */
    float eta;          /* sum_k exp(-(S_k - rho)/lambda)                   */
    float ess;          /* effective sample size 1 / sum_k w_k^2            */
    int32_t nonfinite;  /* 1 if rho/eta/u is not finite (reference propagates NaN); 2 if a
                           peer-exchange step gave up waiting for another rank (u_prev kept) */
    int32_t reach;      /* check_reach result (arm / whole-body)            */
    int32_t _pad;
} mppi_stats;

typedef struct mppi_engine mppi_engine;

int32_t mppi_abi_version(void);
const char* mppi_last_error(void);
/* sizeof(mppi_config), sizeof(mppi_joint), sizeof(mppi_stats): lets a binding check its layout. */
void mppi_struct_sizes(int32_t* config, int32_t* joint, int32_t* stats);

/* Reference defaults for a model (drone: K=1000 H=32 sigma=30I; arm: K=100 H=32
 * sigma=0.1I, Kinova chain must still be filled in by the caller). */
void mppi_config_default(mppi_config* cfg, int32_t model);

/* Sizes of the packed host-side state / output rows for a config. */
int32_t mppi_state_dim(const mppi_config* cfg);   /* doubles per vehicle  */
int32_t mppi_output_dim(const mppi_config* cfg);  /* doubles per vehicle  */
int32_t mppi_traj_channels(const mppi_config* cfg);

mppi_status mppi_create(const mppi_config* cfg, mppi_engine** out);
void mppi_destroy(mppi_engine* e);

/* Run on a caller stream (hipStream_t cast to void*); NULL = engine-owned stream. */
mppi_status mppi_set_stream(mppi_engine* e, void* hip_stream);

/* Joint-space tracking target of MPPI_COST_JOINT_TRACK per vehicle: (H, nq) fp32, the
 * joint_trajectories argument of CostManager.update_pose_cost (cost_manager.py:64-69;
 * the reference passes zeros, mppi.py:134).  NULL restores zeros. */
mppi_status mppi_set_joint_trajectory(mppi_engine* e, int32_t vehicle, const float* traj_h_nq);

/* Goal per vehicle: position (3) and orientation quaternion xyzw (4; ignored by DRONE). */
mppi_status mppi_set_target(mppi_engine* e, int32_t vehicle, const float* pos3, const float* quat_xyzw4);

/* Target trajectory of one vehicle, for an engine created with MPPI_COST_TARGET_TRACK in
 * cfg.cost_terms (else MPPI_ERR_STATE; vehicle out of range: MPPI_ERR_INVALID_ARG).  H rows: row t
 * is the pose wanted at horizon index t, the state after t + 1 integration steps, (t + 1) dt from
 * now -- a position (pos_h3, (H,3)) and an orientation quaternion xyzw (quat_h4, (H,4); ignored by
 * DRONE and QUADROTOR; rows need not be unit, mppi_target_rotation divides by |q|^2).
 *   ARM, WHOLEBODY   S_k = sum_{t<H-1} [w_sp |p_kt - p*_t| + w_so |eulerZYX(R_kt^-1 R*_t)|]
 *                          + w_tp |p_k,H-1 - p*_H-1| + w_to |eulerZYX(R_k,H-1^-1 R*_H-1)|
 *                          + the enabled extra terms (pose_cost.py:24-63 with the row for its constant)
 *   DRONE, QUADROTOR S_k = 100 sum_{t<H-1} |p_t - p*_t|^2 + 20 |p_H-1 - p*_H-1|^2 (drone_mppi.py:87-107)
 * quat_h4 NULL: every orientation row is the vehicle's fixed target orientation.  pos_h3 NULL
 * clears the table: every row is the vehicle's fixed target (mppi_set_target) again, which is also
 * the state of an engine never given a table; mppi_set_target refills the rows of a clear vehicle.
 * The arm's check_reach measures against row 0 (qdes is the state one step ahead); mppi_get_plan
 * measures cost_t[t] and pos_err[t] against row t.  A batch (mppi_run_steps(n)) uses one table for
 * all n steps: the table changes only through this call, between steps, like the state.  The rows
 * are copied into the engine's staging memory (the caller's arrays are free on return) and uploaded
 * on the engine's stream, ordered before the next step on either dispatch path. */
mppi_status mppi_set_target_trajectory(mppi_engine* e, int32_t vehicle, const float* pos_h3, const float* quat_h4);

/* Warm start (V,H,A) -- reference attribute u_prev (mppi.py:58, drone_mppi.py:29). */
mppi_status mppi_set_u_prev(mppi_engine* e, const float* u_prev);
mppi_status mppi_get_u_prev(mppi_engine* e, float* u_prev);

/* Measured state, packed per vehicle (doubles):
 *   DRONE:     x(3) v(3)
 *   ARM:       base xyz(3) quat xyzw(4) q(nq) qd(nq)        (q_full[:7]+q_full[7:], v_full[6:])
 *   WHOLEBODY: base xyz(3) quat xyzw(4) q(nq) base vel(3) qd(nq)
 *   QUADROTOR: xyz(3) rpy(3) (roll, pitch, yaw; R = Rz(yaw) Ry(pitch) Rx(roll), drone.py:126-154)
 *              v world(3) omega body(3)
 *   AERIAL:    xyz(3) rpy(3) q(nq) | v world(3) omega body(3) qd(nq)   (12 + 2 nq; float32 tensors)
 * Async host->device (pinned staging) on the engine stream. */
mppi_status mppi_set_state(mppi_engine* e, const double* state);

/* Step counter used as the Philox counter word (device resident).  On an engine connected by the
 * peer exchange it also moves the exchange epoch carried in the tags (every rank must call it the
 * same number of times, like the steps themselves): words left in the regions under the old
 * counter then never pass for a later step's. */
mppi_status mppi_set_step_counter(mppi_engine* e, uint32_t step);
mppi_status mppi_get_step_counter(mppi_engine* e, uint32_t* step);

/* Split-phase step (async, stream ordered).  d_noise: device eps (V,K,H,A) in
 * INJECTED mode, else NULL.  With shard_count > 1 either bind a zero-initialised
 * exchange buffer of shard_count*V*slot floats (mppi_rollout writes this shard's
 * slot and zeroes the others at the same positions); the caller sums it across
 * shards (one all-reduce), then calls mppi_finalize -- or let the engine own the
 * collective (mppi_comm_init below). */
mppi_status mppi_exchange_slot_floats(mppi_engine* e, int64_t* slot_floats);
mppi_status mppi_bind_exchange(mppi_engine* e, float* d_exchange);
mppi_status mppi_rollout(mppi_engine* e, const float* d_noise);
mppi_status mppi_finalize(mppi_engine* e);

/* Native collective: one process per GPU, one engine per process.
 * Every rank first checks mppi_comm_available (RCCL loadable, every entry point
 * present) and the ranks agree on the outcome before any of them enters the init.
 * Rank 0 makes an id, the caller broadcasts it (torch.distributed), and every rank
 * calls mppi_comm_init with it (collective); rank/world are the config's
 * shard_rank/shard_count.  The engine then owns an RCCL communicator over xGMI and
 * its zero-padded (shard_count, V, slot) exchange buffer, and mppi_step /
 * mppi_run_steps run rollout -> pack -> ONE all-reduce(SUM) -> finalize on the engine
 * stream with no host round trip.  mppi_exchange is that all-reduce alone (split
 * phases).  A one-rank communicator runs the same sharded path on one GPU.  The
 * reference has no distributed code (mppi.py:31 pins one device). */
mppi_status mppi_comm_available(void);
mppi_status mppi_comm_unique_id(uint8_t id[MPPI_COMM_ID_BYTES]);
/* The init is non-blocking with a deadline: the communicator (ncclCommInitRankConfig,
 * blocking = 0) is polled until it is ready or timeout_ms passes (<= 0: the
 * MPPI_COMM_INIT_TIMEOUT_MS environment value, default 60000); a communicator not
 * ready by then is aborted and the call returns MPPI_ERR_COMM, so a rank whose peers
 * never join returns instead of hanging.  mppi_comm_init = mppi_comm_init_ex(e, id, 0). */
mppi_status mppi_comm_init(mppi_engine* e, const uint8_t id[MPPI_COMM_ID_BYTES]);
mppi_status mppi_comm_init_ex(mppi_engine* e, const uint8_t id[MPPI_COMM_ID_BYTES], int32_t timeout_ms);
/* The communicator's own rank count and rank (ncclCommCount / ncclCommUserRank). */
mppi_status mppi_comm_info(mppi_engine* e, int32_t* nranks, int32_t* rank);
mppi_status mppi_exchange(mppi_engine* e);

/* Peer exchange: the sharded step without a collective (replaces the pack ->
 * all-reduce -> combine above for one-vehicle shards, at most 8 ranks).  Each rank's engine
 * opens an exchange region in its own GPU memory (uncached, 2 x ranks x finalize blocks x 68
 * words of 8 B: 5.6 MB at 8 ranks for the C4 shard) and exports it (mppi_peer_open -> an IPC
 * handle); the caller all-gathers the handles (torch.distributed) and every rank maps the
 * others' regions (mppi_peer_connect, the handles in rank order).  From then on each finalize
 * block stores its partial -- (rho, eta, eta2, nan) and its window of N[t], every 8 B word
 * tagged with the step -- into every other rank's region over xGMI, and combines the ranks'
 * partials (its own from registers, the others from its own region once all their tags are the
 * step's): a control step is the unsharded step's two kernels (native dispatch included), no
 * PACK launch, no host-enqueued collective.  Every rank finalises bit-identically, and one
 * rank reproduces the unsharded engine exactly.
 * Failure handling.  A block that waits 2 s for a peer proposes to give the step up; within a rank
 * the step is all or nothing (mppi_peer_info): the first block's proposal decides for every block
 * of the rank, so either every slice of u_prev is updated or every one is kept (w_eps = 0).  A rank
 * that gives the step up reports it twice -- into the control word of this rank in EVERY rank's
 * region (a peer still polling that step gives it up too) and into this engine's sticky word.  From
 * then on every rank's finalize blocks find the report in their own region and give every step up
 * at once (u_prev held on every rank, no 2 s waits) until the host resets the exchange, so no rank
 * keeps updating a warm start the others did not.  The host sees it as stats nonfinite = 2 from
 * mppi_read_outputs (this step's flag on any dim, or the sticky word: any block of any step of a
 * batch), as MPPI_ERR_PEER_TIMEOUT from mppi_synchronize, and through mppi_peer_status (this rank's
 * sticky word and every rank's report as stored in this rank's region).  Recovery is collective
 * (distributed.py ShardedEngine.resync): agree over the process group, take the warm start, step
 * counter and epoch of the lowest rank that is not torn (rank 0 normally), and call mppi_peer_reset
 * on every rank between two barriers.
 * Every rank must run the same sequence of steps with the same step counter (the tags are the
 * Philox counter): a rank that skips a step or rewinds its counter alone leaves the others
 * waiting out the 2 s bound.  mppi_get_weighted_noise gathers the last exchanged step's
 * partials (after mppi_kernel_timing, which exchanges nothing, it is undefined, as the
 * records it reads are then the timing launches').
 * Not combinable with mppi_comm_init / mppi_bind_exchange on the same engine. */
mppi_status mppi_peer_open(mppi_engine* e, uint8_t handle[MPPI_PEER_HANDLE_BYTES]);
mppi_status mppi_peer_connect(mppi_engine* e, const uint8_t* handles /* shard_count x MPPI_PEER_HANDLE_BYTES */);
/* The same connection for ranks inside ONE process (one process driving several engines: on one
 * GPU, or on several GPUs with peer access): mppi_peer_region returns this engine's region as a
 * device address after mppi_peer_open, and mppi_peer_connect_ptrs takes every rank's address in
 * rank order (this engine's own included) instead of IPC handles; across GPUs the caller enables
 * peer access first (hipDeviceEnablePeerAccess).  Every engine's steps must then be in flight
 * together (native dispatch: mppi_run_steps returns once the packets are queued). */
mppi_status mppi_peer_region(mppi_engine* e, uint64_t* device_address);
mppi_status mppi_peer_connect_ptrs(mppi_engine* e, const uint64_t* device_addresses /* shard_count */);
/* Connection check (collective, before the first step; a barrier between phases): phase 0 copies
 * a pattern word into this rank's slot of every rank's region; phase 1 checks that this rank's
 * region holds every rank's word (MPPI_OK, else MPPI_ERR_COMM) and clears it; phase 2 runs the
 * finalize's own tagged stores and polls over the regions in a one-wave kernel (every rank's word
 * within 2 s, else MPPI_ERR_COMM) and clears the region again. */
mppi_status mppi_peer_probe(mppi_engine* e, int32_t phase);
/* The exchange's failure state: sticky = this engine's timeout word (the given-up step's tag, 0 =
 * none; host memory, no device access); reports (kMaxPeers = 8 words, may be NULL) = the timeout
 * reports in this rank's region, word r from rank r (tag << 32 | 1, 0 = none; a device-to-host copy
 * after the engine's work); epoch (may be NULL) = the exchange epoch of the tags. */
mppi_status mppi_peer_status(mppi_engine* e, uint32_t* sticky, uint64_t* reports, uint32_t* epoch);
/* The connection and the warm start's integrity (ABI 9): connected = the ranks whose tagged word
 * reached this rank's region in mppi_peer_probe's kernel phase (phase 2; 0 before it), rank = this
 * engine's shard_rank, torn (may be NULL) = the step tag of a step this rank's warm start came out
 * of torn, 0 = none.  Within a rank a step is all or nothing: a finalize block updates its slice
 * of u_prev only if every peer word arrived in time with no timeout report in sight, and marks the
 * rank's decision word; a late block reports, waits 100 us for any such mark, and if its rank
 * committed keeps polling for a second 2 s bound instead of keeping its slice.  Only if that
 * passes too is the warm start torn (the resync then takes its u_prev from a rank that is not
 * torn). */
mppi_status mppi_peer_info(mppi_engine* e, int32_t* connected, int32_t* rank, uint32_t* torn);
/* Collective recovery after a timeout: with every rank's engine synchronised and a barrier passed
 * (no kernel writes into any region), clear this rank's region and sticky word and take the step
 * counter and epoch the ranks agreed on; a second barrier follows before any rank steps again. */
mppi_status mppi_peer_reset(mppi_engine* e, uint32_t step, uint32_t epoch);

/* Synchronise and copy the step's outputs: out (V, output_dim) doubles
 *   DRONE: x_des(3) v_des(3);  ARM: qdes(nq) vdes(nq);  WHOLEBODY: x(3) v(3) qdes(nq) vdes(nq)
 *   QUADROTOR: x_des = (xyz, rpy)(6), v_des = (v, omega)(6): the model's first step under u0
 *   AERIAL:    x_des(6) v_des(6) as QUADROTOR (the base's first step under u0[0..3]), then qdes(nq)
 *              vdes(nq) as ARM (mppi.py:157-158, qdes from the old u_prev[0])
 * u0 (V, A) floats and stats (V) may be NULL. */
mppi_status mppi_read_outputs(mppi_engine* e, double* out, float* u0, mppi_stats* stats);

/* One whole control step: set_state, (upload host noise), rollout, finalize, read_outputs.
 * h_noise: host eps (V,K,H,A) in INJECTED mode, else NULL.  Single-shard, a shard connected
 * by the peer exchange, or a shard with an engine-owned communicator. */
mppi_status mppi_step(mppi_engine* e, const double* state, const float* h_noise, double* out,
                      float* u0, mppi_stats* stats);

/* n back-to-back asynchronous control steps (rollout + finalize each, device
 * noise, state and warm start resident on the GPU); single-shard engines, shards connected
 * by the peer exchange, or shards with an engine-owned communicator (rollout, PACK,
 * all-reduce, finalize).
 * No host synchronisation: pair with mppi_synchronize / mppi_read_outputs.  The outputs of a
 * batch (mppi_read_outputs) are those of its LAST step; its earlier steps need not write any.
 * The same holds for the trajectory and cost buffers (mppi_get_trajectory, mppi_get_costs,
 * mppi_get_weights): after a batch they hold its last step's values, and the earlier steps do not
 * write them where the library has a quiet rollout for the engine's shape (mppi_kernel_info).
 * Single-shard and peer-exchange engines dispatch the steps natively: raw AQL packets on an
 * HSA queue the engine owns, the kernels from the library's code objects, their arguments
 * resident in device memory (MPPI_DISPATCH = auto (default) | aql (required) | hip). */
mppi_status mppi_run_steps(mppi_engine* e, int32_t n);

/* How the last mppi_run_steps and the last mppi_step were dispatched:
 * "<aql | hip: why not native>; calls: <aql (arguments in <where>) | hip>".  One-vehicle control
 * calls with device noise also go out as native packets: the state rides in the rollout's
 * arguments, which the host writes per call into a ring of blocks in host-writable device memory
 * (the GPU's CPU-visible kernarg or fine-grained pool, through the BAR, followed by an HDP
 * flush), or into pinned host memory when the device has no such pool or MPPI_AQL_CALL_HOSTMEM=1.
 * Native dispatch is refused (HIP launches instead, the reason here) when the engine's queue
 * fails its creation probe: dispatch ids that are not the queue's packet indices, as under a
 * tool that intercepts queues (rocprofv3 --pmc). */
mppi_status mppi_dispatch_info(mppi_engine* e, char* buf, int32_t len);
/* Which kernels the last mppi_run_steps and the last mppi_step ran:
 * "batch: rollout <symbol>, finalize <symbol>, quiet finalize <symbol | none>, quiet rollout
 * <symbol | none>; call: rollout <symbol>, finalize <symbol>" ("none" before the first of either),
 * the symbols as the library's code objects name them.  The outputs of a batch are those of its last
 * step: its earlier steps run a finalize that updates the warm start and writes nothing else (the
 * quiet finalize) and a rollout that writes its block records and nothing else -- no trajectory
 * planes, costs or handed-over vehicle constants (the quiet rollout) -- wherever the library has
 * them for the engine's shape.  Peer-exchange and sharded engines, stored or injected noise and
 * engines with timing or diagnostics keep the full rollout on every step.  An engine created with
 * MPPI_GENERIC_KERNELS=1 in the environment (tests, A/B) runs the kernels of every shape and the
 * full finalize and rollout on every step; the text then ends in "; MPPI_GENERIC_KERNELS". */
mppi_status mppi_kernel_info(mppi_engine* e, char* buf, int32_t len);

mppi_status mppi_synchronize(mppi_engine* e);

/* Prewarm for a controller that ticks with idle gaps (the arm node's rospy.Rate(100) loop,
 * kinova.py:101; no reference counterpart -- the reference's torch calls pay the same wake-up).
 * A call on a native queue left idle for more than ~50-100 us runs ~6-7 us longer than back to
 * back.  While window_us > 0 a host thread of the engine predicts the next mppi_step from the
 * median interval of the last calls' start times and, from window_us before that until the call
 * starts (at most window_us after it), puts a pair of one-wave packets on the engine's native
 * queue every 25 us; those write a scratch word only, so results are unchanged.  Calls back to back
 * (interval < 4 windows) or slower than 1 s get no touches; nor do calls that go out as HIP
 * launches (HIP dispatch, several vehicles, an RCCL or torch-collective shard; a peer-exchange
 * shard's calls are native).  Through each window the thread sleeps
 * between touches (MPPI_PREWARM_SPIN=1, a diagnostic: it spins).
 * window_us: 0 = off (the default), else 50 .. 5000.  mppi_destroy stops it.
 * mppi_get_prewarm: the window and the touches so far. */
mppi_status mppi_set_prewarm(mppi_engine* e, int32_t window_us);
mppi_status mppi_get_prewarm(mppi_engine* e, int32_t* window_us, int64_t* touches);

/* Readback in the reference's layouts (synchronous):
 * After mppi_run_steps(n) the costs, weights and trajectories are those of the batch's last step
 * (its earlier steps do not write them: mppi_run_steps).
 *   costs    S (V,K)                         compute_all_cost()
 *   weights  w (V,K)                         compute_weights()
 *   noise    eps (V,K,H,A)                   sampling()            [store_noise]
 *   traj     (V,K,H,C) C = traj_channels    DRONE p(3) / ARM q(nq)+EE(16) / WB p(3)+q(nq)+EE(16)
 *                                            QUADROTOR xyz(3)+rpy(3) (drone_mppi.py:62 trajectory)
 *                                            AERIAL xyz(3)+rpy(3)+q(nq)+EE(16)
 *            EE as the 4x4 row-major matrix of urdf_fk.py:108       [store_trajectory]
 *   wnoise   w_eps before / after SavGol (V,H,A), recomputed from the records the last
 *            step combined (a k_finalize launch in READBACK mode): the step itself stores
 *            no readback copies                                      */
mppi_status mppi_get_costs(mppi_engine* e, float* S);
mppi_status mppi_get_weights(mppi_engine* e, float* w);
mppi_status mppi_get_noise(mppi_engine* e, float* eps);
mppi_status mppi_get_trajectory(mppi_engine* e, float* traj);
mppi_status mppi_get_weighted_noise(mppi_engine* e, float* raw, float* smoothed);

/* The nominal plan: the rollout of the current warm start u_prev with zero noise from the current
 * state (synchronous; any engine: single, fleet, sharded, peer -- u_prev is the same on every rank).
 *   traj    (V,H,C)  C = mppi_traj_channels, the per-(t) layout of mppi_get_trajectory
 *   cost_t  (V,H)    the step's share of S: every enabled term, stage weights for t < H-1, terminal at H-1
 *   pos_err (V,H)    L1 distance of the EE (ARM, WHOLEBODY, AERIAL) or the vehicle (DRONE, QUADROTOR) position to
 *                    the target: check_reach's measure (utils/pose.py:121-123) along the plan
 *   S       (V)      the cost the rollout kernel gives this sample; sum_t cost_t
 * Any pointer may be NULL.  The state and targets are the ones last set (mppi_set_state / mppi_step,
 * mppi_set_target, mppi_set_joint_trajectory; zeros before the first), the controls the device's
 * u_prev: a zero warm start gives the ballistic path, after a step it is the plan just committed to.
 * One launch of k_plan on the engine's stream (one block per vehicle, lane = horizon step), outside
 * the control step: nothing the step reads or writes is touched. */
mppi_status mppi_get_plan(mppi_engine* e, float* traj, float* cost_t, float* pos_err, float* S);

/* ---- Obstacle avoidance: sphere scenes in the rollout cost (the project's own term; the reference
 * has no counterpart).  ARM, WHOLEBODY and DRONE; a QUADROTOR or AERIAL config with a scene is
 * MPPI_ERR_INVALID_ARG.
 *
 * Body spheres are the robot's geometry, engine-wide and fixed at creation (mppi_scene): sphere b
 * has a frame f, an offset o in that frame and a radius r_b > 0.  f indexes cfg.joints: frame f is
 * the world transform after joints 0..f of the chain, fixed joints included (forward_kinematics'
 * tf_fk after joint f); f = -1 is the base transform alone, T(base xyz, quat) -- for WHOLEBODY its
 * translation includes p_drone(k, t).  The world centre is T_f (o, 1).  DRONE has no chain: f = -1,
 * the centre p(k, t) + o in world axes.
 * Obstacles are per vehicle (mppi_set_obstacles), at most MPPI_MAX_OBSTACLES spheres: centre c
 * (world, m), radius r_o > 0, velocity vel (m/s).  At horizon row t (the state after t + 1
 * integration steps, as in mppi_set_target_trajectory) the centre is c + vel (t + 1) dt.  A batch
 * (mppi_run_steps(n)) uses the same set, unadvanced, for all n steps.
 * With d_bo the centre distance and g_bo = d_bo - r_b - r_o the clearance,
 *   x_obs(k,t) = w_obs sum_{b,o} max(0, margin - g_bo) + penalty [min_{b,o} g_bo < 0]
 *   S_k += sum_{t<H} x_obs(k,t)          (no discount; after the CostManager terms)
 * and the per-sample clearance clr_k = min_{t,b,o} g_bo (+inf with no obstacle or no body sphere).
 * Project constants (mppi_scene_default): w_obs = 100, margin = 0.05 m, penalty = 1e4; the default
 * body spheres are placeholders for the user's collision model: 0.05 m at each arm joint frame
 * origin, 0.30 m on frame -1 for WHOLEBODY and DRONE. */
#define MPPI_MAX_OBSTACLES 16
#define MPPI_MAX_BODY_SPHERES 16
typedef struct { int32_t frame; float offset[3]; float radius; } mppi_body_sphere;
typedef struct { int32_t n_body; mppi_body_sphere body[MPPI_MAX_BODY_SPHERES];
                 float w_obs, margin, penalty; } mppi_scene;
/* The project's default spheres and weights for the config's model and chain. */
void mppi_scene_default(mppi_scene* scene, const mppi_config* cfg);
/* mppi_create with a scene (NULL scene: mppi_create).  MPPI_ERR_INVALID_ARG: QUADROTOR, AERIAL, n_body
 * outside 0..16, a frame outside [-1, n_joints) (DRONE: other than -1), a non-finite value, a
 * radius <= 0, a negative weight.  Runs the scene kernels (k_rollout_ob; no quiet form). */
mppi_status mppi_create_scene(const mppi_config* cfg, const mppi_scene* scene, mppi_engine** out);
/* The obstacles of one vehicle: n in 0..16 (0 clears, the state after creation), center_n3 (n,3),
 * radius_n (n), vel_n3 (n,3) or NULL = static.  MPPI_ERR_STATE on an engine created without a scene;
 * MPPI_ERR_INVALID_ARG for n or the vehicle out of range, a non-finite value or a radius <= 0.  The
 * rows are copied to the engine's staging memory (the caller's arrays are free on return) and
 * uploaded on the engine's stream, ordered before the next step on either dispatch path. */
mppi_status mppi_set_obstacles(mppi_engine* e, int32_t vehicle, int32_t n, const float* center_n3,
                               const float* radius_n, const float* vel_n3);
/* clr (V,K): the per-sample clearances of the last rollout, valid as mppi_get_costs is. */
mppi_status mppi_get_clearances(mppi_engine* e, float* clr_vk);
/* clr (V,H): min_{b,o} g_bo at step t of the nominal plan (mppi_get_plan's rollout, whose cost_t
 * and S include the obstacle term on a scene engine). */
mppi_status mppi_get_plan_clearance(mppi_engine* e, float* clr_vh);

/* ---- Distance-field environments: a voxel signed distance field as one more obstacle of a scene
 * engine (walls, shelves, floors: what a planning stack hands over as an ESDF).  ARM, WHOLEBODY and
 * DRONE; QUADROTOR and AERIAL are MPPI_ERR_INVALID_ARG, as for a scene.
 *
 * The field is engine-wide: one world, shared by all V vehicles.  It is a nodal grid d[iz][iy][ix]
 * of fp32 signed distances in metres (negative inside), C order (nz, ny, nx); node (ix, iy, iz)
 * stands at origin + voxel (ix, iy, iz) in world axes.  Dims and voxel are fixed at creation; the
 * data and the origin are replaceable (a local map window that moves with the vehicle).
 * Sampling at a world point c: u = (c - origin) (1 / voxel), clamped per axis to [0, n - 1];
 * i = min(floor(u), n - 2), f = u - i; trilinear interpolation of the 8 nodes, x, then y, then z,
 * each lerp a + f (b - a).  A point outside the grid reads the value at its clamped position -- the
 * field does not extrapolate, so pad the grid by the distance the robot may leave it.  The clamp
 * comes before the integer conversion and maps NaN and +-inf coordinates onto the grid: no input
 * can form an address outside it.
 * The term: for body sphere b at row t, g_b,field = d(c_b(k,t)) - r_b joins the obstacle
 * accumulators above as one more obstacle:
 *   x_obs(k,t) = w_obs sum_{b, o in obstacles U {field}} max(0, margin - g_bo) + penalty [min g < 0]
 * and clr_k, the plan's cost_t, S and mppi_get_plan_clearance take the min / sum over the same
 * set.  No new weights; the field is static over the horizon and over a batch.  Before a field is
 * set, and after it is cleared, it contributes nothing (the engine equals a scene engine). */
#define MPPI_FIELD_MAX_VOXELS (1 << 21)
typedef struct { int32_t dims[3];   /* nx, ny, nz: each 2..512, product <= MPPI_FIELD_MAX_VOXELS */
                 float voxel;       /* m, > 0 */
                 float origin[3];
                 int32_t reserved;  /* 0 (the struct is 32 bytes) */ } mppi_field_desc;
/* mppi_create_scene with a field of these dims (scene NULL: mppi_scene_default).  The field buffer
 * and its pinned staging copy are allocated here; the field starts cleared.  MPPI_ERR_INVALID_ARG:
 * what mppi_create_scene refuses, a NULL descriptor, dims outside 2..512 or their product past
 * MPPI_FIELD_MAX_VOXELS, a voxel that is not finite and > 0, a non-finite origin.  Runs the field
 * kernels (k_rollout_df; no quiet form). */
mppi_status mppi_create_scene_field(const mppi_config* cfg, const mppi_scene* scene, const mppi_field_desc* field,
                                    mppi_engine** out);
/* Replaces the field: origin3 (NULL: keep the current one), d_zyx (nz,ny,nx) (NULL: clear -- the
 * field contributes nothing until the next set).  MPPI_ERR_STATE on an engine not created by
 * mppi_create_scene_field; MPPI_ERR_INVALID_ARG for a non-finite origin or value.  The data is
 * packed into the engine's staging memory (the caller's array is free on return) and uploaded on
 * the engine's stream, ordered before the next step on either dispatch path; no allocation. */
mppi_status mppi_set_distance_field(mppi_engine* e, const float* origin3, const float* d_zyx);

/* Occupancy grids: the field built on the device from the map a node actually holds (octomap, a
 * depth-camera voxel map, a local window).  A grid of nodes, each occupied or free, becomes a signed
 * field as follows.  D2_occ(n) is the smallest squared index distance from node n to an occupied node,
 * D2_free(n) the same to a free node: integers, at most 3 * 511^2.  Outside the grid is unknown and
 * supplies no seeds of either kind.  Nodes are the centres of cubes of side voxel:
 *   free node      d = +voxel (sqrt(D2_occ)  - 0.5)
 *   occupied node  d = -voxel (sqrt(D2_free) - 0.5)
 * so the zero of the trilinear interpolation falls on the face between an occupied node and its free
 * neighbour.  d is then clamped to [-cap, +cap]: cap = max_dist when max_dist > 0, else
 * voxel (nx + ny + nz), more than any in-grid distance.  A grid with no occupied node reads +cap
 * everywhere, one with no free node -cap.  Arithmetic: t = sqrtf((float)D2); d = voxel * (t - 0.5f), then
 * the clamp, all in fp32 with a correctly rounded square root -- the host and the device compute it with
 * the same inline, every operation is exactly rounded, and the two agree bit for bit.
 *
 * mppi_set_occupancy replaces the field by the one of occ_zyx (nz,ny,nx) uint8, C order, nonzero =
 * occupied; origin3 NULL keeps the current origin.  MPPI_ERR_STATE on an engine not created by
 * mppi_create_scene_field; MPPI_ERR_INVALID_ARG for a NULL occ_zyx, a non-finite origin, a max_dist that
 * is NaN or +inf.  The bytes are copied into the engine's staging memory (the caller's array is free on
 * return; one byte per node crosses the bus) and an exact separable distance transform in int32
 * squared distances (k_edt_x, k_edt_axis for y and z, k_edt_finish) runs on the engine's stream,
 * ordered before the next step on either dispatch path.  Its device scratch (9 bytes per node) is
 * allocated at the first call and never grows.  mppi_set_distance_field, with data or NULL, keeps
 * working on the same engine in any order. */
mppi_status mppi_set_occupancy(mppi_engine* e, const float* origin3, const uint8_t* occ_zyx, float max_dist);
/* The field as it stands on the device (synchronous): is_set (0: cleared), its origin, d_zyx (nz,ny,nx)
 * = the first word of every x-pair.  Any pointer may be NULL.  After mppi_set_distance_field(d) it
 * returns d bit for bit; after mppi_set_occupancy what the controller sees.  MPPI_ERR_STATE on an
 * engine not created by mppi_create_scene_field. */
mppi_status mppi_get_distance_field(mppi_engine* e, int32_t* is_set, float* origin3, float* d_zyx);

/* Depth images: the occupancy map carved and marked on the device from what a depth camera delivers, so
 * that only the image and a camera pose cross the bus (sensor -> map -> field -> rollout cost on the GPU).
 *
 * The map.  A field engine owns a persistent occupancy map: one byte per node, (nz, ny, nx), 0 = free,
 * 1 = occupied, all free until first written.  mppi_set_occupancy seeds it (nonzero reads back as 1);
 * mppi_set_distance_field, with data or NULL, leaves it alone, and the next map call (mppi_integrate_depth,
 * mppi_shift_map) rebuilds the field from the map.
 *
 * The view.  depth_hw is (height, width) float32 metres along the optical axis (sensor_msgs/Image 32FC1).
 * Rows and columns 0, stride, 2 stride, ... are used.  Per used pixel (column i, row j, value z):
 *   NaN, -inf, z < z_min     the pixel is skipped
 *   z_min <= z <= z_max      a return at z
 *   z > z_max, +inf          a miss: the ray ends at z_max and marks nothing
 * Arithmetic: fp32 throughout, every product-sum an explicit fmaf, no contraction.  inv_fx = 1 / fx,
 * inv_fy = 1 / fy, inv_voxel = 1 / voxel and R = mppi_target_rotation(quat_xyzw) are formed once on the host.
 *   xn = ((float)i - cx) inv_fx, yn = ((float)j - cy) inv_fy, p_cam = (xn z, yn z, z)
 *   w_d  = fmaf(R[3d], p0, fmaf(R[3d+1], p1, fmaf(R[3d+2], p2, pos_d)))
 *   ue_d = (w_d - origin_d) inv_voxel (the end point), uo_d = (pos_d - origin_d) inv_voxel (the camera)
 * A ray with a non-finite ue or uo is skipped.  A point u is in the grid iff -0.5 <= u_d < n_d - 0.5 on all
 * three axes, tested in float; only then is node_d = (int)floorf(u_d + 0.5f) formed.  The test comes before
 * the integer conversion, so no input can form an address outside the grid: not NaN, not +-inf, not 3e38
 * metres, not a camera a light-year away.
 * March: du = ue - uo, L = max_d |du_d|, n = (int)fminf(fmaxf(ceilf(2 L), 1), MPPI_DEPTH_MAX_SAMPLES),
 * inv_n = 1.0f / (float)n (a correctly rounded division); sample m, 0 <= m < n, is
 * u_d(m) = fmaf((float)m inv_n, du_d, uo_d).
 *   carve set F   the nodes of all in-grid samples of all rays, except a return's samples that fall in
 *                 that return's own end-point node (carve = 0: F is empty)
 *   mark set O    the in-grid end-point nodes of the returns
 * One image turns the map into (map \ F) U O: occupied wins within a frame.  The result is a pure function
 * of (map, image, view); it does not depend on thread order (both passes store constants).  The kernels
 * visit only the samples a conservative slab clip leaves (csrc/mppi_depth.h depth_clip); the result is the
 * set above, bit for bit, and the host twin runs the same inlines.
 * Out of scope: probabilistic (log-odds) fusion, lens distortion, point-cloud input, filtering the robot's
 * own arm out of the image (z_min is the only guard), per-vehicle maps. */
#define MPPI_DEPTH_MAX_PIXELS  (1 << 20)
#define MPPI_DEPTH_MAX_SAMPLES 16384
typedef struct {
    int32_t width, height;      /* columns, rows: >= 1, product <= MPPI_DEPTH_MAX_PIXELS            */
    int32_t stride;             /* rows and columns 0, stride, 2 stride, ... are used; >= 1          */
    int32_t carve;              /* 1: clear free space along the rays; 0: mark end points only       */
    float fx, fy, cx, cy;       /* pinhole, pixels (CameraInfo K[0], K[4], K[2], K[5]); fx, fy > 0   */
    float z_min, z_max;         /* m, 0 <= z_min < z_max, z_max / voxel <= 4096                      */
    float pos[3], quat_xyzw[4]; /* the optical frame (z forward, x right, y down) in the world       */
    int32_t reserved[3];        /* 0 */
} mppi_depth_view;              /* 80 bytes */
/* One image into the map (k_depth_carve, k_depth_mark), then the transform of mppi_set_occupancy under
 * max_dist, and the header's copy with the set flag on: all on the engine's stream, ordered before the next
 * step on either dispatch path.  The image is copied to pinned staging of its own (the caller's array is
 * free on return); staging and its device twin hold MPPI_DEPTH_MAX_PIXELS floats, allocated at the first
 * call and never grown.  If no map call came before, the transform's scratch is allocated and the map
 * zero-filled.  MPPI_ERR_STATE on an engine without a field; MPPI_ERR_INVALID_ARG for a NULL view or image,
 * a non-finite view value, fx or fy <= 0, a size, stride or z limit outside the ranges above, a quaternion
 * whose squared norm is outside [0.5, 2] (others are normalised, as targets are), a nonzero reserved word,
 * a max_dist that is NaN or +inf. */
mppi_status mppi_integrate_depth(mppi_engine* e, const mppi_depth_view* view, const float* depth_hw, float max_dist);
/* Moves the window with the vehicle (k_map_shift): new node (ix, iy, iz) = old node (ix + sx, iy + sy,
 * iz + sz), free where that falls outside the grid; the origin moves to fmaf((float)s_d, voxel, origin_d).
 * A zero shift changes nothing, |s_d| >= n_d clears the map.  The copy goes through the transform's int32
 * scratch (no new allocation); the transform runs and the field flag is set, as above.  MPPI_ERR_STATE
 * without a field; MPPI_ERR_INVALID_ARG for a NULL shift, a max_dist that is NaN or +inf, a shift that
 * takes the origin out of the finite range. */
mppi_status mppi_shift_map(mppi_engine* e, const int32_t shift_xyz[3], float max_dist);
/* The map as it stands on the device (synchronous), (nz, ny, nx), 0 or 1.  All free, with no allocation,
 * before the first map call.  MPPI_ERR_STATE without a field. */
mppi_status mppi_get_occupancy(mppi_engine* e, uint8_t* occ_zyx);

/* ---- Self-collision avoidance: pairs of body spheres in the scene rollout cost (the project's own
 * term; what a MoveIt-style stack keeps as the allowed-collision matrix, turned round: the pairs that
 * are NOT allowed to touch).  ARM and WHOLEBODY; DRONE (no chain: every pair is rigid), QUADROTOR and
 * AERIAL are MPPI_ERR_INVALID_ARG.
 *
 * A pair list is up to MPPI_MAX_SELF_PAIRS unordered pairs (a, b) of the scene's body spheres, indexed
 * as in mppi_scene.body; engine-wide and fixed at creation.  With c_b(k,t) the sphere's world centre
 * as the obstacle term defines it and g_ab = |c_a - c_b| - r_a - r_b,
 *   x_self(k,t) = w_self sum_{(a,b)} max(0, margin - g_ab) + penalty [min_{(a,b)} g_ab < 0]
 *   S_k += sum_{t<H} x_self(k,t)          (no discount; after the obstacle / field term)
 * and the per-sample self clearance sclr_k = min_{t,(a,b)} g_ab (+inf with no pair).  The weights are
 * the term's own (self margins are usually tighter than obstacle margins); project constants
 * (mppi_self_collision_default): w_self = 100, margin = 0.02 m, penalty = 1e4.  The term does not
 * depend on the base pose, so ARM and WHOLEBODY share the definition.
 * sep(a, b) is the number of non-fixed chain joints j with f_lo < j <= f_hi (the two spheres' frames):
 * a pair with sep = 0 is rigid -- its distance can never change -- and is refused as a configuration
 * error (frames -1 and 0 of the Kinova chain, whose joint 0 is fixed, are such a pair). */
#define MPPI_MAX_SELF_PAIRS 32
typedef struct { int32_t n_pairs; int32_t pair[MPPI_MAX_SELF_PAIRS][2];
                 float w_self, margin, penalty; int32_t reserved; } mppi_self_collision;
/* Every pair of the scene's spheres (scene NULL: mppi_scene_default) with sep >= 3, in lexicographic
 * (a, b) order, cut off at MPPI_MAX_SELF_PAIRS, with the default weights: like the default body
 * spheres a placeholder for the user's collision model. */
void mppi_self_collision_default(mppi_self_collision* out, const mppi_config* cfg, const mppi_scene* scene);
/* mppi_create_scene / mppi_create_scene_field with a pair list (scene NULL: mppi_scene_default; field
 * NULL: no distance field; self NULL: MPPI_ERR_INVALID_ARG).  MPPI_ERR_INVALID_ARG, with the pair
 * named in mppi_last_error: what those refuse, the DRONE model, n_pairs outside 0..32, an index outside
 * [0, n_body), a = b, the same unordered pair twice, a rigid pair, a non-finite or negative weight,
 * margin or penalty; and an explicit block_threads whose block would not hold the kernel's LDS (the
 * centres of the spheres that appear in a pair ride in a per-lane LDS column: 12 B per such sphere
 * and thread; a block of 64 threads always fits, and block_threads = 0 picks the largest of 256, 128
 * and 64 that keeps the block at or below 64 KiB).  The engine is a scene engine (and a field engine
 * with `field`): mppi_set_obstacles, mppi_get_clearances, mppi_set_distance_field and
 * mppi_set_occupancy work on it unchanged; mppi_get_plan's cost_t and S include the term.  Runs the
 * self kernels (k_rollout_sc, with a field k_rollout_sf; no quiet form). */
mppi_status mppi_create_scene_self(const mppi_config* cfg, const mppi_scene* scene, const mppi_field_desc* field,
                                   const mppi_self_collision* self, mppi_engine** out);
/* sclr (V,K): the per-sample self clearances of the last rollout, valid as mppi_get_costs is.
 * MPPI_ERR_STATE on an engine not created by mppi_create_scene_self. */
mppi_status mppi_get_self_clearances(mppi_engine* e, float* sclr_vk);
/* sclr (V,H): min_{(a,b)} g_ab at step t of the nominal plan (mppi_get_plan's rollout).
 * MPPI_ERR_STATE on an engine not created by mppi_create_scene_self. */
mppi_status mppi_get_plan_self_clearance(mppi_engine* e, float* sclr_vh);

/* ---- Rotor limits: bounds on thrust and body torque in the QUADROTOR and AERIAL rollouts (every MPPI
 * stack has control bounds; without them the optimum can be a plan the vehicle cannot fly).  DRONE, ARM
 * and WHOLEBODY are MPPI_ERR_INVALID_ARG: their outputs are formed inside the finalize, which limits
 * do not touch.
 *
 * Bounds lo[a] <= hi[a] on action dims a = 0..3 (thrust, tau_x, tau_y, tau_z), engine-wide.  Whether an
 * engine has limits is fixed at creation; the values may be replaced at run time (a degraded rotor, a
 * sagging battery).  -inf for lo and +inf for hi leave a side open; AERIAL's joint dims 4..10 are not
 * bounded.  For sample k, row t, dim a, with u = u_prev[t][a] and eps as drawn or injected, every
 * operation one fp32 operation, none fused with a neighbour:
 *   a0   = fl(u + eps)
 *   v'   = min(max(a0, lo), hi)
 *   eps' = (a0 == v') ? eps : fl(v' - u)                        the effective noise
 *   c    = (a0 == v') ? a0  : min(max(fl(u + eps'), lo), hi)    the control the dynamics integrate
 * An unsaturated draw is untouched bit for bit; c lies within [lo, hi] always.  eps' replaces eps
 * everywhere downstream of the draw: in the block records N = sum_k e_k eps'_k, in the stored noise
 * (store_noise, mppi_get_noise) and in the kernels' noise tile.  So u_prev + sum_k w_k eps'_k =
 * sum_k w_k v'_k, a convex combination of controls within the bounds, and the finalize is the plain
 * engine's.  mppi_get_plan integrates c with eps = 0: the clamped warm start.
 * u_prev itself stays the raw warm start of the reference's law, u_prev + SavGol(w_eps): the filter's
 * negative taps can carry a row past a bound by a small amount; the next rollout clamps what it
 * integrates.  The u0 that mppi_read_outputs and mppi_step return is clamped on the host, and the base's
 * twelve outputs (formed on the host for these two models) are the first step under that clamped u0.
 * An engine whose four bounds are all infinite equals the plain engine bit for bit: costs,
 * trajectories, stored noise, u_prev and outputs.
 * Runs the bounded kernels (k_rollout_quad_b, with MPPI_COST_TARGET_TRACK k_rollout_quad_tt_b,
 * k_rollout_aerial_b; k_plan_quad_b, k_plan_aerial_b) on every step of a batch (no quiet form). */
typedef struct { float lo[4], hi[4]; } mppi_limits;             /* thrust, tau_x, tau_y, tau_z */
/* thrust in [0, 2 m g] from cfg's quad_mass and quad_gravity (fp32 product); the torques unbounded. */
void mppi_limits_default(mppi_limits* lim, const mppi_config* cfg);
/* mppi_create with limits (NULL limits: mppi_create).  MPPI_ERR_INVALID_ARG, with the dim or the model
 * named in mppi_last_error: a NaN bound, lo > hi, the DRONE, ARM or WHOLEBODY model, shard_count > 1. */
mppi_status mppi_create_limits(const mppi_config* cfg, const mppi_limits* limits, mppi_engine** out);
/* Replaces the bounds: validated as at creation, copied to the engine's staging memory and uploaded on
 * the engine's stream, ordered before the next step on either dispatch path.  MPPI_ERR_STATE on an
 * engine not created with limits. */
mppi_status mppi_set_limits(mppi_engine* e, const mppi_limits* limits);
/* has: 1 on an engine created with limits (then *limits: the bounds as last set), else 0.  Either
 * output may be NULL. */
mppi_status mppi_get_limits(mppi_engine* e, int32_t* has, mppi_limits* limits);
/* Host replay of the four lines above (csrc/mppi_limits.h, the kernels' own; no GPU): u (H,4), eps
 * (K,H,4) into eps' (K,H,4) and c (K,H,4); either output may be NULL. */
mppi_status mppi_limits_apply(const mppi_limits* limits, const float* u_h4, const float* eps_kh4, int32_t K, int32_t H,
                              float* eps_eff_kh4, float* ctl_kh4);

#define MPPI_MAX_ELITES 64
/* The n lowest-cost samples of the last rollout of every vehicle, best first (synchronous).
 *   idx  (V,n) int32   sample index within this engine's K (a shard: local; global = shard_rank*K + idx)
 *   S    (V,n)         their costs: mppi_get_costs()[v, idx]
 *   w    (V,n)         their softmin weights: mppi_get_weights()[v, idx]
 *   traj (V,n,H,C)     their rollouts in mppi_get_trajectory's row layout (C = mppi_traj_channels)  [store_trajectory]
 * Any output pointer may be NULL.
 * Order: a total order, so every result is unique -- ascending in (cost, index), where -0 counts as
 * +0, +inf comes after every finite cost, every NaN (any sign or payload) after +inf, and equal
 * costs go by the lower index first: numpy's argsort(S[v], kind="stable")[:n].
 * Valid as mppi_get_costs / mppi_get_trajectory are: after mppi_step that call's samples, after
 * mppi_run_steps the batch's last step, after mppi_rollout that rollout; w uses the rho and eta
 * mppi_get_weights uses.
 * Errors: n < 1, n > MPPI_MAX_ELITES or n > K: MPPI_ERR_INVALID_ARG; traj on an engine created
 * without store_trajectory: MPPI_ERR_STATE (idx, S and w work on such an engine).
 * Two or three small launches on the engine's stream (select per share of the costs, select and
 * sort, gather the rows) and one copy, outside the control step: nothing the step reads or writes
 * is touched.  The buffers are allocated at the first call, for MPPI_MAX_ELITES. */
mppi_status mppi_get_elites(mppi_engine* e, int32_t n, int32_t* idx, float* S, float* w, float* traj);

/* Kernel timing with HIP events on the engine stream (bench / roofline). */
mppi_status mppi_enable_timing(mppi_engine* e, int32_t enable);
mppi_status mppi_get_timing(mppi_engine* e, double* rollout_ms_total, double* finalize_ms_total,
                            int64_t* n_rollout, int64_t* n_finalize);
/* Average device time of the two kernels measured back to back: n rollout launches
 * bracketed by one event pair, then n finalize launches bracketed by another (the
 * per-launch pairs of mppi_enable_timing add ~2-3 us of event overhead each).  The
 * warm start and step counter are saved and restored, and the timing launches write
 * their outputs (out/u0/stats) to device scratch, so the controller state and a pending
 * mppi_read_outputs are unchanged (mppi_get_weighted_noise then reflects the timing launches'
 * records: read it before timing).  The
 * trajectory and cost buffers (mppi_get_trajectory / mppi_get_costs / mppi_get_weights)
 * DO hold the timing loop's last rollout afterwards.  Single-shard engines with device
 * noise. */
mppi_status mppi_kernel_timing(mppi_engine* e, int32_t n, double* rollout_us, double* finalize_us);

/* mppi_kernel_timing plus pair_us: the average of n (rollout, finalize) pairs launched as
 * a control step runs them (the rollout after a finalize, its inputs just written).  Also
 * on a shard: the finalize then combines the exchange slots as they stand (no collective).
 * pair_us may be NULL. */
mppi_status mppi_kernel_timing_ex(mppi_engine* e, int32_t n, double* rollout_us, double* finalize_us,
                                  double* pair_us);

/* Average time of the step's all-reduce (mppi_exchange) over n back-to-back calls on the
 * engine stream.  Collective: every rank of the communicator calls it with the same n.
 * The slots are summed in place, so run a step (which repacks them) before reading outputs. */
mppi_status mppi_exchange_timing(mppi_engine* e, int32_t n, double* allreduce_us);

/* Algorithmic HBM bytes one mppi_rollout launch moves. */
int64_t mppi_rollout_bytes(const mppi_config* cfg);

/* Host-side helpers (no GPU needed): the fp32 constants the engine bakes, exposed so
 * the CPU test-suite can pin them against the reference fixtures. */
void mppi_joint_origin(const mppi_joint* j, float* T16);                 /* transformation_matrix.py:28-35 */
void mppi_base_transform(const double* xyzquat, int32_t f64, float* T16); /* urdf_fk.py:30-55             */
void mppi_target_rotation(const float* quat_xyzw, float* R9);            /* rotation_conversions.py:45-75 */
int32_t mppi_savgol_coefficients(int32_t window, int32_t order, float* c); /* svg_filter.py:50-55        */
/* Host FK of one joint vector (check_reach, urdf_fk.py:60-75); base as xyzquat. */
mppi_status mppi_host_fk(const mppi_joint* joints, int32_t n_joints, const double* q, const double* xyzquat,
                         int32_t f64, float* T16);

/* mppi_set_occupancy's field on the host, by the same definition and the same inline for the value:
 * desc as mppi_create_scene_field validates it, occ_zyx and d_zyx (nz,ny,nx).  Separable, at worst
 * O(n) per line per output node.  MPPI_ERR_INVALID_ARG for a NULL pointer, a descriptor
 * mppi_create_scene_field refuses, a max_dist that is NaN or +inf. */
mppi_status mppi_occupancy_field(const mppi_field_desc* desc, const uint8_t* occ_zyx, float max_dist, float* d_zyx);
/* mppi_integrate_depth's map update on the host, by the same definition and the same inlines: occ_zyx_inout
 * (nz,ny,nx) is updated in place (nonzero counts as occupied; on return every node holds 0 or 1) and equals
 * the device map, as mppi_get_occupancy returns it, bit for bit.  desc as mppi_create_scene_field validates it; the view and the image as
 * mppi_integrate_depth validates them (MPPI_ERR_INVALID_ARG, also for a NULL map). */
mppi_status mppi_depth_integrate_host(const mppi_field_desc* desc, const mppi_depth_view* view, const float* depth_hw,
                                      uint8_t* occ_zyx_inout);

/* Device RNG check: standard normals z (K,H,A) and the raw Philox words (K,H,W),
 * W = mppi_philox_words(A), exactly as the rollout kernel draws them for (seed, step,
 * vehicle, global k0..k0+K): A/8 Philox4x32-10 calls, then the A mod 8 remainder from one
 * Philox2x32-10 call (remainder <= 4) or one more Philox4x32-10 call.
 * A in {2, 3, 4, 7, 8, 10, 11}. */
int32_t mppi_philox_words(int32_t A);
mppi_status mppi_philox_normals(uint64_t seed, uint32_t step, int32_t vehicle, int64_t k0, int32_t K,
                                int32_t H, int32_t A, int32_t device, float* z, uint32_t* raw);

/* ---------------------------------------------------------------------------------------
 * Host rigid-body dynamics of the arm node.  The reference node
 * calls pin.computeAllTerms(model, data, q, v) on the free-flyer model of
 * full_robot_floating2.urdf every tick (kinova.py:54-61, 126) and applies
 *     tau = M[6:,6:] (400 (qdes - q[7:]) - 40 v[6:]) + nle[6:]              (kinova.py:184)
 * These replace those Pinocchio calls (double precision, Pinocchio's conventions: q = base
 * xyz + quaternion xyzw + joints, v = base linear + angular velocity in the base frame +
 * joint rates, gravity (0,0,-g)).  Fixed-joint links are merged into their movable
 * ancestor.  K = 1 per tick: host code, no GPU. */
typedef struct {
    int32_t parent;        /* index of the parent link entry, -1 = the world                  */
    int32_t type;          /* joint attaching this link: MPPI_JOINT_FIXED / REVOLUTE /
                            * PRISMATIC / FLOATING (root only)                                 */
    double xyz[3], rpy[3]; /* joint origin in the parent link frame (URDF <origin>)           */
    double axis[3];        /* joint axis in the joint frame (URDF <axis>)                     */
    double mass;           /* URDF <inertial>: mass, COM in the link frame, inertia about the */
    double com[3];         /*   COM in the link frame (row-major 3x3; the <inertial> origin    */
    double inertia[9];     /*   rotation already applied)                                     */
} mppi_link;

typedef struct mppi_dyn mppi_dyn;

/* Build the model from links in topological order (robot/urdf_tree.py writes them). */
mppi_status mppi_dyn_create(const mppi_link* links, int32_t n_links, double gravity, mppi_dyn** out);
void mppi_dyn_destroy(mppi_dyn* d);
void mppi_dyn_dims(const mppi_dyn* d, int32_t* nq, int32_t* nv, int32_t* n_bodies);
/* Inverse dynamics tau = M(q) a + nle(q, v) (a NULL = 0), recursive Newton-Euler. */
mppi_status mppi_dyn_rnea(mppi_dyn* d, const double* q, const double* v, const double* a, double* tau);
/* pin.computeAllTerms' M (nv x nv, row-major) and nle = C(q,v) v + g(q) (nv); either may be NULL. */
mppi_status mppi_dyn_terms(mppi_dyn* d, const double* q, const double* v, double* M, double* nle);
/* kinova.py:184 for the trailing actuated joints (rows first_v..nv-1):
 * tau = M[first_v:, first_v:] (kp (qdes - q_act) - kd v_act) + nle[first_v:], as ONE RNEA
 * pass with a = (0, ades) (the base-acceleration columns of M are multiplied by 0). */
mppi_status mppi_computed_torque(mppi_dyn* d, const double* q, const double* v, const double* qdes, double kp,
                                 double kd, int32_t first_v, double* tau);

#ifdef __cplusplus
}
#endif
#endif /* MPPI_HIP_H */
