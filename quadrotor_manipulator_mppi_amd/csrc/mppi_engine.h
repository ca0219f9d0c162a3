// mppi_engine.h -- the engine object behind include/mppi_hip.h and the host-side helpers its
// translation units share.  Internal: not part of the public ABI.
//
// The host side of libmppi_hip.so is split by concern:
//   mppi_host_math.cpp   error state, config defaults and validation, the reference's fp32 tensor
//                        builders (joint origins, base and target rotations), SavGol taps, host FK
//   mppi_layout.cpp      layout_of: what create derives from a configuration without a device -- sizes,
//                        launch geometry, Sigma^-1, the baked chain, the kernels' parameter structs
//                        (mppi_layout.h; no HIP, so it runs and is tested without a GPU)
//   mppi_engine.cpp      create (allocate, bind, upload) / destroy, the finalize tails, state and
//                        target uploads, readbacks, timing
//   mppi_launches.cpp    the launch-parameter builders (rollout_params, finalize_params: every
//                        launch's DevParams / FinParams and the quiet rule), launches described
//                        instead of made, the native paths' description cache (DescCache)
//   mppi_step.cpp        the control step: rollout, finalize, outputs, native (AQL) batches and calls
//   mppi_debug.cpp       the diagnostics entry points (mppi_debug_*: described launches, stamps, the
//                        native queue's probes), none of them on the step's path
//   mppi_exchange.cpp    the sharded step's exchanges: the engine-owned RCCL communicator and the
//                        peer exchange (regions, connect, probe, status, reset)
//   mppi_prewarm.cpp     the opt-in prewarm thread (mppi_set_prewarm)
//
// Threads.  Every entry point of one engine is called from one thread at a time (the Python
// wrapper serialises them), except the prewarm thread, which reads only the atomics marked for it
// below (call_t, call_n, pw_*) and e->aql once pw_native has been stored with release after it.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "mppi_aql.h"
#include "mppi_layout.h"

// Whose completion the pending outputs wait for: nothing to read; a HIP-launched read step (its
// tagged records, ev_out as the backstop); a native batch (its completion signal); a native
// control call (its records, tagged with a bit-31 sequence number).
enum class Pending { None, Hip, Batch, Call };

// A native path's launch descriptions and the parameters they were made from.  The capture formats
// both kernels' symbol names and packs ~2 KB of arguments (~0.4 us), so a batch or a control call
// reuses them while its parameters match.  roll_quiet and fin_quiet are the launches of a batch's
// steps before its last (the same descriptions as roll and fin where no quiet kernel applies); a
// control call has none.
struct DescCache {
    bool valid = false;
    int threads = 0;
    mppi::DevParams p{};
    mppi::FinParams f{};
    mppi::LaunchDesc roll{}, fin{}, roll_quiet{}, fin_quiet{};
    const float* ttab = nullptr;   // a tracking engine's target table (its rollouts' extra argument; fixed per engine)
    float* scene = nullptr;        // a scene engine's buffer (likewise)
    const float* field = nullptr;  // a field engine's field buffer (likewise)
    int self_members = -1;         // a self engine's paired spheres (likewise; -1: not one)
    const float* limits = nullptr; // a bounded engine's limits buffer (likewise)
    // ignore_vc0: the vehicle constants (the state) may differ -- a control call patches them in
    bool matches(const mppi::DevParams& p, const mppi::FinParams& f, int threads, bool ignore_vc0) const;
    // describes (p, f) and, where given, the quiet pair; the launchers' status (0: valid again)
    int refresh(const mppi::DevParams& p, const mppi::FinParams& f, int threads,
                const mppi::DevParams* p_quiet = nullptr, const mppi::FinParams* f_quiet = nullptr);
};
// The rollout's last argument is its DevParams by value: where the vehicle constants, and the
// sequence word in them (VehicleConst::_pad[0], kSeqFromVc), lie in a description's argument block.
inline uint32_t roll_vc0_off(const mppi::LaunchDesc& roll) {
    return roll.arg_bytes - (uint32_t)sizeof(mppi::DevParams) + (uint32_t)offsetof(mppi::DevParams, vc0);
}
inline uint32_t roll_seq_off(const mppi::LaunchDesc& roll) {
    return roll_vc0_off(roll) + (uint32_t)offsetof(mppi::VehicleConst, _pad);
}

// The layout (cfg, the sizes, dp, fp, ...: mppi_layout.h) and the device state built on it.
struct mppi_engine : mppi_host::EngineLayout {
    hipStream_t own_stream = nullptr, stream = nullptr;
    float* d_sigma = nullptr;
    mppi::JointDev* d_joints = nullptr;
    mppi::VehicleConst* d_vc = nullptr;
    float* d_u_prev = nullptr;
    float* d_noise_in = nullptr;
    uint32_t step_ctr = 0;              // Philox counter word; +1 per finalized step
    uint32_t out_seq = 0;               // completion-flag value of the step read_outputs waits for
    // the native paths' launch descriptions (DescCache): a batch's, reused while the step's parameters
    // are unchanged, and a control call's, reused while only the state changes
    DescCache batch, call;
    // the kernels the last batch and the last control call ran (mppi_kernel_info)
    std::string kern_batch = "none", kern_call = "none";
    int kern_batch_state = 0;           // kern_batch describes the resident native batch: 1 one step, 2 several
    bool kern_call_hip = false, kern_call_peer = false;   // kern_call describes the HIP-launched call (as of peer)
    std::vector<double> rec_out;        // a read step's outputs assembled from its tagged records
    std::vector<float> rec_u0, rec_stats;
    std::vector<float> fk_O, fk_ax;     // the joints' origins and unit axes for check_reach's host FK
    uint32_t seq_ctr = 0;               // last completion-flag value handed out: monotonic and
                                        // independent of step_ctr (mppi_set_step_counter rewinds that)
    bool event_wait = false;            // MPPI_EVENT_WAIT=1: wait on ev_out instead of polling flags
    bool no_flag_dbg = false;           // MPPI_DEBUG_NO_FLAG=1 (diagnostics, with MPPI_EVENT_WAIT=1): no step
                                        // writes the completion flag, so the last step runs like the others
    int out_dbg = 0;                    // MPPI_DEBUG_OUT (diagnostics): 1 = unread steps write their outputs
                                        // to device scratch, 2 = mppi_kernel_timing writes to mapped host memory
    float* d_traj = nullptr;
    float* d_noise_out = nullptr;
    float* d_S = nullptr;
    float* d_hdr = nullptr;     // (V,nb,4) block record headers
    float* d_rdata = nullptr;   // (V,A,nb,H) block record bodies
    unsigned char* d_out = nullptr;   // device scratch in h_out's layout (mppi_kernel_timing's outputs)
    mppi::FinTail* d_tail = nullptr;  // [kTailSlots] the finalize's tail parameters per launch kind
    float* d_wraw = nullptr;
    float* d_wsmooth = nullptr;
    float* d_w = nullptr;
    float* d_sinv = nullptr;      // extra cost terms: Sigma^-1 (A,A)
    float* d_gamma = nullptr;     //   gamma^t (H)
    float* d_jtraj = nullptr;     //   joint tracking target (V,H,nq)
    // the target table of a tracking engine (cost_terms & MPPI_COST_TARGET_TRACK; else none): (V,H,12)
    // rows p*(3), R*(9) on the device; its pinned host copy, the uploads' staging (what the device
    // holds or is about to: check_reach reads row 0), ev_tt recorded behind the last upload; and per
    // vehicle whether a table is set (clear: every row is the fixed target, mppi_set_target refills them)
    float* d_ttab = nullptr;
    float* h_ttab = nullptr;
    hipEvent_t ev_tt = nullptr;
    bool tt_pending = false;
    std::vector<unsigned char> ttab_set;
    // the scene of an obstacle-avoiding engine (mppi_create_scene; else none): the device buffer
    // (mppi_obstacles.h: body table, the vehicles' obstacle blocks, the clearances), the pinned staging
    // copy of the obstacle blocks (V, kSceneObsW) and the event recorded behind the last upload.  Such an
    // engine always owns a target table (d_ttab; clear without the tracking bit).
    float* d_scene = nullptr;
    float* h_scene = nullptr;
    hipEvent_t ev_scene = nullptr;
    bool scene_pending = false;
    // the distance field of a field engine (mppi_create_scene_field; else none; such an engine has a scene):
    // the device buffer (mppi_field.h: header, cells), its pinned staging copy of the same size, both
    // allocated at creation, and the event recorded behind the last upload
    float* d_field = nullptr;
    float* h_field = nullptr;
    hipEvent_t ev_field = nullptr;
    bool field_pending = false;
    // the rotor limits of a bounded engine (mppi_create_limits; else none): the device buffer (mppi_limits.h: lo[4],
    // hi[4]) the bounded kernels reach through a pointer fixed at creation, its pinned staging copy and the event
    // recorded behind the last upload (EngineLayout::limits: the bounds as last set)
    float* d_limits = nullptr;
    float* h_limits = nullptr;
    hipEvent_t ev_limits = nullptr;
    bool limits_pending = false;
    std::vector<float> lim_u0;          // mppi_read_outputs: the step's u0 with its rotor dims clamped
    // mppi_set_occupancy's device scratch (allocated at its first call, for the field's dims: the two
    // int32 grids of the transform, then the occupancy bytes; mppi_edt.h edt_scratch_bytes)
    void* d_edt = nullptr;
    // mppi_integrate_depth's image: pinned staging and its device twin, MPPI_DEPTH_MAX_PIXELS floats each,
    // allocated at its first call (ev_field guards the staging copy, as it does h_field)
    float* h_depth = nullptr;
    float* d_depth = nullptr;
    float* d_exchange = nullptr;
    // mppi_get_plan's buffers (allocated at its first call): the host's vehicle constants; the
    // planes (V,C,H), cost_t (V,H), pos_err (V,H) and S (V) in one block, and its pinned host copy
    mppi::VehicleConst* d_plan_vc = nullptr;
    float* d_plan = nullptr;
    float* h_plan = nullptr;
    // mppi_get_elites' buffers (allocated at its first call, for MPPI_MAX_ELITES): stage A's candidate
    // keys (V,B,64); the output block idx, S, w (V,n each) and rows (V,n,H,Cr; with store_trajectory),
    // contiguous for the n of the call, and its pinned host copy
    unsigned long long* d_elite_cand = nullptr;
    float* d_elites = nullptr;
    float* h_elites = nullptr;
    ncclComm_t comm = nullptr;          // engine-owned RCCL communicator (mppi_comm_init)
    float* d_xown = nullptr;            // its exchange buffer (shard_count * V * P floats)
    bool peer = false;                  // peer exchange connected (mppi_peer_connect): no PACK, no collective
    int x_connected = 0;                // ranks whose word the kernel probe received (mppi_peer_probe phase 2)
    unsigned long long* d_xregion = nullptr;   // this rank's exchange region (uncached device memory)
    size_t x_bytes = 0;
    std::vector<void*> x_opened;        // the other ranks' regions, IPC-mapped
    unsigned long long** d_xpeers = nullptr;   // (shard_count) region pointers, device resident
    uint32_t x_epoch = 0;               // the exchange epoch in the tags (mppi_dev.h peer_tag): moved by
                                        // mppi_set_step_counter and mppi_peer_reset on a connected engine
    uint32_t* d_xstall = nullptr;       // diagnostics (mppi_debug_peer_stall): a finalize block's stall
    unsigned long long* d_xdec = nullptr;   // the peer exchange's commit marks (2 parities x finalize blocks)
    bool overlap = false;               // MPPI_OVERLAP=1 (experiment): native batches dispatch each rollout
                                        // while the finalize before it runs (mppi_device.h kNoiseOverlap)
    uint32_t* d_ovl = nullptr;          // its (V, A, fin_ts) step counters, one per finalize block
    mppi::VehicleConst* h_vc = nullptr; // pinned staging
    unsigned char* h_out = nullptr;     // pinned + mapped: k_finalize writes it directly
    unsigned char* h_out_dev = nullptr; // device view of h_out
    hipEvent_t ev_vc = nullptr, ev_out = nullptr;
    bool vc_pending = false, state_set = false;
    Pending pending = Pending::None;    // the finalised step mppi_read_outputs may read
    std::vector<float> tpos, tquat;
    std::vector<double> state;
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> roll_pairs, fin_pairs;
    double roll_ms = 0.0, fin_ms = 0.0;
    unsigned long long* d_stamps = nullptr;    // MPPI_STAMPS diagnostics
    unsigned long long* d_fstamps = nullptr;
    std::vector<double> fstamp_sum;
    int64_t fstamp_n = 0;
    std::vector<double> stamp_sum;
    int64_t stamp_n = 0;
    double clk_sum = 0.0;
    int64_t roll_n = 0, fin_n = 0;
    // native dispatch of mppi_run_steps (mppi_aql.cpp): MPPI_DISPATCH = hip | aql | auto (default)
    mppi_aql::Step* aql = nullptr;
    int aql_mode = 2;                   // 0 hip, 1 aql (required), 2 auto (aql when available)
    bool aql_tried = false;             // step_create attempted (its failure is final for the engine)
    bool aql_off = false;               // this engine's launches are not dispatchable natively
    std::string aql_why = "no mppi_run_steps yet";   // why the last run went through HIP ("" = native)
    bool calls_native = false;          // the last mppi_step went out as native packets
    double call_wait_us = 0.0;          // diagnostics (MPPI_AQL_PROFILE): the last call's flag wait
    // prewarm (mppi_set_prewarm, mppi_prewarm.cpp): a host thread learns the control calls' cadence
    // from their start times and touches the native queue through a window before each predicted call
    std::thread pw_thr;
    std::mutex pw_mu;                   // (for pw_cv only)
    std::condition_variable pw_cv;
    std::atomic<int32_t> pw_us{0};      // the window half-width; 0: off
    std::atomic<bool> pw_stop{false};
    std::atomic<int64_t> pw_touches{0};
    std::atomic<int64_t> call_t[8];     // steady-clock start of the last 8 control calls (ring)
    std::atomic<int64_t> call_n{0};     // control calls recorded
    bool pw_spin = false;               // diagnostics (MPPI_PREWARM_SPIN=1): spin between touches
    std::atomic<bool> pw_native{false}; // the last control call went out as native packets (release:
                                        // stored after e->aql, so the prewarm thread may read it)
};

namespace mppi_host {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return ::mppi_host::fail(MPPI_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                \
                                     hipGetErrorString(_e), __FILE__, __LINE__);                   \
    } while (0)

// ------------------------------------------------------------ engine (mppi_engine.cpp)
// the step goes through the exchange slots: several shards, or an engine-owned communicator (a
// one-rank communicator runs the same pack -> all-reduce -> combine).  A shard connected by the
// peer exchange steps like an unsharded engine: its finalize does the exchange.
inline bool sharded(const mppi_engine* e) { return (e->cfg.shard_count > 1 || e->comm) && !e->peer; }
void pack_fields(const mppi_engine* e, mppi::FinParams& f);
// out, u0, stats and flags of a FinParams or FinTail over an output buffer in h_out's layout
template <class X>
inline void bind_outputs(X& x, unsigned char* base, const mppi_engine* e) {
    x.out = (double*)base;
    x.u0 = (float*)(base + off_u0(e));
    x.stats = (float*)(base + off_stats(e));
    x.flags = (uint32_t*)(base + off_flags(e));
}
// The finalize's tail parameters, one device copy per launch kind (d_tail[kTailSlots]); each kind
// is derived from e->fp as it stands, and written again when a member it carries changes.
struct Tails { mppi::FinTail t[mppi::kTailSlots]; };
Tails tails_of(const mppi_engine* e);
// synchronises the engine's stream, then copies the given kinds' tails (a bit per kTail* slot)
mppi_status upload_tails(mppi_engine* e, unsigned slots);
inline mppi_status upload_pack_tail(mppi_engine* e) { return upload_tails(e, 1u << mppi::kTailPack); }
// async copy to the host on the engine's stream, then synchronise
mppi_status download(mppi_engine* e, void* dst, const void* src, size_t bytes);
mppi_status aql_join(mppi_engine* e);
mppi_status use_device(mppi_engine* e);
mppi_status build_vehicle_consts(mppi_engine* e);
void quad_outputs(const mppi_engine* e, const double* s, const float* u0, double* out);
void aerial_outputs(const mppi_engine* e, const double* s, const float* u0, double* out);
mppi_status upload_consts(mppi_engine* e);
// A tracking engine's table, as upload_consts moves the V > 1 vehicle constants: target_rows_begin
// waits until the last copy out of the staging rows has run (they may then be rewritten),
// target_rows_fixed sets vehicle v's staging rows to its fixed target, upload_target_rows copies them
// to the device on the engine's stream (ordered before the next step on both dispatch paths: a HIP
// launch follows it on the stream, a native submission drains the stream first).
mppi_status target_rows_begin(mppi_engine* e);
void target_rows_fixed(mppi_engine* e, int v);
mppi_status upload_target_rows(mppi_engine* e, int v);
hipEvent_t pool_event(mppi_engine* e);
mppi_status drain_timing(mppi_engine* e);

inline uint32_t sticky_timeout(const mppi_engine* e) {
    return e->h_out ? *(const volatile uint32_t*)(e->h_out + off_xerr(e)) : 0u;
}
// this rank's exchange region past its control words (mppi_dev.h kXCtl): the partials' base
inline unsigned long long* xdata(const mppi_engine* e) { return e->d_xregion + mppi::kXCtl; }

// ------------------------------------------------------ launches (mppi_launches.cpp)
// The launch-parameter builders: every launch of the step's kernels takes its parameters from these
// two.  What a single launch owns -- the HIP launches' step counter and fresh sequence number, the
// MPPI_DEBUG_OUT tails, a batch's kNoiseOverlap -- its call site sets on what they return.
// Hip: the HIP launches'.  Batch, Call: a native batch's or control call's description -- the step
// counter relative to the dispatch id (kNoiseStepFromId; set by step_prepare / step_call),
// completion by the batch's signal or by the flags whose sequence number rides in the vehicle
// constants (kSeqFromVc).
enum class StepPath { Hip, Batch, Call };
// FINAL: the step's finalize.  PACK: a shard's block records folded into its exchange slot.
// SCRATCH: a FINAL into device scratch (the mapped buffer's layout; the SCRATCH tail) with no
// completion flag, so a pending read_outputs / get_weighted_noise still returns the last real step
// (on a shard it combines the exchange slots as they stand; xerr stays at the mapped buffer).
// READBACK: w_eps and its SavGol of the records the last step combined.
enum class FinKind { Final, Pack, Scratch, Readback };
// quiet: a step of a batch before its last (never read) asks for the quiet kernels and gets the full
// parameters back where none applies, so "no quiet kernel" shows as the same symbol.
mppi::DevParams rollout_params(const mppi_engine* e, StepPath path, const float* d_noise, bool quiet);
mppi::FinParams finalize_params(const mppi_engine* e, FinKind kind, StepPath path = StepPath::Hip, bool quiet = false);
// The quiet rule, on the switches as values (the builders; the engine-less mppi_debug_*_kernels).
// A batch's steps before its last may run the quiet FINAL (mppi_finalize.hip kRoleQuiet: u_prev and
// nothing else; the outputs of a batch are those of its last step).  diag: an engine with stamps,
// timing or output diagnostics or the overlap experiment; it and MPPI_GENERIC_KERNELS (generic & 3)
// keep the full kernel on every step; so does the launcher where no quiet kernel applies (the
// geometry, a peer exchange).
inline int32_t quiet_fin_kern(int32_t kern, int generic, bool diag) {
    return (generic & 3) || diag ? kern : kern | mppi::kFinKernQuiet;
}
// Those steps' rollouts likewise run the quiet rollout (mppi_rollout.h rollout_body QUIET: the
// records and nothing else), so a batch's trajectory planes, costs and handed-over vehicle
// constants are its last step's.  Not on a peer engine (the exchange's tag rides in the handed-over
// step word every step) or a shard (its PACK and collective are left as they are); the launcher
// keeps the full kernel where no quiet one applies (stored or injected noise, the extended kernels,
// other geometries).
inline int32_t quiet_roll_kern(int32_t kern, int generic, bool diag, bool peer, bool shard) {
    return (generic & 11) || diag || peer || shard ? kern : kern | mppi::kRollKernQuiet;
}
// a launch described into d instead of made (mppi_device.h go(); the launchers' status)
// The rollout's launch: the tracking kernels (cost_terms & MPPI_COST_TARGET_TRACK) take the engine's
// target table as an extra argument; every other launch is mppi_launch_rollout's.
// A scene engine's (scene non-null) run the scene kernels, with or without the tracking bit.
// A field engine's (field non-null, with its scene) run the field kernels.
// A bounded engine's (limits non-null: its limits buffer; QUADROTOR and AERIAL, never a scene engine) run the
// bounded kernels, QUADROTOR's with or without the tracking bit.
inline int launch_rollout(const mppi::DevParams& p, const float* ttab, int threads, void* stream, float* scene = nullptr,
                          const float* field = nullptr, int self_members = -1, const float* limits = nullptr) {
    if (limits) {
        if (p.model == MPPI_MODEL_QUADROTOR)
            return mppi_launch_rollout_quad_b(&p, (p.cost_terms & MPPI_COST_TARGET_TRACK) ? ttab : nullptr, limits, threads, stream);
        return p.model == MPPI_MODEL_AERIAL ? mppi_launch_rollout_aerial_b(&p, limits, threads, stream) : -1;
    }
    // a self engine's (self_members >= 0: the spheres that appear in a pair; with its scene) run the self kernels
    if (self_members >= 0) return mppi_launch_rollout_self(&p, ttab, scene, field, self_members, threads, stream);
    if (field) return mppi_launch_rollout_field(&p, ttab, scene, field, threads, stream);
    if (scene) return mppi_launch_rollout_scene(&p, ttab, scene, threads, stream);
    return (p.cost_terms & MPPI_COST_TARGET_TRACK) ? mppi_launch_rollout_track(&p, ttab, threads, stream)
                                                   : mppi_launch_rollout(&p, threads, stream);
}
int describe(const mppi::DevParams& p, int threads, mppi::LaunchDesc* d, const float* ttab = nullptr, float* scene = nullptr,
             const float* field = nullptr, int self_members = -1, const float* limits = nullptr);
int describe(const mppi::FinParams& f, mppi::LaunchDesc* d);
// -------------------------------------------------------------- step (mppi_step.cpp)
// why this engine's steps cannot go native (nullptr: they can).  A batch may carry the stamps /
// no-flag diagnostics natively (the timeline build measures the native step that way); a control
// call waits on the flags, so it may not.
const char* aql_ineligible(const mppi_engine* e, bool batch = false);

// ------------------------------------------------------- diagnostics (mppi_debug.cpp)
// the symbol a launch would run, by the launchers' own description of it ("?": none)
std::string fin_symbol(const mppi::FinParams& f, mppi::LaunchDesc* desc = nullptr);
std::string roll_symbol(const mppi::DevParams& p, int threads, mppi::LaunchDesc* desc = nullptr, const float* ttab = nullptr,
                        float* scene = nullptr, const float* field = nullptr, int self_members = -1, const float* limits = nullptr);

// ------------------------------------------------------ exchange (mppi_exchange.cpp)
// RCCL, resolved at the first mppi_comm_* call (dlopen: the library loads and its single-GPU
// paths run without RCCL; inside a torch process this binds the librccl.so.1 torch already
// loaded, so there is one RCCL per process).
struct Rccl {
    bool ok = false;
    std::string why;
    ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
    ncclResult_t (*init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*all_reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                               hipStream_t) = nullptr;
    ncclResult_t (*destroy)(ncclComm_t) = nullptr;
    const char* (*err)(ncclResult_t) = nullptr;
    // the non-blocking init with a deadline (mppi_comm_init_ex) and the communicator's own
    // view of its size (mppi_comm_info)
    ncclResult_t (*init_rank_config)(ncclComm_t*, int, ncclUniqueId, int, ncclConfig_t*) = nullptr;
    ncclResult_t (*async_error)(ncclComm_t, ncclResult_t*) = nullptr;
    ncclResult_t (*abort)(ncclComm_t) = nullptr;
    ncclResult_t (*count)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*user_rank)(const ncclComm_t, int*) = nullptr;
};
const Rccl& rccl();
// the engine's exchange resources (communicator, mapped peer regions), released by mppi_destroy
void exchange_release(mppi_engine* e);

// ------------------------------------------------------- prewarm (mppi_prewarm.cpp)
void note_call(mppi_engine* e);      // mppi_step entry (the caller's thread)
void prewarm_stop(mppi_engine* e);   // joins the thread (mppi_destroy, mppi_set_prewarm)
int prewarm_plan(const int64_t* t, int m, int64_t win, int64_t* start, int64_t* end);

// MPPI_STAMPS diagnostics: stamp indices in program order and the phase each difference measures
// (see the STAMP calls in mppi_rollout.h / mppi_finalize.hip).
inline const std::vector<int> kRollStampOrder = {0, 9, 10, 8, 1, 2, 3, 4, 5, 11, 6, 12, 7};
inline const char* const kRollStampNames[] = {"", "loads(waited)", "philox0", "lds-writes(waited)", "barrier",
                                              "noise", "integrator", "fk+cost", "S+softmin", "deposit",
                                              "combine-barrier", "fw", "record"};
inline const std::vector<int> kFinStampOrder = {0, 7, 8, 1, 2, 3, 4, 5, 6};
inline const char* const kFinStampNames[] = {"", "loads-issued", "accum(last chunk)", "wave-fold", "barrier",
                                             "combine", "w_eps", "savgol", "update+outputs"};

}  // namespace mppi_host
