// mppi_rollout.h -- gfx950 (CDNA4) rollout kernel of the MPPI control step (the
// template; instantiated per model in mppi_rollout_{drone,arm,arm_h32,arm32,wb}.hip so the
// translation units compile in parallel, through the launchers of mppi_rollout_launch.h).
// The pieces the body is made of: mppi_noise.h (Philox, Box-Muller), mppi_integrator.h,
// mppi_fk.h (FK chain, pose cost), mppi_stores.h, mppi_diag.h (knockouts, stamps, sections).
//
//   k_rollout   one launch per step: noise draw -> double-integrator rollout ->
//               FK chain -> per-rollout cost -> online-softmin partials.
//               Replaces standard_normal_noise.py:22-50, urdf_fk.py:79-108,
//               urdfparser.py:122-163, pose_cost.py:24-63 (arm) and
//               drone_mppi.py:40-107 (drone), mppi.py:184-188 (softmin).
//   (k_finalize, the second launch of a step, is in mppi_finalize.hip.)
//
// Lane mapping: a wave64 holds R = 64/L rollouts, one
// L-lane segment each, lane = timestep t (L = pow2 >= H, 16..64; H > 64 runs
// ceil(H/64) chunks per lane).  The two cumsums of the integrator run in a
// transposed lane map through the wave's LDS slot (integrate_lds; DPP segment scans
// for H > 64); the FK chain, cost and softmin are lane-local; S_k is a segment
// reduction.
// Trajectories are stored as SoA planes (V,C,K,H): every store instruction of a
// wave writes 64 consecutive floats (256 B).
#pragma once
#include "mppi_device.h"
#include "mppi_diag.h"
#include "mppi_noise.h"
#include "mppi_fk.h"
#include "mppi_stores.h"
#include "mppi_integrator.h"
#include "mppi_obstacles.h"
#include "mppi_field.h"
#include "mppi_self.h"

// The leading scalar arguments are preloaded into SGPRs at wave launch on gfx950
// (-mllvm -amdgpu-kernarg-preload-count, build.py): the first group's Philox
// draw and the u_prev / joint-table loads start without waiting for the
// kernel-argument segment (its first s_load costs ~1.5k cycles).
// ONEG: every wave runs exactly one rollout group (iters == 1).  Straight-line code with
// no loop-carried softmin state: the common whole-body kernel fits in 52 VGPRs, so it is
// budgeted for 8 waves per SIMD (the looping variant needs 87: 5 waves; the fp64-state
// arm kernel would spill at 64 and keeps the 4-wave budget -- C3 runs 2 waves per SIMD).  At the C4 shard
// (whole-body K=8192 H=64) that is 1024 blocks x 8 waves, all resident at once: twice the
// latency hiding of 512 blocks x 2 groups, and no wave left alone in the grid's tail.
// B512 (k_rollout_s, ONEG only): the block is 512 threads and the launch is a plain one (no overlap
// wait), both known at compile time: one u_prev load per 512 warm-start words the shape can have
// instead of four, one joint-table load instead of two, and the loops that only a smaller block or
// a longer warm start needs (the staging tails, the absent waves' fill) and the overlap poll are
// not in the instantiation.  The launcher picks it when all of that holds (launch_rollout_x).
//
// roll_occ: waves per SIMD the rollout kernel is register-budgeted for (4: <= 128 VGPRs).
// NCH == 4 (H in 193..256) is budgeted for 2 waves (<= 256 VGPRs): at 4 it spilled
// 0.3-2 KB per lane and ran 2.3x slower (arm K=4096 H=256 40.7 -> 28.1 us, whole-body
// 81.8 -> 35.3 us); NCH == 2 keeps 4 (its 8-96 B spill is cheaper than 3 or 2 waves:
// arm H=128 13.6 us at 4, 16.7 at 3 and 2; profiles/r02/ab_rollout_occupancy_long_h.txt).
// The extended (XC) NCH == 2 kernels likewise run best at 2 (whole-body K=8192 H=128 full
// Sigma 72.1 -> 43.6 us, arm 21.8 -> 19.3); XC NCH == 1 keeps 4 (2 and 3 measured slower;
// profiles/r02/ab_rollout_occupancy_xc.txt)
// the scene body's accumulators (a hinge or cost sum, a min clearance); nothing in the other bodies
// A kernel-argument float read where it is used (the self bodies' cost-term weights): the address depends on an
// opaque zero, so the load is not hoisted to the prologue and merged with its neighbours into one 16 B load.  That
// load lived to the end of the kernel; the scalar allocator gave it a stack slot, then rematerialised every use,
// and the unused slot stayed in the kernel's private segment (20 B with the scavenging word, no instruction
// addressing it) in the one-vehicle forms.
__device__ __forceinline__ float late_arg(const float& x) {
    int z = 0;
    asm volatile("" : "+s"(z));
    return (&x)[z];
}
template <bool OBS> struct ObsAcc {};
template <> struct ObsAcc<true> { float sum = 0.0f, gmin = INFINITY; };
// the self body's: those, and the self-collision pairs' hinge or cost sum and min clearance.  One object with the
// scene's, not a second one: a further (empty) accumulator in the other bodies moved registers in kernels this
// header also builds for the drone.
struct SelfAcc : ObsAcc<true> { float ssum = 0.0f, sgmin = INFINITY; };
template <bool OBS, bool SLF> using RollAcc = std::conditional_t<SLF, SelfAcc, ObsAcc<OBS>>;
template <int NCH, bool F64, bool XC, bool ONEG>
constexpr int roll_occ() {
    return (ONEG && !F64) ? 8 : (NCH >= 4 ? 2 : NCH == 2 ? (XC ? 2 : 4) : 4);
}
// QUIET (k_rollout_q, k_rollout_ql): the rollout of a batch's step before its last (mppi_step.cpp
// quiet_rollout): nothing reads that step's trajectory planes, costs S, stored noise or handed-over
// vehicle constants before the next step overwrites them (the quiet FINAL after it reads only the
// records), so the instantiation has none of those stores, nor the plane descriptor, the S staging
// in LDS or block 0's hand-off.  Everything the records are made of is the same code in the same
// order: the records are bit-identical to the full kernel's.
// TRK (k_rollout_tt; MPPI_COST_TARGET_TRACK): the pose target moves along the horizon.  The lane's
// step(s) t are fixed for the block's lifetime, so it fetches its row(s) of the target table
// (V, H, 12), one per 64-lane chunk, once, with the prologue's other global loads, and the pose cost
// (the drone branch: the position cost) takes p*_t and R*_t from those registers instead of the
// vehicle constants.  An extended (XC) body: extra terms, a full Sigma and generic chains go with it.
// OBS (k_rollout_ob; mppi_create_scene): the sphere scene's term (mppi_obstacles.h).  A tracking (TRK)
// body -- a scene engine always owns a target table -- whose block stages the engine's body table and
// the vehicle's obstacle rows in static LDS with the prologue's other loads; as each frame of the FK
// chain completes, the lane runs that frame's spheres against the obstacles at its own row time
// (wave-uniform LDS reads), and the step's term joins the extra terms' segment sums.  The per-sample
// clearance, a segment min, is staged and written through beside S (into the scene buffer).
// FLD (k_rollout_df; mppi_create_scene_field): a scene (OBS) body with the engine's distance field
// (mppi_field.h) as one more obstacle.  The field's header rides in LDS behind the staged scene; per body
// sphere the lane samples the field at the centre it has just formed (four 8 B loads of x-pairs; the
// lanes of a segment are consecutive t of one sample, so neighbouring centres share lines) and feeds
// g = d(c) - r_b into the same hinge sum and min.  A field not set is a wave-uniform skip.
// SLF (k_rollout_sc, with FLD k_rollout_sf; mppi_create_scene_self): a scene body with the self-collision
// pairs (mppi_self.h).  The pair tables ride in static LDS beside the scene; the chain walk stores the
// centre of every sphere that appears in a pair into the lane's own LDS column (behind the staged runs:
// 3 * members words per thread, no barrier), and after the chain of a (k, t) a wave-uniform loop over the
// pairs forms the step's second hinge sum and min.  That term joins S after the obstacle term, and the
// per-sample self clearance goes out as the clearance does, a third staged run.  ARM and WHOLEBODY, blocks
// of at most 256 threads (launch_rollout_self sizes the LDS).
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool VONE, bool XC, bool ONEG, bool B512, bool QUIET = false,
          bool TRK = false, bool OBS = false, bool FLD = false, bool SLF = false>
__device__ __forceinline__ void rollout_body(const uint32_t seed_lo, const uint32_t seed_hi,
                                             const uint32_t step_arg, const uint32_t k_off,
                                             const int32_t noise_arg, const int32_t H_arg,
                                             const int32_t geo_arg,
                                             const float* __restrict__ u_prev,
                                             const JointDev* __restrict__ jtab, const DevParams& pk,
                                             const float* __restrict__ ttab = nullptr,
                                             float* __restrict__ scene = nullptr,
                                             const float* __restrict__ field = nullptr) {
    static_assert(!B512 || ONEG, "the fixed-block body is a single-group one");
    static_assert(!FLD || OBS, "the field body is a scene one");
    static_assert(!SLF || (OBS && MODEL != MPPI_MODEL_DRONE), "the self body is a scene one of a model with a chain");
    static_assert(!OBS || (TRK && !B512), "the scene body is a tracking one of every block size");
    static_assert(!TRK || (XC && !QUIET), "the tracking body is an extended one, and has no quiet form");
    static_assert(!QUIET || (!XC && NCH == 1), "the quiet body exists for the common one-chunk kernels");
    constexpr bool kTraj = !QUIET && !(MPPI_KO & 16);      // trajectory planes
    constexpr bool kCosts = !QUIET && !(MPPI_KO & 1024);   // the cost vector S
    constexpr bool kHand = !QUIET && !(MPPI_KO & 2048);    // block 0's vehicle-constant hand-off
    // eta^2 (the outputs' effective sample size).  The quiet body forms none: the quiet FINAL, the only
    // reader of a quiet step's records, turns eta^2 into nothing (mppi_finalize.hip: the effective sample
    // size of the outputs section alone), so the header's third word is written as 0.
    constexpr bool kEta2 = !QUIET;
    constexpr int R = 64 / LSEG;
    constexpr int QOFF = (MODEL == MPPI_MODEL_WHOLEBODY) ? 3 : 0;
    constexpr int NQ = (MODEL == MPPI_MODEL_DRONE) ? 0 : NA - QOFF;
    constexpr int kJW = (int)(sizeof(JointDev) * kMaxJ / 4);   // joint table, dwords
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // Scalars and (V == 1) the vehicle constants are read from the kernel
    // arguments with scalar loads (SGPR operands, no LDS latency in the hot
    // phases); the joint table and (V > 1) the vehicle block go to LDS.
    __shared__ JointDev jnt[kMaxJ];
    __shared__ VehicleConst vcv;
    __shared__ __attribute__((aligned(16))) float scn[OBS ? kSceneLdsW + (FLD ? kFieldHdrW : 0) : 4];   // OBS: the body table, then the vehicle's obstacles (FLD: then the field's header)
    __shared__ __attribute__((aligned(16))) float slf[SLF ? kSelfHdrW : 4];   // SLF: the pair region's header and tables
    const DevParams& p = pk;
    const int v = blockIdx.y;
    // block size and groups per block as one preloaded argument (threads | iters << 16): blockDim
    // would be an implicit-argument s_load, p.iters a kernel-argument one
    const int nthr = B512 ? 512 : (geo_arg & 0xFFFF), iters = ONEG ? 1 : (geo_arg >> 16);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nw = nthr >> 6;
    const int sub = lane / LSEG, t0 = lane & (LSEG - 1);
    const int32_t noise_mode = noise_arg & 0xFF;
    const uint32_t step_ctr = step_of(step_arg, noise_arg);   // (native dispatch: from the dispatch id)
    // the vehicle's Philox key: its index in the whole fleet (mppi_config.vehicle_offset rides in the
    // noise argument's high half), so a fleet split over engines draws what one engine would
    const uint32_t vkey = (uint32_t)v + ((uint32_t)noise_arg >> 16);
    STAMPRT(13);
    STAMP(0);
    // issue the global loads first (addresses need only preloaded scalars and the
    // kernarg pointer), keep the values in registers across the Philox draw
    float* u_lds = smem;
    const int HA = H_arg * NA;
    const float* usrc = u_prev + (size_t)v * HA;
    // loads per thread that cover the warm start (H*A <= LSEG*NCH*NA words) and the joint table
    constexpr int NU = B512 ? (LSEG * NCH * NA + 511) / 512 : 4, NJ = B512 ? (kJW + 511) / 512 : 2;
    float ur[NU];
    int jr[NJ];
    // an overlapped batch (kNoiseOverlap): u_prev is read only after the finalize before this
    // rollout has written it (the wait below, after the first group's normals)
    const bool ovl = !B512 && (noise_arg & kNoiseOverlap) != 0;
    auto load_u = [&]() __attribute__((always_inline)) {
        // through a buffer resource over this vehicle's u_prev: 32-bit offsets, and the rows past
        // H*A read 0 from the range check (no per-load branch, no 64-bit address math)
        const __amdgpu_buffer_rsrc_t urs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(usrc), 0, (MPPI_KO & 128) ? 0 : HA * 4, 0x00020000);
#pragma unroll
        for (int j = 0; j < NU; ++j)
            ur[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(urs, (tid + j * nthr) * 4, 0, kAuxDev));
    };
    if (!ovl) load_u();
    if (MODEL != MPPI_MODEL_DRONE) {
        const int* js = (const int*)jtab;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int i = tid + j * nthr;
            jr[j] = (i < kJW) ? js[i] : 0;
        }
    }
    // vehicle constants -> LDS (uniform reads in the FK / cost; keeping ~60 of them
    // in SGPRs spills): V == 1 from the kernel arguments, else from vc[v]
    constexpr int kVCW = (int)(sizeof(VehicleConst) / 4);
    const int vcr = (tid < kVCW) ? (VONE ? ((const int*)&pk.vc0)[tid] : ((const int*)(pk.vc + v))[tid]) : 0;
    // the lane's target rows (t clamped to H - 1: the pad lanes read the last row, their cost is masked)
    float tgt[TRK ? NCH : 1][12];
    if constexpr (TRK) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int t = t0 + 64 * c, tc = (t < H_arg) ? t : H_arg - 1;
            load_target_row<MODEL == MPPI_MODEL_DRONE>(ttab + ((size_t)v * H_arg + tc) * 12, tgt[c]);
        }
    }
    // the scene word this thread stages (the body table, then vehicle v's block)
    auto scene_word = [&](int i) __attribute__((always_inline)) {
        return scene[i < kSceneBodyW ? i : i + v * kSceneObsW];
    };
    float scr = 0.0f;
    if constexpr (OBS) scr = (tid < kSceneLdsW) ? scene_word(tid) : 0.0f;
    // SLF: the pair region's offset in the scene buffer (the body table's spare word; uniform)
    int soff = 0;
    if constexpr (SLF) soff = scene_int(scene + kSelfWord);
    float fhr = 0.0f;   // FLD: the field header word this thread stages (the block's last wave: nthr >= 64 > kFieldHdrW)
    if constexpr (FLD) fhr = (tid >= nthr - kFieldHdrW) ? field[tid - (nthr - kFieldHdrW)] : 0.0f;
    // touch every kernel-argument line the hot phases read (one s_load per 64 B): they
    // land in the scalar cache while the first group's Philox draw runs below
    // (an integer fold: uniform, so SALU -- a float sum took one VALU op per line)
    // kRoom (the kernels with the SGPRs for it: the single-group common ones k_rollout_q, k_rollout_s and
    // the fp64 single-group k_rollout / k_rollout_ql -- the looping and the extended ones stand at 98..106
    // already, and the fp32 single-group kernels of every block size, budgeted for 8 waves per SIMD,
    // spilled 4..21 SGPRs with it): instead of the touches, the values themselves -- every DevParams
    // scalar the body reads after the staging barrier, as wide s_loads here, made opaque by the empty
    // asms after the draw, so none is re-loaded or sunk to its use.  Left to the compiler each was an
    // s_load at its use, waited for on the spot: 10 round trips on the wave's chain at C3, five of them
    // in the block combine.  These kernels then read nothing of the argument segment after the barrier.
    constexpr bool kRoom = ONEG && !XC && (B512 || F64);
    uint32_t kwarm = 0u;
    if constexpr (!kRoom) {
        const uint32_t* kp = (const uint32_t*)&pk;
#pragma unroll
        for (int o = 0; o < (int)(offsetof(DevParams, sigma) / 4); o += 16) kwarm ^= kp[o];
    }
    // (HOT(m): member m of the arguments -- the pinned copy, or in a kernel without them the plain read)
#define HOT(m) (kRoom ? s_##m : pk.m)
    int32_t s_K = 0, s_nb = 0, s_j0 = 0, s_hp = 0, s_C = 0, s_store_traj = 0, s_store_noise = 0;
    float s_dt = 0.0f, s_dt2 = 0.0f, s_coef = 0.0f, s_w_sp = 0.0f, s_w_so = 0.0f, s_w_tp = 0.0f, s_w_to = 0.0f, s_sdiag[NA];
    float *s_hdr = nullptr, *s_rdata = nullptr, *s_traj = nullptr, *s_S = nullptr, *s_noise_out = nullptr;
    const float* s_noise_in = nullptr;
#pragma unroll
    for (int a = 0; a < NA; ++a) s_sdiag[a] = kRoom ? pk.sdiag[a] : 0.0f;
    if constexpr (kRoom) {
        s_K = pk.K; s_nb = pk.nb; s_j0 = pk.j0;
        s_dt = pk.dt; s_dt2 = pk.dt2; s_coef = pk.coef;
        s_w_sp = pk.w_sp; s_w_so = pk.w_so; s_w_tp = pk.w_tp; s_w_to = pk.w_to;
        s_hdr = pk.hdr; s_rdata = pk.rdata; s_noise_in = pk.noise_in;
        if constexpr (!QUIET) {   // the full kernels' own: trajectory planes, costs, stored noise
            s_hp = pk.hp; s_C = pk.C; s_store_traj = pk.store_traj; s_store_noise = pk.store_noise;
            s_traj = pk.traj; s_S = pk.S; s_noise_out = pk.noise_out;
        }
    }
    STAMPW(9);
    // the first group's standard normals overlap the loads above
    float z0[NCH][NA];
    SECTION("prologue_philox");
    if (noise_mode != MPPI_NOISE_INJECTED) {
        const uint32_t kg = k_off + (uint32_t)((blockIdx.x * nw + wid) * R + sub);
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            draw_normals<NA>(z0[c], kg, (uint32_t)(t0 + 64 * c), vkey, step_ctr, seed_lo, seed_hi);
    }
    if (ovl) {   // wave 0 waits until every finalize block of the previous step has counted it (its
                 // slice of u_prev written and drained), then the block goes on together
        if (wid == 0) {
            const uint32_t* fl = pk.ovl + (size_t)v * pk.ovl_n;
            const int nfl = pk.ovl_n;
            for (;;) {
                bool ok = true;
                for (int i = lane; i < nfl; i += 64) ok &= (int32_t)(ld_dev(fl + i) - step_ctr) >= 0;
                if (__builtin_amdgcn_ballot_w64(!ok) == 0ull) break;
                __builtin_amdgcn_s_sleep(1);
            }
        }
        lds_barrier();
        load_u();
    }
    SECTION("prologue_staging");
    STAMP(10);
    if constexpr (kRoom) {   // one wait for all of them, behind the draw
        asm volatile("" : "+s"(s_K), "+s"(s_nb), "+s"(s_j0), "+s"(s_dt), "+s"(s_dt2), "+s"(s_coef), "+s"(s_w_sp), "+s"(s_w_so),
                          "+s"(s_w_tp), "+s"(s_w_to), "+s"(s_hdr), "+s"(s_rdata), "+s"(s_noise_in));
        if constexpr (!QUIET)
            asm volatile("" : "+s"(s_hp), "+s"(s_C), "+s"(s_store_traj), "+s"(s_store_noise), "+s"(s_traj), "+s"(s_S),
                              "+s"(s_noise_out));
        if constexpr (NA == 3) asm volatile("" : "+s"(s_sdiag[0]), "+s"(s_sdiag[1]), "+s"(s_sdiag[2]));
        else if constexpr (NA == 7)
            asm volatile("" : "+s"(s_sdiag[0]), "+s"(s_sdiag[1]), "+s"(s_sdiag[2]), "+s"(s_sdiag[3]), "+s"(s_sdiag[4]),
                              "+s"(s_sdiag[5]), "+s"(s_sdiag[6]));
        else {
            static_assert(NA == 10, "pin the noise scales of a new action width here");
            asm volatile("" : "+s"(s_sdiag[0]), "+s"(s_sdiag[1]), "+s"(s_sdiag[2]), "+s"(s_sdiag[3]), "+s"(s_sdiag[4]),
                              "+s"(s_sdiag[5]), "+s"(s_sdiag[6]), "+s"(s_sdiag[7]), "+s"(s_sdiag[8]), "+s"(s_sdiag[9]));
        }
    } else {
        asm volatile("" :: "s"(kwarm));
    }
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        const int i = tid + j * nthr;
        if (i < HA) u_lds[i] = ur[j];
    }
    if constexpr (!B512)
        for (int i = tid + 4 * nthr; i < HA; i += nthr) u_lds[i] = usrc[i];   // H*A > 2048
    if (MODEL != MPPI_MODEL_DRONE) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int i = tid + j * nthr;
            if (i < kJW) ((int*)jnt)[i] = jr[j];
        }
        if constexpr (!B512)
            for (int i = tid + 2 * nthr; i < kJW; i += nthr) ((int*)jnt)[i] = ((const int*)jtab)[i];
    }
    if (tid < kVCW) {
        ((int*)&vcv)[tid] = vcr;
        if (kHand && VONE && blockIdx.x == 0)   // hand vc0 to the finalize (written through), with this
                                       // step's Philox counter in a spare word (the peer exchange's tag)
            __hip_atomic_store((int*)pk.vc + tid, tid == kVcStepWord ? (int)step_ctr : vcr, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (!B512) {
        for (int i = tid + nthr; i < kVCW; i += nthr) {   // nthr < 124
            const int x = VONE ? ((const int*)&pk.vc0)[i] : ((const int*)(pk.vc + v))[i];
            ((int*)&vcv)[i] = x;
            if (kHand && VONE && blockIdx.x == 0)
                __hip_atomic_store((int*)pk.vc + i, i == kVcStepWord ? (int)step_ctr : x, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if constexpr (OBS) {
        if (tid < kSceneLdsW) scn[tid] = scr;
        for (int i = tid + nthr; i < kSceneLdsW; i += nthr) scn[i] = scene_word(i);   // nthr < 224
    }
    if constexpr (FLD)
        if (tid >= nthr - kFieldHdrW) scn[kSceneLdsW + tid - (nthr - kFieldHdrW)] = fhr;
    if constexpr (SLF)
        for (int i = tid; i < kSelfHdrW; i += nthr) slf[i] = scene[(size_t)soff + i];
    STAMPW(8);
    if (!(MPPI_KO & 256)) lds_barrier();
    const VehicleConst& vc = vcv;
    const int H = H_arg, K = HOT(K);
    constexpr int kWs = wave_slot_floats<NA, NCH, LSEG>();
    float* const xw = smem + ((HA + 3) & ~3) + wid * kWs;   // this wave's LDS slot
    // the block's costs, nw * R consecutive k per group, staged in LDS for write-through store runs
    // after the combine barrier (st_dev_run)
    float* const s_stage = smem + ((HA + 3) & ~3) + 8 * kWs;
    // OBS: the block's clearances, staged the same way behind the costs
    float* const c_stage = OBS ? s_stage + iters * cost_run_stride(nw * R) : nullptr;
    // SLF: the self clearances behind those, then the centre column (this lane's words: pitch nthr)
    float* const sc_stage = SLF ? c_stage + iters * cost_run_stride(nw * R) : nullptr;
    float* const scol = SLF ? sc_stage + iters * cost_run_stride(nw * R) + tid : nullptr;
    STAMP(1);

    // trajectory planes of vehicle v (from kernel arguments and blockIdx only, so the
    // descriptor stays in SGPRs)
    // rows padded to 64 B (hp = H rounded up to 16) and written whole, pad lanes included: the
    // write-through stores then never leave a partial 64 B sector for HBM to merge
    const int hp = kTraj ? HOT(hp) : 0;
    const uint32_t plane_b = (uint32_t)K * (uint32_t)hp * 4u;
    const __amdgpu_buffer_rsrc_t trs = traj_rsrc(kTraj ? HOT(traj) + (size_t)v * HOT(C) * K * hp : nullptr, plane_b,
                                                 kTraj ? HOT(C) : 0);

    float acc[NCH][NA];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int a = 0; a < NA; ++a) acc[c][a] = 0.0f;
    float rho_w = INFINITY, eta_w = 0.0f, eta2_w = 0.0f;   // wave-uniform
    bool nan_w = false;

    // One group of R rollouts per wave.  Written as a lambda so the common
    // single-group launch (iters == 1, e.g. K=4096 H=32) is straight-line code:
    // no loop-invariant hoisting of address math / key schedules into SGPRs.
    auto group = [&](const int it) __attribute__((always_inline)) {   // (the NCH = 4 extended kernel called it out of line: a 1.7 KB stack frame)
        asm volatile("" ::: "memory");   // keep LDS constant reads inside the group
        SECTION("noise");
        // group it of block b: groups b, b + nb, ...  All blocks' groups of one iteration are
        // consecutive, so the grid's concurrent trajectory stores stay in one region of the planes
        // (consecutive groups per block scattered them: whole-body K=65536 85.5 -> 106-110 us)
        const int g = blockIdx.x + it * HOT(nb);
        const int k = (g * nw + wid) * R + sub;
        const bool kval = k < K;
        const int kc = kval ? k : K - 1;   // clamped: every load stays in bounds
        const uint32_t kg = k_off + (uint32_t)k;

        // ---- A1/A2: eps = z Sigma (device Philox) or injected; act = u_prev + eps
        float eps[NCH][NA], act[NCH][NA];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int t = t0 + 64 * c;
            const bool val = kval && t < H;
            const int tc = (t < H) ? t : H - 1;
            if (noise_mode == MPPI_NOISE_INJECTED) {
                const float* src = HOT(noise_in) + (((size_t)v * K + kc) * H + tc) * NA;
#pragma unroll
                for (int a = 0; a < NA; ++a) eps[c][a] = src[a];
            } else {
                float z[NA];
                if (it == 0) {
#pragma unroll
                    for (int a = 0; a < NA; ++a) z[a] = z0[c][a];
                } else {
                    draw_normals<NA>(z, kg, (uint32_t)t, vkey, step_ctr, seed_lo, seed_hi);
                }
                if (!XC || p.sigma_diag) {   // a full Sigma runs in the extended (XC) kernel
#pragma unroll
                    for (int a = 0; a < NA; ++a) eps[c][a] = z[a] * (kRoom ? s_sdiag[a] : pk.sdiag[a]);
                } else {
#pragma unroll
                    for (int b = 0; b < NA; ++b) {
                        float e = 0.0f;
#pragma unroll
                        for (int a = 0; a < NA; ++a) e += z[a] * p.sigma[a * NA + b];
                        eps[c][b] = e;
                    }
                }
            }
            // the warm-start row first, unconditionally (tc is clamped): inside the select the
            // compiler turned every LDS read into its own exec-masked branch and s_waitcnt,
            // NA serial LDS round trips per lane
            float ur[NA];
#pragma unroll
            for (int a = 0; a < NA; ++a) ur[a] = u_lds[tc * NA + a];
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                eps[c][a] = val ? eps[c][a] : 0.0f;
                act[c][a] = val ? ur[a] + eps[c][a] : 0.0f;
            }
            if (!QUIET && HOT(store_noise) && val) {   // (readback only: written through, st_dev)
                float* dst = HOT(noise_out) + (((size_t)v * K + k) * H + t) * NA;
#pragma unroll
                for (int a = 0; a < NA; ++a) st_dev(dst + a, eps[c][a]);
            }
        }
        // extra CostManager terms on the controls (cost_manager.py:83,86): covar
        // u_t^T Sigma^-1 v_t (covar_cost.py:20-25) and action w*gamma^t*||v_t||^2
        // (action_cost.py:14-24); per lane, summed over t with the costs below
        float ecov = 0.0f, eact = 0.0f, gts[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) gts[c] = 0.0f;
        // (the tracking bit alone reads neither gamma_t nor sinv)
        if (XC && (TRK ? (p.cost_terms & ~MPPI_COST_TARGET_TRACK) : p.cost_terms)) {   // (the XC kernel also runs a full Sigma
                                    //  without extra terms: gamma_t / sinv exist only with cost_terms)
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int t = t0 + 64 * c;
                const bool val = kval && t < H;
                const int tc = (t < H) ? t : H - 1;
                gts[c] = val ? p.gamma_t[tc] : 0.0f;
                if (p.cost_terms & MPPI_COST_COVAR) {
                    float qd = 0.0f;
#pragma unroll
                    for (int a = 0; a < NA; ++a) {
                        float y = 0.0f;
                        if (p.sigma_diag) {
                            y = p.sinv[a * NA + a] * act[c][a];
                        } else {
#pragma unroll
                            for (int b = 0; b < NA; ++b) y = fmaf(p.sinv[a * NA + b], act[c][b], y);
                        }
                        qd = fmaf(u_lds[tc * NA + a], y, qd);
                    }
                    ecov += val ? qd : 0.0f;
                }
                if (p.cost_terms & MPPI_COST_ACTION) {
                    float s2 = 0.0f;
#pragma unroll
                    for (int a = 0; a < NA; ++a) s2 = fmaf(act[c][a], act[c][a], s2);
                    eact += val ? (p.w_act * s2) * gts[c] : 0.0f;
                }
            }
        }
        if (it == 0) STAMP(2);
        SECTION("integrator");

        // ---- A3: double integrator (standard_normal_noise.py:41-48).  Both cumsums
        //      are fp32 Kogge-Stone scans over DPP: they sum small increments
        //      (a*dt, v*dt + a*dt^2/2), so their rounding stays ~1e-10 absolute, far
        //      below one ulp of the positions; q0 is added in the state
        //      dtype (fp64 state -> fp64 positions, as update_joint's float64 arrays).
        float posf[NCH][NA];
        double posd[NCH][F64 ? NA : 1];
        if constexpr (NCH == 1 && !(MPPI_KO & 1)) {
            float inc[NA];
            integrate_lds<LSEG, NA>(act[0], xw, lane, HOT(dt), 0.5f * HOT(dt2), vc.vel0f, inc);
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                if (!F64) {
                    posf[0][a] = inc[a] + vc.pos0f[a];
                } else {
                    posd[0][a] = (double)inc[a] + vc.pos0[a];
                    posf[0][a] = (float)posd[0][a];
                }
            }
        } else {
#pragma clang fp contract(off)
            float carry1[NA], carry2[NA], lastv[NA];
#pragma unroll
            for (int a = 0; a < NA; ++a) { carry1[a] = 0.0f; carry2[a] = 0.0f; lastv[a] = 0.0f; }
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                float c1[NA], c2[NA];
#pragma unroll
                for (int a = 0; a < NA; ++a) c1[a] = act[c][a] * HOT(dt);
                seg_scan_f32_multi<LSEG, NA>(c1);
#pragma unroll
                for (int a = 0; a < NA; ++a) {
                    if (NCH > 1) {
                        c1[a] += carry1[a];
                        carry1[a] = read_lane_f32(c1[a], 63);
                    }
                    // (0.5 a) dt^2 == a (0.5 dt^2) bit for bit: both are one rounding of the
                    // same product, the halvings being exact
                    const float h2 = act[c][a] * (0.5f * HOT(dt2));
                    const float velf = c1[a] + vc.vel0f[a];
                    float prev = dpp_f32<0x138, 0xF>(velf);     // wave_shr:1
                    if (t0 == 0) prev = (c == 0) ? vc.vel0f[a] : lastv[a];
                    if (NCH > 1) lastv[a] = read_lane_f32(velf, 63);
                    c2[a] = prev * HOT(dt) + h2;
                }
                seg_scan_f32_multi<LSEG, NA>(c2);
#pragma unroll
                for (int a = 0; a < NA; ++a) {
                    if (NCH > 1) {
                        c2[a] += carry2[a];
                        carry2[a] = read_lane_f32(c2[a], 63);
                    }
                    if (!F64) {
                        posf[c][a] = c2[a] + vc.pos0f[a];
                    } else {
                        posd[c][a] = (double)c2[a] + vc.pos0[a];
                        posf[c][a] = (float)posd[c][a];
                    }
                }
            }
        }
        if (it == 0) STAMP(3);
        SECTION("fk_chain");
        if (ONEG) set_wave_prio(2);   // progress priority (single group): see below

        // eps is read again only by the softmin accumulate at the end of the group: park
        // it in this wave's LDS slot (the integrator is done with it; each lane its own
        // row, so no hand-off) across the FK and cost, the kernel's register peak.  The
        // compiler barriers stop it from forwarding the stored values in registers.
        // In the extended and the multi-chunk kernels only: the common one-chunk kernels keep it in
        // registers (whole-body 89 -> 96 VGPRs, still 5 waves per SIMD, no scratch; same-process A/B, mean of
        // both orders, profiles/r05/eps_stash: C3 -0.10 us per step, whole-body K=8192 -0.22, K=65536 -1.7,
        // V=8 fleet -1.7)
        constexpr bool kStash = NA >= 7 && (XC || NCH > 1);
        constexpr int kESP = (NCH == 1) ? IntegGeom<LSEG, NA>::P : NA;   // row pitch (odd for NCH == 1)
        if constexpr (kStash) {
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int a = 0; a < NA; ++a) xw[(c * 64 + lane) * kESP + a] = eps[c][a];
            asm volatile("" ::: "memory");
        }

        // ---- A4-A10: FK + per-step cost, trajectory planes
        float xs[NCH];
        float ecen = 0.0f, ejt = 0.0f, elim = 0.0f;
        RollAcc<OBS, SLF> oacc;   // OBS: the lane's obstacle term and min clearance over its steps (SLF: and the self-collision term's)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int t = t0 + 64 * c;
            const bool val = kval && t < H;
            const bool term = (t == H - 1);
            float x;
            // OBS: this step's hinge sum and min clearance (the obstacles at their row time (t + 1) dt)
            RollAcc<OBS, SLF> ostep;   // (SLF: and the pairs' hinge sum and min clearance of this step)
            const uint32_t toff = ((uint32_t)k * (uint32_t)hp + (uint32_t)t) * 4u;   // byte offset in a plane
            const bool stv = kTraj && HOT(store_traj) && kval && t < hp;   // row incl. its pad (finite values)
            if (MODEL == MPPI_MODEL_DRONE) {
                const float dx = posf[c][0] - (TRK ? tgt[c][0] : vc.tpos[0]), dy = posf[c][1] - (TRK ? tgt[c][1] : vc.tpos[1]),
                            dz = posf[c][2] - (TRK ? tgt[c][2] : vc.tpos[2]);
                x = dx * dx + dy * dy + dz * dz;
                if constexpr (OBS) {   // no chain: the spheres ride on p(k,t) in world axes
                    const float Td[12] = {1.0f, 0.0f, 0.0f, posf[c][0], 0.0f, 1.0f, 0.0f, posf[c][1], 0.0f, 0.0f, 1.0f, posf[c][2]};
                    if constexpr (FLD) obs_frame_field(Td, scn, scn + kSceneBodyW, 0, (float)(t + 1) * p.dt, scn + kSceneLdsW, field + kFieldHdrW, ostep.sum, ostep.gmin);
                    else obs_frame(Td, scn, scn + kSceneBodyW, 0, (float)(t + 1) * p.dt, ostep.sum, ostep.gmin);
                }
                if (stv) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) traj_store(trs, toff, (uint32_t)a * plane_b, posf[c][a]);
                }
            } else {
                // joint angle j in the state dtype (fp64 state -> fp64 sin/cos reduction)
                auto qang = [&](int cc_, int j) {
                    if constexpr (F64) return posd[cc_][QOFF + j]; else return posf[cc_][QOFF + j];
                };
                if (stv) {   // positions first: each dies after its joint's FK step
#pragma unroll
                    for (int a = 0; a < NA; ++a) traj_store(trs, toff, (uint32_t)a * plane_b, posf[c][a]);
                }
                Mat34 T;   // base (times the folded leading fixed joints)
#pragma unroll
                for (int i = 0; i < 12; ++i) T.m[i] = vc.base[i];
                if (MODEL == MPPI_MODEL_WHOLEBODY) {   // [R(rpy) | p_drone(k,t)] * M_fixed
                    T.m[3] += posf[c][0]; T.m[7] += posf[c][1]; T.m[11] += posf[c][2];
                }
                // OBS: the spheres of a frame slot as soon as T is that frame (slot 0: the folded base)
                auto obs_at = [&](int slot) __attribute__((always_inline)) {
                    if constexpr (SLF) obs_frame_self<FLD>(T.m, scn, scn + kSceneBodyW, slot, (float)(t + 1) * p.dt, FLD ? scn + kSceneLdsW : nullptr,
                                                           FLD ? field + kFieldHdrW : nullptr, slf, scol, nthr, ostep.sum, ostep.gmin);
                    else if constexpr (FLD) obs_frame_field(T.m, scn, scn + kSceneBodyW, slot, (float)(t + 1) * p.dt, scn + kSceneLdsW, field + kFieldHdrW, ostep.sum, ostep.gmin);
                    else if constexpr (OBS) obs_frame(T.m, scn, scn + kSceneBodyW, slot, (float)(t + 1) * p.dt, ostep.sum, ostep.gmin);
                };
                obs_at(0);
                if (MPPI_KO & 4) {
                    T.m[3] += posf[c][QOFF]; T.m[7] += posf[c][QOFF + 1];
                } else if (NQ == 7 && (!XC || p.chain_fast == 2)) {   // Kinova: origin rotations are signed
                    // permutations (the common kernel runs only this chain; any other goes to XC)
                    // the C3 kernels (arm, fp64 state, one 32-lane segment; the max-ilp unit): the seven joints'
                    // sin / cos (each needs only the integrator's q_j) formed ahead of the chain, seven independent
                    // reductions and transcendental pairs, instead of each inside its joint's step, where its
                    // result is consumed at once
                    if constexpr (!XC && NCH == 1 && F64 && LSEG == 32 && MODEL == MPPI_MODEL_ARM) {
                        float sj[7], cj[7];
#pragma unroll
                        for (int j = 0; j < 7; ++j) sincos_joint(qang(c, j), sj[j], cj[j]);
                        __builtin_amdgcn_sched_barrier(0);   // (the scheduler would sink each pair to its use)
                        kin_joint_sc<0>(T, jnt[HOT(j0) + 0].O, sj[0], cj[0]);
                        kin_joint_sc<1>(T, jnt[HOT(j0) + 1].O, sj[1], cj[1]);
                        kin_joint_sc<2>(T, jnt[HOT(j0) + 2].O, sj[2], cj[2]);
                        kin_joint_sc<3>(T, jnt[HOT(j0) + 3].O, sj[3], cj[3]);
                        kin_joint_sc<4>(T, jnt[HOT(j0) + 4].O, sj[4], cj[4]);
                        kin_joint_sc<5>(T, jnt[HOT(j0) + 5].O, sj[5], cj[5]);
                        kin_joint_sc<6>(T, jnt[HOT(j0) + 6].O, sj[6], cj[6]);
                    } else {
                        kin_joint<0>(T, jnt[HOT(j0) + 0].O, qang(c, 0));
                        obs_at(1);
                        kin_joint<1>(T, jnt[HOT(j0) + 1].O, qang(c, 1));
                        obs_at(2);
                        kin_joint<2>(T, jnt[HOT(j0) + 2].O, qang(c, 2));
                        obs_at(3);
                        kin_joint<3>(T, jnt[HOT(j0) + 3].O, qang(c, 3));
                        obs_at(4);
                        kin_joint<4>(T, jnt[HOT(j0) + 4].O, qang(c, 4));
                        obs_at(5);
                        kin_joint<5>(T, jnt[HOT(j0) + 5].O, qang(c, 5));
                        obs_at(6);
                        kin_joint<6>(T, jnt[HOT(j0) + 6].O, qang(c, 6));
                        obs_at(7);
                    }
                } else if (!XC) {   // (unreachable: the common kernel is dispatched for Kinova chains only)
                } else if (p.chain_fast) {   // nq revolute-z joints, q_index = 0..nq-1 in order
#pragma unroll
                    for (int j = 0; j < NQ; ++j) {
                        const JointDev& J = jnt[HOT(j0) + j];
                        mul_affine(T, J.O);
                        float s, cc;
                        sincos_joint(qang(c, j), s, cc);
                        const float omc = 1.0f - cc, r22 = cc + omc;
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            const float a0 = T.m[4 * i], a1 = T.m[4 * i + 1];
                            T.m[4 * i] = a0 * cc + a1 * s;
                            T.m[4 * i + 1] = a1 * cc - a0 * s;
                            T.m[4 * i + 2] = T.m[4 * i + 2] * r22;
                        }
                        obs_at(j + 1);
                    }
                } else {
                    for (int jn = HOT(j0); jn < p.nj; ++jn) {
                        const JointDev& J = jnt[jn];
                        mul_affine(T, J.O);
                        if (J.type == MPPI_JOINT_FIXED) {
                            obs_at(jn - HOT(j0) + 1);
                            continue;
                        }
                        double qd = 0.0;
                        float qf = 0.0f;
#pragma unroll
                        for (int a = 0; a < NQ; ++a)
                            if (a == J.q_index) {
                                qd = F64 ? posd[c][QOFF + a] : 0.0;
                                qf = posf[c][QOFF + a];
                            }
                        if (J.type == MPPI_JOINT_REVOLUTE) {
                            float s, cc;
                            if constexpr (F64) sincos_joint(qd, s, cc); else sincos_joint(qf, s, cc);
                            mul_revolute(T, J, cc, s);
                        } else {
                            mul_prismatic(T, J, qf);
                        }
                        obs_at(jn - HOT(j0) + 1);
                    }
                }
                if constexpr (SLF) self_pairs(slf, scol, nthr, ostep.ssum, ostep.sgmin);   // every member's centre is in the column
                // the four weights as SGPR values: selecting between two kernel-argument
                // addresses per lane would otherwise become two vector loads in the FK
                const float wsp = uniform_f32(HOT(w_sp)), wso = uniform_f32(HOT(w_so)), wtp = uniform_f32(HOT(w_tp)),
                            wto = uniform_f32(HOT(w_to));
                SECTION("pose_cost");
                if constexpr (TRK) x = pose_cost_row(T, tgt[c], term ? wtp : wsp, term ? wto : wso);
                else x = (MPPI_KO & 8) ? T.m[3] + T.m[7] + T.m[11] + T.m[0] : pose_cost(T, vc, term ? wtp : wsp, term ? wto : wso);
                SECTION("traj_ee_stores");
                if (stv) {
#pragma unroll
                    for (int i = 0; i < 12; ++i) traj_store(trs, toff, (uint32_t)(NA + i) * plane_b, T.m[i]);
                }
            }
            xs[c] = val ? x : 0.0f;
            if constexpr (OBS) {
                oacc.sum += val ? obs_step_cost(scn, ostep.sum, ostep.gmin) : 0.0f;
                oacc.gmin = fminf(oacc.gmin, val ? ostep.gmin : INFINITY);
            }
            if constexpr (SLF) {
                oacc.ssum += val ? self_step_cost(slf, ostep.ssum, ostep.sgmin) : 0.0f;
                oacc.sgmin = fminf(oacc.sgmin, val ? ostep.sgmin : INFINITY);
            }
            // extra joint-space terms (cost_manager.py:84,85,87; joint_space_cost.py)
            if (XC && (p.cost_terms & (MPPI_COST_CENTER | MPPI_COST_JOINT_TRACK | MPPI_COST_JOINT_LIMIT))) {
                const int tc = (t < H) ? t : H - 1;
                const float* jt = p.jtraj ? p.jtraj + ((size_t)v * H + tc) * NQ : nullptr;
                float sc = 0.0f, sj = 0.0f;
                bool out = false;
#pragma unroll
                for (int j = 0; j < NQ; ++j) {
                    const float qj = posf[c][QOFF + j];
                    const float dc = qj - vc.qc[j];
                    sc = fmaf(dc, dc, sc);
                    const float dj = qj - (jt ? jt[j] : 0.0f);
                    sj = fmaf(dj, dj, sj);
                    const double qd = F64 ? posd[c][QOFF + j] : (double)qj;   // limits in the state dtype
                    out |= (qd < (double)vc.qlo[j]) | (qd > (double)vc.qhi[j]);
                }
                if (val) {
                    if constexpr (SLF) {   // (the weights as late reads: late_arg)
                        if (p.cost_terms & MPPI_COST_CENTER) ecen += (late_arg(pk.w_cen) * sc) * gts[c];
                        if (p.cost_terms & MPPI_COST_JOINT_TRACK) ejt += (late_arg(pk.w_jt) * sj) * gts[c];
                        if ((p.cost_terms & MPPI_COST_JOINT_LIMIT) && out) elim += late_arg(pk.lim_pen) * gts[c];
                    } else {
                        if (p.cost_terms & MPPI_COST_CENTER) ecen += (p.w_cen * sc) * gts[c];
                        if (p.cost_terms & MPPI_COST_JOINT_TRACK) ejt += (p.w_jt * sj) * gts[c];
                        if ((p.cost_terms & MPPI_COST_JOINT_LIMIT) && out) elim += p.lim_pen * gts[c];
                    }
                }
            }
        }
        if (it == 0) STAMP(4);
        SECTION("cost_sum_softmin");
        if (ONEG) set_wave_prio(1);

        // ---- S_k = fl(ws * sum_{t<H-1} x_t) + fl(wt * x_{H-1}) per segment (wave-uniform picks)
        float st = 0.0f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) st += (t0 + 64 * c < H - 1) ? xs[c] : 0.0f;
        st = seg_scan_f32<LSEG>(st);
        float xt = 0.0f;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            if (c == (H - 1) / 64) xt = xs[c];
        float S_seg[R];
#pragma unroll
        for (int s = 0; s < R; ++s) {
            const int ks = (g * nw + wid) * R + s;
            const float stage = read_lane_f32(st, s * LSEG + LSEG - 1);
            const float term = read_lane_f32(xt, s * LSEG + ((H - 1) & 63));
            float S = (MODEL == MPPI_MODEL_DRONE) ? (HOT(w_sp) * stage) + (HOT(w_tp) * term) : stage + term;
            S_seg[s] = (ks < K) ? S : INFINITY;
        }
        if (XC) {   // S += covar, center, jtraj, action, limit
            float tsum[5] = {ecov, ecen, ejt, eact, elim};
            const int bits[5] = {MPPI_COST_COVAR, MPPI_COST_CENTER, MPPI_COST_JOINT_TRACK, MPPI_COST_ACTION,
                                 MPPI_COST_JOINT_LIMIT};
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                if (!(p.cost_terms & bits[i])) continue;
                const float ts = seg_scan_f32<LSEG>(tsum[i]);
#pragma unroll
                for (int s = 0; s < R; ++s) {
                    float add = read_lane_f32(ts, s * LSEG + LSEG - 1);
                    if (i == 0) {
                        if constexpr (SLF) add = late_arg(pk.w_cov) * add;
                        else add = p.w_cov * add;
                    }
                    S_seg[s] += add;
                }
            }
        }
        if constexpr (OBS) {   // S += the obstacle term (after the CostManager terms); the sample's clearance
            const float ts = seg_scan_f32<LSEG>(oacc.sum);
#pragma unroll
            for (int s = 0; s < R; ++s) S_seg[s] += read_lane_f32(ts, s * LSEG + LSEG - 1);
            const float clr = seg_min_f32<LSEG>(oacc.gmin);
            if (kCosts && kval && t0 == 0) c_stage[it * cost_run_stride(nw * R) + wid * R + sub] = clr;
        }
        if constexpr (SLF) {   // S += the self-collision term (after the obstacle term); the sample's self clearance
            const float ts = seg_scan_f32<LSEG>(oacc.ssum);
#pragma unroll
            for (int s = 0; s < R; ++s) S_seg[s] += read_lane_f32(ts, s * LSEG + LSEG - 1);
            const float sclr = seg_min_f32<LSEG>(oacc.sgmin);
            if (kCosts && kval && t0 == 0) sc_stage[it * cost_run_stride(nw * R) + wid * R + sub] = sclr;
        }
        float S_mine = S_seg[0];
#pragma unroll
        for (int s = 1; s < R; ++s) S_mine = (sub == s) ? S_seg[s] : S_mine;
        // (s_S named: the group's closure keeps the reference round 3's plain S store gave it.  Without it
        // the every-knockout build of the whole-body k_rollout_q allocates two VGPRs the other way round;
        // drop it with the next change to these kernels' instruction streams.)
        (void)s_S;
        if (kCosts && kval && t0 == 0) s_stage[it * cost_run_stride(nw * R) + wid * R + sub] = S_mine;

        // ---- online softmin (mppi.py:184-188) over this wave's rollouts (scalar bookkeeping)
        float m = INFINITY;
#pragma unroll
        for (int s = 0; s < R; ++s) {
            const bool bad = S_seg[s] != S_seg[s];
            nan_w |= bad;
            if (!bad) m = fminf(m, S_seg[s]);
        }
        if (m < INFINITY) {
            const float rn = fminf(rho_w, m);
            // The selects around this section's exps stay.  This one is free where it counts: in a
            // single-group kernel rho_w is the constant +inf here and f folds to 0, while a bare
            // exp(coef * (inf - rn)) would not fold (coef's sign is a run-time fact).  The next guards
            // S_seg = NaN (a NaN cost is kept out of the min but is still an S_seg: exp(NaN) != 0) along
            // with k >= K's +inf, and e_mine's guard is the same NaN test.
            const float f = (rho_w == INFINITY) ? 0.0f : __expf(HOT(coef) * (rho_w - rn));
            float es = 0.0f, e2 = 0.0f;
#pragma unroll
            for (int s = 0; s < R; ++s) {
                const float e = (S_seg[s] < INFINITY) ? __expf(HOT(coef) * (S_seg[s] - rn)) : 0.0f;
                es += e;
                if constexpr (kEta2) e2 += e * e;
            }
            eta_w = eta_w * f + es;
            if constexpr (kEta2) eta2_w = eta2_w * f * f + e2;
            const float e_mine = (kval && !(S_mine != S_mine)) ? __expf(HOT(coef) * (S_mine - rn)) : 0.0f;
            if constexpr (kStash) {
                asm volatile("" ::: "memory");
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int a = 0; a < NA; ++a) eps[c][a] = xw[(c * 64 + lane) * kESP + a];
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c)
#pragma unroll
                for (int a = 0; a < NA; ++a) acc[c][a] = acc[c][a] * f + e_mine * eps[c][a];
            rho_w = rn;
        }
    };
    if (ONEG) {
        // Progress priority: 3 until the integrator is done, 2 through FK and cost, 1 for the
        // softmin, 0 in the block combine.  The waves of a SIMD start over ~2 us of launch
        // ramp; under the arbiter's oldest-first order the early ones would finish early and
        // leave the late ones to run alone -- here a wave that is ahead yields.  (Priorities off
        // measured slower: DESIGN.md §11, profiles/r05/prio/.)
        set_wave_prio(3);
        group(0);
        set_wave_prio(0);
    } else if (iters == 1) {
        group(0);
    } else {
        // Wave priority by remaining groups: the SIMD arbiter otherwise favours the oldest
        // wave, so the waves of a SIMD finish their (equal) work one after another and the
        // last ones run alone, without latency hiding (the grid's tail).  A
        // wave that is ahead drops its priority, the laggards catch up.
        for (int it = 0; it < iters; ++it) {
            set_wave_prio(iters - 1 - it);
            group(it);
        }
        set_wave_prio(0);
    }
    STAMP(5);
    SECTION("block_combine_record");

    // ---- cross-wave combine in LDS -> one partial record per block, one barrier:
    //      after the barrier every record thread takes rho_b = min of the 8 wave slots'
    //      rho and rescales them itself (f_w = exp(-(rho_w - rho_b)/lambda)).
    //      LDS: [8][4 + NCH*64*NA]; every lane (all R segments) deposits acc
    float* wsh = smem + ((HA + 3) & ~3);           // always 8 wave slots (unrolled reads)
    const int wstride = kWs;   // >= 4 + NCH*64*NA (the integrator's buffer may be larger)
    float* mine = wsh + wid * wstride;
    if (lane == 0) {
        mine[0] = rho_w; mine[1] = eta_w; mine[2] = eta2_w; mine[3] = nan_w ? 1.0f : 0.0f;
    }
    if constexpr (!B512)
        for (int i = nw * wstride + tid; i < 8 * wstride; i += nthr)   // absent waves: rho = inf, acc = 0
            wsh[i] = ((i - nw * wstride) % wstride == 0) ? INFINITY : 0.0f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int a = 0; a < NA; ++a) mine[4 + (c * 64 + lane) * NA + a] = acc[c][a];
    // The record stores' bases and offsets: they depend on the block's index, nb, H and NA
    // alone, so they are formed here, ahead of the barrier, and made opaque -- between the barrier and
    // the stores, where the block's other waves are already idle, only LDS reads and arithmetic remain.
    // A one-vehicle kernel has v = 0: no vehicle offset (64-bit scalar multiplies) at all.
    // (In the kernels with SGPRs to spare, kRoom; the others form them between the barrier and the stores.)
    const uint32_t vz = (kRoom && VONE) ? 0u : (uint32_t)v;
    uint32_t hoff, rbase, rstride;
    float *hdr_u, *rdata_v;
    auto header_base = [&]() __attribute__((always_inline)) {
        hoff = (vz * (uint32_t)HOT(nb) + blockIdx.x) * 16u;
        hdr_u = uniform_ptr(HOT(hdr));
    };
    auto body_base = [&]() __attribute__((always_inline)) {
        rdata_v = uniform_ptr(HOT(rdata) + (size_t)vz * NA * HOT(nb) * H);   // this vehicle's bodies (< 1 GiB)
        rbase = blockIdx.x * (uint32_t)H;
        rstride = (uint32_t)HOT(nb) * (uint32_t)H;
    };
    if constexpr (kRoom) {
        header_base();
        body_base();
        // (uniform, but the compiler may have formed them on the VALU for a vector user: an asm operand must be an SGPR)
        hoff = __builtin_amdgcn_readfirstlane(hoff);
        rbase = __builtin_amdgcn_readfirstlane(rbase);
        rstride = __builtin_amdgcn_readfirstlane(rstride);
        asm volatile("" : "+s"(hoff), "+s"(hdr_u), "+s"(rdata_v), "+s"(rbase), "+s"(rstride));
    }
    STAMPW(11);
    lds_barrier();
    STAMP(6);
    if (kCosts && wid == nw - 1) {
        // The block's costs: one write-through run per group (st_dev_run), nw * R consecutive
        // samples each -- one whole 64 B line per group at R = 2 (H <= 32: C2, C3).  Issued by
        // the block's last wave, which has the fewest record stores behind it: from wave 0 the
        // write-through made the drone C2 step 0.2-0.3 us slower, from the last wave it is
        // within the A/B noise of round 3's plain stores (profiles/r04/ab_cost_store_variants.txt)
        const int nS = nw * R, q = (nS + 3) >> 2;
        float* const Sv = uniform_ptr(HOT(S) + (size_t)v * K);
        for (int i = lane; i < iters * q; i += 64) {
            const int it = i / q, k0 = (blockIdx.x + it * HOT(nb)) * nS;
            st_dev_run(Sv, (uint32_t)k0, s_stage + it * cost_run_stride(nS), min(nS, K - k0), i - it * q);
        }
        if constexpr (OBS) {   // the clearances beside them: (V, K) in the scene buffer
            float* const Cv = uniform_ptr(scene + (size_t)scene_int(scn + 4) + (size_t)v * K);
            for (int i = lane; i < iters * q; i += 64) {
                const int it = i / q, k0 = (blockIdx.x + it * HOT(nb)) * nS;
                st_dev_run(Cv, (uint32_t)k0, c_stage + it * cost_run_stride(nS), min(nS, K - k0), i - it * q);
            }
        }
        if constexpr (SLF) {   // and the self clearances: (V, K) in the pair region
            float* const Cs = uniform_ptr(scene + (size_t)scene_int(slf + 5) + (size_t)v * K);
            for (int i = lane; i < iters * q; i += 64) {
                const int it = i / q, k0 = (blockIdx.x + it * HOT(nb)) * nS;
                st_dev_run(Cs, (uint32_t)k0, sc_stage + it * cost_run_stride(nS), min(nS, K - k0), i - it * q);
            }
        }
    }
    // rho_b = the min of the 8 wave slots, which every thread reads for f_w anyway (an LDS
    // atomicMin before the barrier cost a waterfall loop and a ds_min per wave)
    float rws[8], rho_b = INFINITY;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        rws[w] = wsh[w * wstride];
        rho_b = fminf(rho_b, rws[w]);
    }
    // f_w = exp(-(rho_w - rho_b)/lambda): lane w evaluates wave w's, every lane reads all 8 back
    // (one transcendental per lane instead of eight)
    float fw[8];
    {
        float mine = INFINITY;
#pragma unroll
        for (int w = 0; w < 8; ++w) mine = ((lane & 7) == w) ? rws[w] : mine;
        const float f = (mine < INFINITY) ? __expf(HOT(coef) * (mine - rho_b)) : 0.0f;
#pragma unroll
        for (int w = 0; w < 8; ++w) fw[w] = read_lane_f32(f, w);
    }
    STAMP(12);
    if (tid == 0) {
        float eta = 0.0f, eta2 = 0.0f, nanf = 0.0f;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            eta += fw[w] * wsh[w * wstride + 1];
            if constexpr (kEta2) eta2 += fw[w] * fw[w] * wsh[w * wstride + 2];
            nanf = fmaxf(nanf, wsh[w * wstride + 3]);
        }
        if constexpr (!kRoom) header_base();
        wt_store4(hdr_u, hoff, make_float4(rho_b, eta, eta2, nanf));
    }
    // record body, dim-major: rdata[v][a][block][t] = sum_w f_w sum_segments acc_w[seg*L + t].
    // (a, t) of element i without an integer division (~25 VALU): a = trunc((i + 1/2) / H)
    // in fp32 is exact, the quotient's error (< 1e-5 for i < A*H <= 2560) being far below
    // the 1/(2H) margin; 32-bit record indices (V*A*nb*H < 2^31, checked at create).
    const float rH = __builtin_amdgcn_rcpf((float)H);   // (1 ulp: far inside the 1/(2H) margin)
    if constexpr (!kRoom) body_base();
    for (int i = tid; i < ((MPPI_KO & 64) ? 0 : HA); i += nthr) {
        const int a = (int)(((float)i + 0.5f) * rH), t = i - a * H;
        const int c = t >> 6, tl = t & 63;
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            float sw = wsh[w * wstride + 4 + (c * 64 + tl) * NA + a];
#pragma unroll
            for (int sg = 1; sg < R; ++sg) sw += wsh[w * wstride + 4 + (c * 64 + sg * LSEG + tl) * NA + a];
            s += fw[w] * sw;
        }
        wt_store(rdata_v, (rbase + (uint32_t)a * rstride + (uint32_t)t) * 4u, s);
    }
    STAMP(7);
    STAMPRT(14);
    drain_stores();
#undef HOT
}

template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool VONE, bool XC, bool ONEG>
__global__ void __launch_bounds__(512, (roll_occ<NCH, F64, XC, ONEG>())) k_rollout(const uint32_t seed_lo, const uint32_t seed_hi,
                                                 const uint32_t step_arg, const uint32_t k_off,
                                                 const int32_t noise_arg, const int32_t H_arg,
                                                 const int32_t geo_arg,
                                                 const float* __restrict__ u_prev,
                                                 const JointDev* __restrict__ jtab, const DevParams pk) {
    rollout_body<MODEL, NA, NCH, LSEG, F64, VONE, XC, ONEG, false>(seed_lo, seed_hi, step_arg, k_off, noise_arg, H_arg,
                                                                   geo_arg, u_prev, jtab, pk);
}
// The single-group kernel at its one block size (B512 above): the same arguments, geo_arg not read.
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool VONE, bool XC>
__global__ void __launch_bounds__(512, (roll_occ<NCH, F64, XC, true>())) k_rollout_s(const uint32_t seed_lo, const uint32_t seed_hi,
                                                 const uint32_t step_arg, const uint32_t k_off,
                                                 const int32_t noise_arg, const int32_t H_arg,
                                                 const int32_t geo_arg,
                                                 const float* __restrict__ u_prev,
                                                 const JointDev* __restrict__ jtab, const DevParams pk) {
    rollout_body<MODEL, NA, NCH, LSEG, F64, VONE, XC, true, true>(seed_lo, seed_hi, step_arg, k_off, noise_arg, H_arg,
                                                                  geo_arg, u_prev, jtab, pk);
}

// The quiet rollout (rollout_body QUIET): k_rollout_q is k_rollout_s's quiet form, k_rollout_ql
// k_rollout's (any block size, one group or a loop of them).  New symbols: the full kernels' names
// stay as they are.  Same arguments as the full kernels, so a launch differs only in its symbol
// and its LDS size (no cost runs).
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool VONE, bool XC, bool ONEG>
__global__ void __launch_bounds__(512, (roll_occ<NCH, F64, XC, ONEG>())) k_rollout_ql(const uint32_t seed_lo, const uint32_t seed_hi,
                                                 const uint32_t step_arg, const uint32_t k_off,
                                                 const int32_t noise_arg, const int32_t H_arg,
                                                 const int32_t geo_arg,
                                                 const float* __restrict__ u_prev,
                                                 const JointDev* __restrict__ jtab, const DevParams pk) {
    rollout_body<MODEL, NA, NCH, LSEG, F64, VONE, XC, ONEG, false, true>(seed_lo, seed_hi, step_arg, k_off, noise_arg,
                                                                         H_arg, geo_arg, u_prev, jtab, pk);
}
// (fp64 state: budgeted for 7 waves per SIMD, the full k_rollout_s's register count (72 VGPRs) gives
// it that many; at the 4-wave budget max-ilp took 79 for the quiet body, at 7 it takes 60 with the
// same instruction count and no scratch -- profiles/r08/quiet_rollout/isa_counts.txt)
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool VONE, bool XC>
__global__ void __launch_bounds__(512, (F64 ? 7 : roll_occ<NCH, F64, XC, true>())) k_rollout_q(const uint32_t seed_lo, const uint32_t seed_hi,
                                                 const uint32_t step_arg, const uint32_t k_off,
                                                 const int32_t noise_arg, const int32_t H_arg,
                                                 const int32_t geo_arg,
                                                 const float* __restrict__ u_prev,
                                                 const JointDev* __restrict__ jtab, const DevParams pk) {
    rollout_body<MODEL, NA, NCH, LSEG, F64, VONE, XC, true, true, true>(seed_lo, seed_hi, step_arg, k_off, noise_arg,
                                                                        H_arg, geo_arg, u_prev, jtab, pk);
}

// The tracking rollout (rollout_body TRK): the extended kernel of every block size, one group or a
// loop of them, under a symbol of its own.  The target table is an extra pointer argument before the
// trailing DevParams (whose size and offsets, and every other kernel's arguments, stay as they are);
// the step counter stays the third argument.
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool VONE>
__global__ void __launch_bounds__(512, (roll_occ<NCH, F64, true, false>())) k_rollout_tt(const uint32_t seed_lo, const uint32_t seed_hi,
                                                 const uint32_t step_arg, const uint32_t k_off,
                                                 const int32_t noise_arg, const int32_t H_arg,
                                                 const int32_t geo_arg,
                                                 const float* __restrict__ u_prev,
                                                 const JointDev* __restrict__ jtab,
                                                 const float* __restrict__ ttab, const DevParams pk) {
    rollout_body<MODEL, NA, NCH, LSEG, F64, VONE, true, false, false, false, true>(seed_lo, seed_hi, step_arg, k_off, noise_arg,
                                                                                   H_arg, geo_arg, u_prev, jtab, pk, ttab);
}

// The scene rollout (rollout_body OBS): the tracking kernel with the obstacle term, under a symbol of
// its own.  The scene buffer (mppi_obstacles.h; read, and written with the clearances) is one more
// pointer argument, next to the target table and before the trailing DevParams.
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool VONE>
__global__ void __launch_bounds__(512, (roll_occ<NCH, F64, true, false>())) k_rollout_ob(const uint32_t seed_lo, const uint32_t seed_hi,
                                                 const uint32_t step_arg, const uint32_t k_off,
                                                 const int32_t noise_arg, const int32_t H_arg,
                                                 const int32_t geo_arg,
                                                 const float* __restrict__ u_prev,
                                                 const JointDev* __restrict__ jtab,
                                                 const float* __restrict__ ttab, float* __restrict__ scene,
                                                 const DevParams pk) {
    rollout_body<MODEL, NA, NCH, LSEG, F64, VONE, true, false, false, false, true, true>(seed_lo, seed_hi, step_arg, k_off, noise_arg,
                                                                                         H_arg, geo_arg, u_prev, jtab, pk, ttab, scene);
}

// The field rollout (rollout_body FLD): the scene kernel with the engine's distance field (mppi_field.h)
// as one more obstacle, under a symbol of its own.  The field buffer is one more pointer argument after
// the scene pointer and before the trailing DevParams.
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool VONE>
__global__ void __launch_bounds__(512, (roll_occ<NCH, F64, true, false>())) k_rollout_df(const uint32_t seed_lo, const uint32_t seed_hi,
                                                 const uint32_t step_arg, const uint32_t k_off,
                                                 const int32_t noise_arg, const int32_t H_arg,
                                                 const int32_t geo_arg,
                                                 const float* __restrict__ u_prev,
                                                 const JointDev* __restrict__ jtab,
                                                 const float* __restrict__ ttab, float* __restrict__ scene,
                                                 const float* __restrict__ field, const DevParams pk) {
    rollout_body<MODEL, NA, NCH, LSEG, F64, VONE, true, false, false, false, true, true, true>(seed_lo, seed_hi, step_arg, k_off, noise_arg,
                                                                                               H_arg, geo_arg, u_prev, jtab, pk, ttab, scene, field);
}

// The self rollouts (rollout_body SLF): the scene kernel (k_rollout_sc) and the field kernel (k_rollout_sf)
// with the self-collision pairs (mppi_self.h), under symbols of their own and with the arguments of the
// kernel each extends -- the pair region lies in the scene buffer.  Blocks of at most 256 threads: the
// centre column bounds a CU to about two waves per SIMD, which is what the registers are budgeted for (the
// four-chunk kernels: one, so that they too run without scratch).
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool VONE>
__global__ void __launch_bounds__(256, (NCH >= 4 ? 1 : 2)) k_rollout_sc(const uint32_t seed_lo, const uint32_t seed_hi,
                                                 const uint32_t step_arg, const uint32_t k_off,
                                                 const int32_t noise_arg, const int32_t H_arg,
                                                 const int32_t geo_arg,
                                                 const float* __restrict__ u_prev,
                                                 const JointDev* __restrict__ jtab,
                                                 const float* __restrict__ ttab, float* __restrict__ scene,
                                                 const DevParams pk) {
    rollout_body<MODEL, NA, NCH, LSEG, F64, VONE, true, false, false, false, true, true, false, true>(
        seed_lo, seed_hi, step_arg, k_off, noise_arg, H_arg, geo_arg, u_prev, jtab, pk, ttab, scene);
}
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool VONE>
__global__ void __launch_bounds__(256, (NCH >= 4 ? 1 : 2)) k_rollout_sf(const uint32_t seed_lo, const uint32_t seed_hi,
                                                 const uint32_t step_arg, const uint32_t k_off,
                                                 const int32_t noise_arg, const int32_t H_arg,
                                                 const int32_t geo_arg,
                                                 const float* __restrict__ u_prev,
                                                 const JointDev* __restrict__ jtab,
                                                 const float* __restrict__ ttab, float* __restrict__ scene,
                                                 const float* __restrict__ field, const DevParams pk) {
    rollout_body<MODEL, NA, NCH, LSEG, F64, VONE, true, false, false, false, true, true, true, true>(
        seed_lo, seed_hi, step_arg, k_off, noise_arg, H_arg, geo_arg, u_prev, jtab, pk, ttab, scene, field);
}
