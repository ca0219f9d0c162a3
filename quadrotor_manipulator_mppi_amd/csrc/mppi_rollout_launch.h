// mppi_rollout_launch.h -- the host-side launchers of the rollout kernels (mppi_rollout.h): which
// instantiation a DevParams runs, its LDS size and its launch.  Included by the rollout units.
#pragma once
#include "mppi_rollout.h"

// The geometries the quiet rollout is instantiated for: the kernels the default shapes run (arm and
// drone at H <= 32, whole-body at H in 33..64; common kernel, one chunk).  Every other launch
// keeps the full kernel on every step.
template <int MODEL, int NCH, int LSEG, bool XC>
constexpr bool quiet_geom() {
    return !XC && NCH == 1 && LSEG == (MODEL == MPPI_MODEL_WHOLEBODY ? 64 : 32);
}

// The kernel of a launch form: FIXED = the single-group kernel at 512 threads (k_rollout_s, quiet
// k_rollout_q), else the kernel of every block size (k_rollout, quiet k_rollout_ql).
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool VONE, bool XC, bool ONEG, bool FIXED, bool QUIET>
constexpr auto rollout_kernel() {
    if constexpr (FIXED && QUIET) return k_rollout_q<MODEL, NA, NCH, LSEG, F64, VONE, XC>;
    else if constexpr (FIXED) return k_rollout_s<MODEL, NA, NCH, LSEG, F64, VONE, XC>;
    else if constexpr (QUIET) return k_rollout_ql<MODEL, NA, NCH, LSEG, F64, VONE, XC, ONEG>;
    else return k_rollout<MODEL, NA, NCH, LSEG, F64, VONE, XC, ONEG>;
}

// A launch's LDS bytes and geometry word (threads | iters << 16); false = a block the kernels do not run.
// LDS: warm start, 8 wave slots, and -- not in the quiet forms -- the block's cost runs: iters of
// them, one per group, each (threads / 64) * R floats padded to 16 B -- sized by the block's own
// waves, not by 8.
template <int NA, int NCH, int LSEG>
inline bool rollout_block(const DevParams& p, int threads, int iters, bool quiet, size_t& lds, int32_t& geo) {
    const int s_run = quiet ? 0 : iters * cost_run_stride((threads / 64) * (64 / LSEG));
    if (threads <= 0 || threads > 512 || iters < 1 || s_run > kMaxCostRun) return false;
    lds = (size_t)(((p.H * NA + 3) & ~3) + 8 * wave_slot_floats<NA, NCH, LSEG>() + s_run) * sizeof(float);
    geo = threads | (iters << 16);
    return true;
}

// The launch of all four (FIXED implies ONEG and ignores `threads`).
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool XC, bool ONEG, bool FIXED, bool QUIET>
inline int launch_rollout_k(const DevParams& p, int threads, hipStream_t s) {
    static_assert(ONEG || !FIXED, "the fixed-block kernel runs one group");
    size_t lds;
    int32_t geo;
    if (FIXED) threads = 512;
    if (!rollout_block<NA, NCH, LSEG>(p, threads, ONEG ? 1 : p.iters, QUIET, lds, geo)) return -1;
    return pick<true, false>(p.V == 1, [&](auto vone) {
        const auto k = rollout_kernel<MODEL, NA, NCH, LSEG, F64, vone(), XC, ONEG, FIXED, QUIET>();
        static_assert(arg_offset<2>(decltype(k)()) == kRollStepOff, "the step counter is the third argument");
        return go(k, dim3(p.nb, p.V), dim3(threads), lds, s, p.seed_lo, p.seed_hi, p.step_ctr, (uint32_t)p.k_offset,
                  p.noise_mode, p.H, geo, p.u_prev, p.joints, p);
    });
}

// the single-group (ONEG) variant exists for the common kernel at NCH == 1; at 512 threads, without
// the overlap experiment's wait and unless the engine asks for the kernels as they were
// (DevParams::kern, MPPI_GENERIC_KERNELS), its fixed-block form
// A launch marked quiet (quiet_launch) runs the quiet form of whichever of the three it would run,
// where that form is instantiated (quiet_geom); the full kernel otherwise.
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool XC>
inline int launch_rollout_x(const DevParams& p, int threads, hipStream_t s) {
    bool quiet = false;
    if constexpr (quiet_geom<MODEL, NCH, LSEG, XC>()) quiet = quiet_launch(p);
    if constexpr (!XC && NCH == 1)
        if (p.iters == 1) {
            if (threads == 512 && !(p.kern & kRollKernGeneric) && !(p.noise_mode & kNoiseOverlap) && p.H <= LSEG * NCH) {
                if constexpr (quiet_geom<MODEL, NCH, LSEG, XC>())
                    if (quiet) return launch_rollout_k<MODEL, NA, NCH, LSEG, F64, XC, true, true, true>(p, threads, s);
                return launch_rollout_k<MODEL, NA, NCH, LSEG, F64, XC, true, true, false>(p, threads, s);
            }
            if constexpr (quiet_geom<MODEL, NCH, LSEG, XC>())
                if (quiet) return launch_rollout_k<MODEL, NA, NCH, LSEG, F64, XC, true, false, true>(p, threads, s);
            return launch_rollout_k<MODEL, NA, NCH, LSEG, F64, XC, true, false, false>(p, threads, s);
        }
    if constexpr (quiet_geom<MODEL, NCH, LSEG, XC>())
        if (quiet) return launch_rollout_k<MODEL, NA, NCH, LSEG, F64, XC, false, false, true>(p, threads, s);
    return launch_rollout_k<MODEL, NA, NCH, LSEG, F64, XC, false, false, false>(p, threads, s);
}

// The extended (XC) instantiation carries the extra CostManager terms, a full
// (non-diagonal) Sigma and the generic FK chains: their registers would otherwise be
// reserved in the common kernel (the full zSigma product alone held the A*A Sigma in
// VGPRs; with the generic chain loops the whole-body kernel needed 98 VGPRs, without
// them 87).  The common kernel assumes a diagonal Sigma, no extra terms and the Kinova
// chain (or no chain: the drone).
template <int MODEL, int NA, int NCH, int LSEG, bool F64>
inline int launch_rollout_t(const DevParams& p, int threads, hipStream_t s) {
    const bool generic_chain = MODEL != MPPI_MODEL_DRONE && !(NA - (MODEL == MPPI_MODEL_WHOLEBODY ? 3 : 0) == 7 &&
                                                              p.chain_fast == 2);
    if (p.cost_terms || !p.sigma_diag || generic_chain)
        return launch_rollout_x<MODEL, NA, NCH, LSEG, F64, true>(p, threads, s);
    return launch_rollout_x<MODEL, NA, NCH, LSEG, F64, false>(p, threads, s);
}

// The geometry ladder: f(NCH, LSEG), as integral constants, of the launch's chunk count and segment
// length (DevParams::nch, L); -1 for any other.  H32 = false leaves out the one-segment-of-32 rung and
// its instantiations (the fp64 arm unit: that geometry lives in mppi_rollout_arm_h32.hip).
template <bool H32 = true, typename F>
inline int pick_geom(const DevParams& p, F&& f) {
    using std::integral_constant;
    if constexpr (H32)
        if (p.nch == 1 && p.L == 32) return f(integral_constant<int, 1>{}, integral_constant<int, 32>{});
    if (p.nch == 1 && p.L == 64) return f(integral_constant<int, 1>{}, integral_constant<int, 64>{});
    if (p.nch == 2) return f(integral_constant<int, 2>{}, integral_constant<int, 64>{});
    if (p.nch == 4) return f(integral_constant<int, 4>{}, integral_constant<int, 64>{});
    return -1;
}

template <int MODEL, int NA, bool F64>
inline int dispatch_geom(const DevParams& p, int threads, hipStream_t s) {
    return pick_geom(p, [&](auto nch, auto l) { return launch_rollout_t<MODEL, NA, nch(), l(), F64>(p, threads, s); });
}

// The tracking launch (DevParams::cost_terms & MPPI_COST_TARGET_TRACK): k_rollout_tt on every step
// of a batch (no quiet form), LDS as the full extended kernel's.
template <int MODEL, int NA, int NCH, int LSEG, bool F64>
inline int launch_rollout_tt(const DevParams& p, const float* ttab, int threads, hipStream_t s) {
    size_t lds;
    int32_t geo;
    if (!rollout_block<NA, NCH, LSEG>(p, threads, p.iters, false, lds, geo)) return -1;
    return pick<true, false>(p.V == 1, [&](auto vone) {
        const auto k = k_rollout_tt<MODEL, NA, NCH, LSEG, F64, vone()>;
        static_assert(arg_offset<2>(decltype(k)()) == kRollStepOff, "the step counter is the third argument");
        return go(k, dim3(p.nb, p.V), dim3(threads), lds, s, p.seed_lo, p.seed_hi, p.step_ctr, (uint32_t)p.k_offset,
                  p.noise_mode, p.H, geo, p.u_prev, p.joints, ttab, p);
    });
}

template <int MODEL, int NA, bool F64>
inline int dispatch_geom_tt(const DevParams& p, const float* ttab, int threads, hipStream_t s) {
    return pick_geom(p, [&](auto nch, auto l) { return launch_rollout_tt<MODEL, NA, nch(), l(), F64>(p, ttab, threads, s); });
}

// The scene launch (an engine of mppi_create_scene: a scene buffer, mppi_obstacles.h): k_rollout_ob on
// every step of a batch (no quiet form), with and without the tracking bit.  LDS as the tracking
// kernel's plus a second run stage, the block's clearances behind its costs.
template <int MODEL, int NA, int NCH, int LSEG, bool F64>
inline int launch_rollout_ob(const DevParams& p, const float* ttab, float* scene, int threads, hipStream_t s) {
    size_t lds;
    int32_t geo;
    if (!ttab || !scene || !rollout_block<NA, NCH, LSEG>(p, threads, p.iters, false, lds, geo)) return -1;
    lds += (size_t)p.iters * cost_run_stride((threads / 64) * (64 / LSEG)) * sizeof(float);
    return pick<true, false>(p.V == 1, [&](auto vone) {
        const auto k = k_rollout_ob<MODEL, NA, NCH, LSEG, F64, vone()>;
        static_assert(arg_offset<2>(decltype(k)()) == kRollStepOff, "the step counter is the third argument");
        return go(k, dim3(p.nb, p.V), dim3(threads), lds, s, p.seed_lo, p.seed_hi, p.step_ctr, (uint32_t)p.k_offset,
                  p.noise_mode, p.H, geo, p.u_prev, p.joints, ttab, scene, p);
    });
}

template <int MODEL, int NA, bool F64>
inline int dispatch_geom_ob(const DevParams& p, const float* ttab, float* scene, int threads, hipStream_t s) {
    return pick_geom(p, [&](auto nch, auto l) { return launch_rollout_ob<MODEL, NA, nch(), l(), F64>(p, ttab, scene, threads, s); });
}

// The field launch (an engine of mppi_create_scene_field: a scene buffer and a field buffer, mppi_field.h):
// k_rollout_df on every step of a batch (no quiet form); LDS as the scene kernel's.
template <int MODEL, int NA, int NCH, int LSEG, bool F64>
inline int launch_rollout_df(const DevParams& p, const float* ttab, float* scene, const float* field, int threads, hipStream_t s) {
    size_t lds;
    int32_t geo;
    if (!ttab || !scene || !field || threads < 64 || !rollout_block<NA, NCH, LSEG>(p, threads, p.iters, false, lds, geo)) return -1;
    lds += (size_t)p.iters * cost_run_stride((threads / 64) * (64 / LSEG)) * sizeof(float);
    return pick<true, false>(p.V == 1, [&](auto vone) {
        const auto k = k_rollout_df<MODEL, NA, NCH, LSEG, F64, vone()>;
        static_assert(arg_offset<2>(decltype(k)()) == kRollStepOff, "the step counter is the third argument");
        static_assert(arg_offset<11>(decltype(k)()) == kRollFieldOff, "the field pointer follows the scene pointer");
        return go(k, dim3(p.nb, p.V), dim3(threads), lds, s, p.seed_lo, p.seed_hi, p.step_ctr, (uint32_t)p.k_offset,
                  p.noise_mode, p.H, geo, p.u_prev, p.joints, ttab, scene, field, p);
    });
}

template <int MODEL, int NA, bool F64>
inline int dispatch_geom_df(const DevParams& p, const float* ttab, float* scene, const float* field, int threads, hipStream_t s) {
    return pick_geom(p, [&](auto nch, auto l) { return launch_rollout_df<MODEL, NA, nch(), l(), F64>(p, ttab, scene, field, threads, s); });
}

// The self launch (an engine of mppi_create_scene_self: the pair region behind its scene buffer, mppi_self.h):
// k_rollout_sc, with a field k_rollout_sf, on every step of a batch (no quiet form).  LDS as the scene
// kernel's plus a third run stage (the self clearances) and the centre column, 3 * members words per
// thread (self_dyn_lds, the figure the layout chose the block by); blocks of 64..256 threads, and
// nothing past the CU's LDS with the kernels' static part.
static_assert(sizeof(JointDev) * kMaxJ + sizeof(VehicleConst) + 4 * (kSceneLdsW + kFieldHdrW + kSelfHdrW) + 64 <= (size_t)kSelfStaticLds,
              "the self kernels' static LDS: joint table, vehicle constants, scene, field header, pair tables");
template <int MODEL, int NA, int NCH, int LSEG, bool F64, bool FLD>
inline int launch_rollout_self(const DevParams& p, const float* ttab, float* scene, const float* field, int members, int threads,
                               hipStream_t s) {
    size_t lds;
    int32_t geo;
    if (!ttab || !scene || (FLD && !field) || members < 0 || members > kSelfMaxMembers || threads < 64 || threads > 256 ||
        !rollout_block<NA, NCH, LSEG>(p, threads, p.iters, false, lds, geo))
        return -1;
    lds += (size_t)(2 * p.iters * cost_run_stride((threads / 64) * (64 / LSEG)) + 3 * members * threads) * sizeof(float);
    if ((int64_t)lds != self_dyn_lds(NA, p.H, threads, p.iters, members) || lds + kSelfStaticLds > (size_t)kSelfLdsMax) return -1;
    return pick<true, false>(p.V == 1, [&](auto vone) {
        if constexpr (FLD) {
            const auto k = k_rollout_sf<MODEL, NA, NCH, LSEG, F64, vone()>;
            static_assert(arg_offset<2>(decltype(k)()) == kRollStepOff, "the step counter is the third argument");
            static_assert(arg_offset<11>(decltype(k)()) == kRollFieldOff, "the field pointer follows the scene pointer");
            return go(k, dim3(p.nb, p.V), dim3(threads), lds, s, p.seed_lo, p.seed_hi, p.step_ctr, (uint32_t)p.k_offset,
                      p.noise_mode, p.H, geo, p.u_prev, p.joints, ttab, scene, field, p);
        } else {
            const auto k = k_rollout_sc<MODEL, NA, NCH, LSEG, F64, vone()>;
            static_assert(arg_offset<2>(decltype(k)()) == kRollStepOff, "the step counter is the third argument");
            return go(k, dim3(p.nb, p.V), dim3(threads), lds, s, p.seed_lo, p.seed_hi, p.step_ctr, (uint32_t)p.k_offset,
                      p.noise_mode, p.H, geo, p.u_prev, p.joints, ttab, scene, p);
        }
    });
}

// every model, state width and geometry of the ladder for one of the two kernels (the self units)
template <bool FLD>
inline int dispatch_self(const DevParams& p, const float* ttab, float* scene, const float* field, int members, int threads, hipStream_t s) {
    const auto geom = [&](auto model, auto na, auto f64) {
        return pick_geom(p, [&](auto nch, auto l) {
            return launch_rollout_self<model(), na(), nch(), l(), f64(), FLD>(p, ttab, scene, field, members, threads, s);
        });
    };
    using std::integral_constant;
    if (p.model == MPPI_MODEL_ARM && p.A == 7)
        return p.state_f64 ? geom(integral_constant<int, MPPI_MODEL_ARM>{}, integral_constant<int, 7>{}, std::true_type{})
                           : geom(integral_constant<int, MPPI_MODEL_ARM>{}, integral_constant<int, 7>{}, std::false_type{});
    if (p.model == MPPI_MODEL_WHOLEBODY && p.A == 10)
        return geom(integral_constant<int, MPPI_MODEL_WHOLEBODY>{}, integral_constant<int, 10>{}, std::false_type{});
    return -1;
}
