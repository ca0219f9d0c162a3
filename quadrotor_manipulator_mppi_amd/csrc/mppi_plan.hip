// mppi_plan.hip -- k_plan, the nominal plan (mppi_get_plan): the rollout of the warm start u_prev
// with zero noise, v_t = u_prev[v, t], one trajectory per vehicle.  Not part of the control step.
//
// One block per vehicle, ceil(H/64) waves, lane = horizon step t.  The double-integrator models
// (drone, arm, whole-body) integrate as k_rollout's multi-chunk path does: two fp32 DPP segment
// scans over t (seg_scan_f32_multi), wave w standing for chunk w, the carries between the 64-lane
// chunks handed on through LDS and added in the same order; the measured position is added in the
// state dtype (fp64 state -> fp64 positions and sin/cos reduction).  Each lane then runs the FK
// chain and the cost terms of its own step with the rollout's device functions (mppi_fk.h
// kin_joint, mul_affine, mul_revolute, mul_prismatic, sincos_joint, pose_cost), and the block sums
// the steps' costs.
// The quadrotor's dynamics are sequential in t: one wave per vehicle, its first four lanes stepping
// the vehicle's axes through k_rollout_quad's step (mppi_quad_step.h).
//
// Outputs (engine-owned, plain stores by the lanes): the state channels and EE rows as planes
// (V, C, H), cost_t (V, H), pos_err (V, H), S (V).
#include "mppi_fk.h"
#include "mppi_integrator.h"   // seg_scan_f32_multi
#include "mppi_obstacles.h"
#include "mppi_field.h"
#include "mppi_self.h"
#include "mppi_quad_step.h"
#include "mppi_aerial.h"
#include "mppi_limits.h"

namespace {

// The chain of one step over the rollout's joint functions (mppi_fk.h kin_joint, mul_affine,
// sincos_joint, mul_revolute, mul_prismatic), chosen at run time as the rollout's extended kernel
// chooses it (DevParams::chain_fast).  Only this dispatch and the three loops below are the plan's
// own: lifted out of rollout_body into functions both kernels call, they changed the rollout's
// register allocation (the step's code objects must stay as they are), so rollout_body keeps its
// copy.  T = base (whole-body: its position added) times the joints at pf (pd: the fp64 angles).
// at_frame(slot): called as each frame of the chain completes (slot 0: the folded base, slot 1 + j:
// after chain joint j0 + j) -- a scene engine's obstacle term (mppi_obstacles.h).
template <int MODEL, int NA, bool F64, typename AtFrame>
__device__ __forceinline__ void plan_fk(Mat34& T, const float (&pf)[NA], const double (&pd)[F64 ? NA : 1],
                                        const VehicleConst& vc, const JointDev* jnt, const DevParams& p,
                                        AtFrame&& at_frame) {
    constexpr int QOFF = (MODEL == MPPI_MODEL_WHOLEBODY) ? 3 : 0;
    constexpr int NQ = NA - QOFF;
    auto qang = [&](int j) {   // joint angle j in the state dtype
        if constexpr (F64) return pd[QOFF + j]; else return pf[QOFF + j];
    };
#pragma unroll
    for (int i = 0; i < 12; ++i) T.m[i] = vc.base[i];
    if (MODEL == MPPI_MODEL_WHOLEBODY) {
        T.m[3] += pf[0]; T.m[7] += pf[1]; T.m[11] += pf[2];
    }
    at_frame(0);
    if (NQ == 7 && p.chain_fast == 2) {   // Kinova
        kin_joint<0>(T, jnt[p.j0 + 0].O, qang(0));
        at_frame(1);
        kin_joint<1>(T, jnt[p.j0 + 1].O, qang(1));
        at_frame(2);
        kin_joint<2>(T, jnt[p.j0 + 2].O, qang(2));
        at_frame(3);
        kin_joint<3>(T, jnt[p.j0 + 3].O, qang(3));
        at_frame(4);
        kin_joint<4>(T, jnt[p.j0 + 4].O, qang(4));
        at_frame(5);
        kin_joint<5>(T, jnt[p.j0 + 5].O, qang(5));
        at_frame(6);
        kin_joint<6>(T, jnt[p.j0 + 6].O, qang(6));
        at_frame(7);
    } else if (p.chain_fast) {   // nq revolute-z joints, q_index = 0..nq-1 in order
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const JointDev& J = jnt[p.j0 + j];
            mul_affine(T, J.O);
            float s, cc;
            sincos_joint(qang(j), s, cc);
            const float omc = 1.0f - cc, r22 = cc + omc;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float a0 = T.m[4 * i], a1 = T.m[4 * i + 1];
                T.m[4 * i] = a0 * cc + a1 * s;
                T.m[4 * i + 1] = a1 * cc - a0 * s;
                T.m[4 * i + 2] = T.m[4 * i + 2] * r22;
            }
            at_frame(j + 1);
        }
    } else {
        for (int jn = p.j0; jn < p.nj; ++jn) {
            const JointDev& J = jnt[jn];
            mul_affine(T, J.O);
            if (J.type == MPPI_JOINT_FIXED) {
                at_frame(jn - p.j0 + 1);
                continue;
            }
            double qd = 0.0;
            float qf = 0.0f;
#pragma unroll
            for (int a = 0; a < NQ; ++a)
                if (a == J.q_index) {
                    qd = F64 ? pd[QOFF + a] : 0.0;
                    qf = pf[QOFF + a];
                }
            if (J.type == MPPI_JOINT_REVOLUTE) {
                float s, cc;
                if constexpr (F64) sincos_joint(qd, s, cc); else sincos_joint(qf, s, cc);
                mul_revolute(T, J, cc, s);
            } else {
                mul_prismatic(T, J, qf);
            }
            at_frame(jn - p.j0 + 1);
        }
    }
}

// The extra CostManager terms of one step before their weights and discount (cost_manager.py:83-87),
// in rollout_body's operation order.  On the controls: u_t^T Sigma^-1 v_t (covar_cost.py:20-25;
// zero noise: v_t = u_t) and ||v_t||^2 (action_cost.py:14-24).
template <int NA>
__device__ __forceinline__ float covar_form(const DevParams& p, const float (&act)[NA]) {
    float qd = 0.0f;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        float y = 0.0f;
        if (p.sigma_diag) {
            y = p.sinv[a * NA + a] * act[a];
        } else {
#pragma unroll
            for (int b = 0; b < NA; ++b) y = fmaf(p.sinv[a * NA + b], act[b], y);
        }
        qd = fmaf(act[a], y, qd);
    }
    return qd;
}
template <int NA>
__device__ __forceinline__ float action_sumsq(const float (&act)[NA]) {
    float s2 = 0.0f;
#pragma unroll
    for (int a = 0; a < NA; ++a) s2 = fmaf(act[a], act[a], s2);
    return s2;
}
// On the joints (joint_space_cost.py): sc = ||q - q_c||^2, sj = ||q - q*_t||^2 (jt = the tracking
// target's row, null = zeros), out = any joint outside its limits (compared in the state dtype).
template <int NA, int QOFF, int NQ, bool F64>
__device__ __forceinline__ void joint_terms(const float (&pf)[NA], const double (&pd)[F64 ? NA : 1],
                                            const VehicleConst& vc, const float* jt, float& sc, float& sj, bool& out) {
    sc = 0.0f; sj = 0.0f;
    out = false;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const float qj = pf[QOFF + j];
        const float dc = qj - vc.qc[j];
        sc = fmaf(dc, dc, sc);
        const float dj = qj - (jt ? jt[j] : 0.0f);
        sj = fmaf(dj, dj, sj);
        const double qd = F64 ? pd[QOFF + j] : (double)qj;
        out |= (qd < (double)vc.qlo[j]) | (qd > (double)vc.qhi[j]);
    }
}

}  // namespace

template <int MODEL, int NA, bool F64>
__global__ void __launch_bounds__(256) k_plan(const float* __restrict__ u_prev, const JointDev* __restrict__ jtab,
                                              const PlanParams pp, const DevParams pk) {
    constexpr int QOFF = (MODEL == MPPI_MODEL_WHOLEBODY) ? 3 : 0;
    constexpr int NQ = (MODEL == MPPI_MODEL_DRONE) ? 0 : NA - QOFF;
    constexpr int kJW = (int)(sizeof(JointDev) * kMaxJ / 4);
    constexpr int kVCW = (int)(sizeof(VehicleConst) / 4);
    constexpr int kMaxWaves = MPPI_MAX_HORIZON / 64;
    __shared__ JointDev jnt[kMaxJ];
    __shared__ VehicleConst vcv;
    __shared__ float tot1[kMaxWaves][NA], tot2[kMaxWaves][NA];   // the waves' scan totals (the chunk carries)
    __shared__ float wsum[kMaxWaves];
    __shared__ __attribute__((aligned(16))) float scn[kSceneLdsW + kFieldHdrW];   // a scene engine's body table and obstacles, a field engine's field header
    // a self engine's pair tables and the lanes' centre columns (mppi_self.h; pitch = the block's threads), in
    // dynamic LDS the launch sizes by the engine's paired spheres: none on every other engine
    constexpr bool kSelf = MODEL != MPPI_MODEL_DRONE;
    extern __shared__ __attribute__((aligned(16))) float plan_dyn[];
    float* const slf = plan_dyn;
    float* const scolumn = plan_dyn + kSelfHdrW;
    const DevParams& p = pk;
    const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nthr = blockDim.x, nw = nthr >> 6;
    const int H = p.H, t = tid;
    const bool val = t < H;
    const int tc = val ? t : H - 1;
    // the warm-start row of this step (the last finalize's: device scope)
    float act[NA];
    {
        const float* ur = u_prev + ((size_t)v * H + tc) * NA;
#pragma unroll
        for (int a = 0; a < NA; ++a) act[a] = ld_dev(ur + a);
#pragma unroll
        for (int a = 0; a < NA; ++a) act[a] = val ? act[a] : 0.0f;
    }
    if (MODEL != MPPI_MODEL_DRONE)
        for (int i = tid; i < kJW; i += nthr) ((int*)jnt)[i] = ((const int*)jtab)[i];
    for (int i = tid; i < kVCW; i += nthr) ((int*)&vcv)[i] = ((const int*)(pp.vc + v))[i];
    if (pp.scene)
        for (int i = tid; i < kSceneLdsW; i += nthr) scn[i] = pp.scene[i < kSceneBodyW ? i : i + v * kSceneObsW];
    if (pp.field && tid < kFieldHdrW) scn[kSceneLdsW + tid] = pp.field[tid];   // (a field engine has a scene)
    // the pair region's offset in the scene buffer (the body table's spare word; 0: not a self engine)
    const int soff = (kSelf && pp.scene && pp.self_members >= 0) ? scene_int(pp.scene + kSelfWord) : 0;
    if (soff)
        for (int i = tid; i < kSelfHdrW; i += nthr) slf[i] = pp.scene[(size_t)soff + i];
    const VehicleConst& vc = vcv;

    // ---- double integrator (standard_normal_noise.py:41-48), k_rollout's NCH > 1 arithmetic
    float posf[NA];
    double posd[F64 ? NA : 1];
    {
#pragma clang fp contract(off)
        float c1[NA], c2[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) c1[a] = act[a] * p.dt;
        seg_scan_f32_multi<64, NA>(c1);
        if (lane == 63) {
#pragma unroll
            for (int a = 0; a < NA; ++a) tot1[wid][a] = c1[a];
        }
        lds_barrier();   // (also: the joint table and the vehicle constants are staged)
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            float carry = 0.0f;   // the velocity increment at the end of the chunk before this one
            for (int w = 0; w < wid; ++w) carry = tot1[w][a] + carry;
            c1[a] += carry;
            const float h2 = act[a] * (0.5f * p.dt2);
            const float velf = c1[a] + vc.vel0f[a];
            float prev = dpp_f32<0x138, 0xF>(velf);     // wave_shr:1
            if (lane == 0) prev = (wid == 0) ? vc.vel0f[a] : carry + vc.vel0f[a];
            c2[a] = prev * p.dt + h2;
        }
        seg_scan_f32_multi<64, NA>(c2);
        if (lane == 63) {
#pragma unroll
            for (int a = 0; a < NA; ++a) tot2[wid][a] = c2[a];
        }
        lds_barrier();
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            float carry = 0.0f;
            for (int w = 0; w < wid; ++w) carry = tot2[w][a] + carry;
            c2[a] += carry;
            if (!F64) {
                posf[a] = c2[a] + vc.pos0f[a];
            } else {
                posd[a] = (double)c2[a] + vc.pos0[a];
                posf[a] = (float)posd[a];
            }
        }
    }

    // ---- FK, the step's cost and position error, the planes
    const bool term = (t == H - 1);
    float* const planes = pp.traj + (size_t)v * p.C * H;
    // this step's target: row t of a tracking engine's table (PlanParams::ttab), else the fixed one
    float tg[12];
    if (pp.ttab) {
        load_target_row<MODEL == MPPI_MODEL_DRONE>(pp.ttab + ((size_t)v * H + tc) * 12, tg);
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) tg[i] = vc.tpos[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) tg[3 + i] = vc.tR[i];
    }
    float cost, perr;
    // a scene engine's term of this step: the hinge sum and the min clearance at row time (t + 1) dt
    float oh = 0.0f, og = INFINITY;
    float sh = 0.0f, sg = INFINITY;   // a self engine's: the pairs' hinge sum and min clearance
    const float otau = (float)(t + 1) * p.dt;
    if (MODEL == MPPI_MODEL_DRONE) {
        const float dx = posf[0] - tg[0], dy = posf[1] - tg[1], dz = posf[2] - tg[2];
        cost = (term ? p.w_tp : p.w_sp) * (dx * dx + dy * dy + dz * dz);
        perr = fabsf(dx) + fabsf(dy) + fabsf(dz);
        if (pp.scene) {
            const float Td[12] = {1.0f, 0.0f, 0.0f, posf[0], 0.0f, 1.0f, 0.0f, posf[1], 0.0f, 0.0f, 1.0f, posf[2]};
            if (pp.field) obs_frame_field(Td, scn, scn + kSceneBodyW, 0, otau, scn + kSceneLdsW, pp.field + kFieldHdrW, oh, og);
            else obs_frame(Td, scn, scn + kSceneBodyW, 0, otau, oh, og);
        }
        if (val) {
#pragma unroll
            for (int a = 0; a < 3; ++a) planes[(size_t)a * H + t] = posf[a];
        }
    } else {
        Mat34 T;
        plan_fk<MODEL, NA, F64>(T, posf, posd, vc, jnt, p, [&](int slot) {
            if (soff && pp.field) obs_frame_self<true>(T.m, scn, scn + kSceneBodyW, slot, otau, scn + kSceneLdsW, pp.field + kFieldHdrW, slf,
                                                       scolumn + tid, nthr, oh, og);
            else if (soff) obs_frame_self<false>(T.m, scn, scn + kSceneBodyW, slot, otau, nullptr, nullptr, slf, scolumn + tid, nthr, oh, og);
            else if (pp.field) obs_frame_field(T.m, scn, scn + kSceneBodyW, slot, otau, scn + kSceneLdsW, pp.field + kFieldHdrW, oh, og);
            else if (pp.scene) obs_frame(T.m, scn, scn + kSceneBodyW, slot, otau, oh, og);
        });
        if (soff) self_pairs(slf, scolumn + tid, nthr, sh, sg);   // (each lane reads what it wrote: no barrier)
        cost = pose_cost_row(T, tg, term ? p.w_tp : p.w_sp, term ? p.w_to : p.w_so);
        perr = fabsf(T.m[3] - tg[0]) + fabsf(T.m[7] - tg[1]) + fabsf(T.m[11] - tg[2]);
        if (val) {
#pragma unroll
            for (int a = 0; a < NA; ++a) planes[(size_t)a * H + t] = posf[a];
#pragma unroll
            for (int i = 0; i < 12; ++i) planes[(size_t)(NA + i) * H + t] = T.m[i];
        }
        if (p.cost_terms & ~MPPI_COST_TARGET_TRACK) {   // the extra CostManager terms in the reference's order (cost_manager.py:83-87)
            const float g = p.gamma_t[tc];
            if (p.cost_terms & MPPI_COST_COVAR) cost += p.w_cov * covar_form<NA>(p, act);
            float sc = 0.0f, sj = 0.0f;
            bool out = false;
            if (p.cost_terms & (MPPI_COST_CENTER | MPPI_COST_JOINT_TRACK | MPPI_COST_JOINT_LIMIT))
                joint_terms<NA, QOFF, NQ, F64>(posf, posd, vc, p.jtraj ? p.jtraj + ((size_t)v * H + tc) * NQ : nullptr,
                                               sc, sj, out);
            if (p.cost_terms & MPPI_COST_CENTER) cost += (p.w_cen * sc) * g;
            if (p.cost_terms & MPPI_COST_JOINT_TRACK) cost += (p.w_jt * sj) * g;
            if (p.cost_terms & MPPI_COST_ACTION) cost += (p.w_act * action_sumsq<NA>(act)) * g;
            if ((p.cost_terms & MPPI_COST_JOINT_LIMIT) && out) cost += p.lim_pen * g;
        }
    }
    if (pp.scene) {   // after the CostManager terms, as the rollout adds it
        cost += obs_step_cost(scn, oh, og);
        if (val) pp.scene[(size_t)scene_int(scn + 5) + (size_t)v * H + t] = og;
    }
    if (soff) {   // after the obstacle term, as the rollout adds it
        cost += self_step_cost(slf, sh, sg);
        if (val) pp.scene[(size_t)scene_int(slf + 6) + (size_t)v * H + t] = sg;
    }
    if (val) {
        pp.cost_t[(size_t)v * H + t] = cost;
        pp.pos_err[(size_t)v * H + t] = perr;
    }
    // ---- S = sum_t cost_t: a fold per wave, the waves' sums through LDS, one lane writes
    const float ws = wave_fold_all(val ? cost : 0.0f, OpAdd());
    if (lane == 0) wsum[wid] = ws;
    lds_barrier();
    if (tid == 0) {
        float S = 0.0f;
        for (int w = 0; w < nw; ++w) S += wsum[w];
        pp.S[v] = S;
    }
}

// (the QUADROTOR and AERIAL kernels: mppi_plan_air.h)
#include "mppi_plan_air.h"

// The launch of the plan kernel for a configuration (through HIP, or described into the calling
// thread's capture target: mppi_debug_plan_kernel).
extern "C" int mppi_launch_plan(const DevParams* p, const PlanParams* pp, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    if (p->H < 1 || p->H > MPPI_MAX_HORIZON || p->V < 1) return -1;
    const dim3 grid(p->V), block(64 * ((p->H + 63) / 64));   // a block per vehicle, a lane per horizon step
    // a self engine's pair tables and centre column (mppi_self.h): at most 120 + 3 * 16 * 256 words
    if (pp->self_members > kSelfMaxMembers || (pp->self_members >= 0 && !pp->scene)) return -1;
    const size_t lds = pp->self_members >= 0 ? sizeof(float) * (size_t)(kSelfHdrW + 3 * pp->self_members * (int)block.x) : 0;
    const auto chain = [&](auto k) { return go(k, grid, block, lds, s, p->u_prev, p->joints, *pp, *p); };
    switch (p->model) {
        case MPPI_MODEL_DRONE:
            if (p->A == 3) return chain(k_plan<MPPI_MODEL_DRONE, 3, false>);
            break;
        case MPPI_MODEL_ARM:
            if (p->A == 7)
                return pick<true, false>(p->state_f64 != 0, [&](auto f64) { return chain(k_plan<MPPI_MODEL_ARM, 7, f64()>); });
            break;
        case MPPI_MODEL_WHOLEBODY:
            if (p->A == 10) return chain(k_plan<MPPI_MODEL_WHOLEBODY, 10, false>);
            break;
        case MPPI_MODEL_QUADROTOR:
            if (p->A != 4 || p->H > 64) break;
            return pick<true, false>(p->q_literal_jinv != 0, [&](auto lit) {
                return go(k_plan_quad<lit()>, grid, block, 0, s, p->u_prev, *pp, *p);
            });
        case MPPI_MODEL_AERIAL:
            if (p->A != kAerialA || p->H > 64 || pp->scene || pp->ttab) break;   // (the Kinova chain: mppi_layout.cpp)
            return pick<true, false>(p->q_literal_jinv != 0, [&](auto lit) {
                return go(k_plan_aerial<lit()>, grid, block, 0, s, p->u_prev, p->joints, *pp, *p);
            });
    }
    return -1;
}
