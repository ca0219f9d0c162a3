// mppi_rollout_aerial.h -- the aerial manipulator's rollout body, its two kernels (k_rollout_aerial; the bounded
// k_rollout_aerial_b) and their launch, shared by mppi_rollout_aerial.hip (the plain kernel's unit; the model and the
// kernel's phases are described there) and mppi_limits.hip (the bounded one's): each unit instantiates its own kernel.
#pragma once
#include <type_traits>

#include "mppi_aerial.h"
#include "mppi_diag.h"
#include "mppi_limits.h"
#include "mppi_noise.h"
#include "mppi_quad_step.h"
#include "mppi_stores.h"

namespace {

constexpr int kAA = kAerialA;              // thrust, tau_xyz, qdd_0..6
constexpr int kAR = kAerialR;              // rollouts per dynamics wave (4 lanes each)
constexpr int kAWaves = 4;
constexpr int kAThreads = 64 * kAWaves;
constexpr int kAThreadsWide = 512;
constexpr int kAPW = kAerialPoseW;         // pose tile floats per (r, t): p(3) rpy(3) and one of padding (odd pitch)

// One rollout's part that needs no base pose (lane = t): the joints, their planes, the arm in the base frame.
struct AerialCtx {
    const float* eps_t;
    const float* u_t;
    int pitch, H, lane, tc;
    bool val;
    float dt, dt2h;
    const VehicleConst* vc;
    AerialChain chain;
};
__device__ __forceinline__ void aerial_arm_part(const AerialCtx& c, const int r, Mat34& T, const bool store,
                                                const __amdgpu_buffer_rsrc_t trs, const uint32_t toff, const uint32_t plane_b) {
    const float* er = c.eps_t + c.tc * c.pitch + r * kAA + 4;
    const float* ur = c.u_t + c.tc * kAA + 4;
    float acc[kAerialNq], q[kAerialNq];
#pragma unroll
    for (int a = 0; a < kAerialNq; ++a) {
        const float x = ur[a] + er[a];   // v = u + eps
        acc[a] = c.val ? x : 0.0f;
    }
    aerial_joints(acc, c.lane, c.dt, c.dt2h, c.vc->pos0f + 4, c.vc->vel0f + 4, q);
    if (store) {
#pragma unroll
        for (int a = 0; a < kAerialNq; ++a) traj_store(trs, toff, (uint32_t)(6 + a) * plane_b, q[a]);
    }
    aerial_arm_fk(T, c.vc->base, c.chain, q);
}

}  // namespace

// LIM (k_rollout_aerial_b; mppi_create_limits): the rotor limits on dims 0..3, as k_rollout_quad's LIM body applies
// them (mppi_limits.h): phase 1 leaves the effective noise eps' in the tile and the stored noise, the dynamics wave
// clamps the sum of its two LDS operands once more.  The joint dims 4..10 are not bounded.
template <bool VONE, bool LIT, int NWD, int NT, bool LIM = false>
__device__ __forceinline__ void rollout_aerial_body(const uint32_t seed_lo, const uint32_t seed_hi, const uint32_t step_arg,
                                                    const uint32_t k_off, const int32_t noise_arg, const int32_t H,
                                                    const float* __restrict__ u_prev, const DevParams& pk,
                                                    const float* __restrict__ lim = nullptr) {
    static_assert(NWD == 1 || NWD == kAWaves, "dynamics waves per block");
    static_assert(NT == kAThreads || (NWD == 1 && NT == kAThreadsWide), "block size");
    constexpr int QR = kAR * NWD;              // rollouts per block
    constexpr int kPitch = QR * kAA + 1;       // eps tile floats per t row (odd: the record phase's lane = t reads)
    constexpr int NH = NT / 64 - NWD;          // helper waves (0: the four-wave form)
    constexpr int NRH = NH > 0 ? (kAR + NH - 1) / NH : 1;   // rollouts a helper wave takes at the most
    extern __shared__ __attribute__((aligned(16))) float alds[];   // eps tile, u_prev, pose tile (aerial_lds_floats)
    __shared__ float e_lds[QR];
    __shared__ __attribute__((aligned(16))) float s_lds[QR];   // the costs, staged for st_dev_run
    __shared__ float wred[kAWaves][4];         // NWD > 1: the waves' (rho, eta, eta2, nan)
    __shared__ float part[NWD > 1 ? kAWaves : 1][64][kAA];   // NWD > 1: the waves' record partials (lane = t)
    const DevParams& p = pk;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, v = blockIdx.y, b = blockIdx.x;
    const int32_t noise_mode = noise_arg & 0xFF;
    const uint32_t step_ctr = step_of(step_arg, noise_arg);   // (native dispatch: from the dispatch id)
    const uint32_t vkey = (uint32_t)v + ((uint32_t)noise_arg >> 16);   // fleet-wide vehicle index (k_rollout)
    const int K = p.K;
    const int kb = b * QR;                       // the block's rollouts kb .. kb+QR-1
    float* const eps_t = alds;
    float* const u_t = alds + (H + 1) * kPitch;
    float* const pose = u_t + (H + 1) * kAA;   // [QR][H+1][kAPW]
    const int PT = (H + 1) * kAPW;
    const VehicleConst& vc = VONE ? pk.vc0 : pk.vc[v];
    if (VONE && b == 0) {   // hand vc0 to the finalize (it reads vc[v])
        constexpr int kVCW = (int)(sizeof(VehicleConst) / 4);
        for (int i = tid; i < kVCW; i += NT)   // (written through: k_rollout's drain_stores)
            __hip_atomic_store((int*)pk.vc + i, i == kVcStepWord ? (int)step_ctr : ((const int*)&pk.vc0)[i],
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (+ the step: mppi_dev.h kVcStepWord)
    }
    // ---- phase 1, all waves: u_prev and the (QR x H x 11) noise tile into LDS (standard_normal_noise.py:22-29):
    //      the 11 normals of (k, t) are k_rollout's draw for 11 dims
    const float* up = u_prev + (size_t)v * H * kAA;
    for (int i = tid; i < H * kAA; i += NT) u_t[i] = ld_dev(up + i);   // (the previous finalize's; device scope)
    float llo[kLimitsN] = {0.0f, 0.0f, 0.0f, 0.0f}, lhi[kLimitsN] = {0.0f, 0.0f, 0.0f, 0.0f};   // LIM: the bounds (wave-uniform)
    if constexpr (LIM) {
#pragma unroll
        for (int a = 0; a < kLimitsN; ++a) { llo[a] = uniform_f32(lim[a]); lhi[a] = uniform_f32(lim[kLimitsN + a]); }
    }
    for (int i = tid; i < QR * H; i += NT) {
        // rollouts past K replicate sample K-1 (noise and all): the dynamics need no masks; weight 0 below
        const int r = i & (QR - 1), t = i / QR, k = kb + r;
        const bool kval = k < K;
        const int kc = kval ? k : K - 1;
        float eps[kAA];
        if (noise_mode == MPPI_NOISE_INJECTED) {
            const float* n = p.noise_in + (((size_t)v * K + kc) * H + t) * kAA;
#pragma unroll
            for (int a = 0; a < kAA; ++a) eps[a] = n[a];
        } else {
            float z[kAA];
            draw_normals<kAA>(z, k_off + (uint32_t)kc, (uint32_t)t, vkey, step_ctr, seed_lo, seed_hi);
            if (p.sigma_diag) {
#pragma unroll
                for (int a = 0; a < kAA; ++a) eps[a] = z[a] * p.sdiag[a];
            } else {
#pragma unroll
                for (int c = 0; c < kAA; ++c) {
                    float e = 0.0f;
#pragma unroll
                    for (int a = 0; a < kAA; ++a) e += z[a] * p.sigma[a * kAA + c];
                    eps[c] = e;
                }
            }
        }
        if constexpr (LIM) {   // eps -> eps' on the rotor dims, against row t of the warm start (device scope)
            float ur[kLimitsN];
#pragma unroll
            for (int a = 0; a < kLimitsN; ++a) ur[a] = ld_dev(up + t * kAA + a);
#pragma unroll
            for (int a = 0; a < kLimitsN; ++a) {
                float c;
                limits_apply(ur[a], eps[a], llo[a], lhi[a], eps[a], c);
            }
        }
        float* dst = eps_t + t * kPitch + r * kAA;
#pragma unroll
        for (int a = 0; a < kAA; ++a) dst[a] = eps[a];
        if (p.store_noise && kval) {   // (readback only: written through, st_dev)
            float* no = p.noise_out + (((size_t)v * K + k) * H + t) * kAA;
#pragma unroll
            for (int a = 0; a < kAA; ++a) st_dev(no + a, eps[a]);
        }
    }
    __syncthreads();

    // what the lanes that cost the end effector share (lane = t)
    const int hp = pk.hp;
    const uint32_t plane_b = (uint32_t)K * (uint32_t)hp * 4u;
    const bool store = p.store_traj != 0 && !(MPPI_KO & 16);
    const __amdgpu_buffer_rsrc_t trs = traj_rsrc(store ? pk.traj + (size_t)v * pk.C * K * hp : nullptr, plane_b, store ? pk.C : 0);
    const bool stl = store && lane < hp;          // the sample's row incl. its pad
    AerialCtx cx;
    cx.eps_t = eps_t; cx.u_t = u_t; cx.pitch = kPitch; cx.H = H; cx.lane = lane;
    cx.val = lane < H; cx.tc = cx.val ? lane : H - 1;
    cx.dt = p.dt; cx.dt2h = 0.5f * p.dt2; cx.vc = &vc;
    aerial_chain_load(cx.chain, p.joints, p.j0);
    const float wsp = uniform_f32(p.w_sp), wso = uniform_f32(p.w_so), wtp = uniform_f32(p.w_tp), wto = uniform_f32(p.w_to);
    // the pose of (r, t), the composition, the cost and the base and EE planes; S_r into s_lds
    auto finish = [&](const int r, const Mat34& T) {
        const float* ps = pose + r * PT + cx.tc * kAPW;
        const float pb[3] = {ps[0], ps[1], ps[2]}, eb[3] = {ps[3], ps[4], ps[5]};
        Mat34 E;
        aerial_compose(E, T, pb, eb);
        const bool term = lane == H - 1;
        const float x = pose_cost(E, vc, term ? wtp : wsp, term ? wto : wso);
        if (stl) {
            const uint32_t toff = ((uint32_t)(kb + r) * (uint32_t)hp + (uint32_t)lane) * 4u;
#pragma unroll
            for (int a = 0; a < 3; ++a) traj_store(trs, toff, (uint32_t)a * plane_b, pb[a]);
#pragma unroll
            for (int a = 0; a < 3; ++a) traj_store(trs, toff, (uint32_t)(3 + a) * plane_b, eb[a]);
#pragma unroll
            for (int i = 0; i < 12; ++i) traj_store(trs, toff, (uint32_t)(6 + kAerialNq + i) * plane_b, E.m[i]);
        }
        // S_k = sum_{t < H-1} x_t + x_{H-1} (the weights are in x)
        const float stage = wave_fold_all(lane < H - 1 ? x : 0.0f, OpAdd());
        const float tm = read_lane_f32(x, H - 1);
        if (lane == 0) s_lds[r] = stage + tm;
    };
    auto arm = [&](const int r, Mat34& T) {
        const uint32_t toff = ((uint32_t)(kb + r) * (uint32_t)hp + (uint32_t)lane) * 4u;
        aerial_arm_part(cx, r, T, stl, trs, toff, plane_b);
    };

    if (wid < NWD) {
        // ---- phase 2, the dynamics waves: lane = (rollout r, axis j), as k_rollout_quad.  Lane 3 follows axis 2
        //      bit for bit and lanes past K replicate sample K-1, so every lane writes the pose tile (duplicates
        //      write equal values to equal addresses).
        const int r = wid * kAR + (lane >> 2), j = lane & 3, jj = j < 3 ? j : 2;
        float x6[6], v6[6], ii3[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            x6[d] = uniform_f32(vc.pos0f[d]); x6[3 + d] = uniform_f32(vc.pos0f[11 + d]);
            v6[d] = uniform_f32(vc.vel0f[d]); v6[3 + d] = uniform_f32(vc.vel0f[11 + d]);
            ii3[d] = p.q_iinv[d];
        }
        auto axis = [&](const float* x3) { return lane_sel(lane_sel(x3[2], x3[1], kM1), x3[0], kM0); };
        const float dt = p.dt, im = p.q_inv_m, kd = p.q_kd;
        const float gj = (j >= 2) ? -p.q_g : 0.0f;      // g = (0, 0, -q_g)
        const float ij = axis(ii3);
        float pj = axis(x6), ej = axis(x6 + 3), vj = axis(v6), wj = axis(v6 + 3);
        const float ox0 = v6[3], oy0 = v6[4], oz0 = v6[5];   // measured body rates
        const float a0 = (j == 0) ? 1.0f : 0.0f;   // J's column 0 is (1, 0, 0)
        // v = u + eps: thrust and this axis' torque.  The LDS operands are loaded one step ahead and added at
        // their use, so the load latency hides behind a step (the tiles have a spare row H, never used).
        const float* rowp = eps_t + r * kAA;
        const float* urp = u_t;
        float pu0 = urp[0], pe0 = rowp[0], pu1 = urp[1 + jj], pe1 = rowp[1 + jj];
        float* pw = pose + r * PT + jj;
        // LIM: this lane's torque bounds (the thrust's are llo[0], lhi[0] in every lane)
        const float tlo = LIM ? axis(llo + 1) : 0.0f, thi = LIM ? axis(lhi + 1) : 0.0f;
        auto step = [&](auto first_c) {
            constexpr bool FIRST = decltype(first_c)::value;
            float thr = pu0 + pe0, tau = pu1 + pe1;
            if constexpr (LIM) { thr = limits_clamp(thr, llo[0], lhi[0]); tau = limits_clamp(tau, tlo, thi); }
            rowp += kPitch;
            urp += kAA;
            pu0 = urp[0]; pe0 = rowp[0]; pu1 = urp[1 + jj]; pe1 = rowp[1 + jj];
            quad_axis_step<LIT, FIRST>(pj, ej, vj, wj, thr, tau, dt, im, kd, gj, ij, a0, ox0, oy0, oz0);
            pw[0] = pj;
            pw[3] = ej;
            pw += kAPW;
        };
        using T_ = std::true_type;
        using F_ = std::false_type;
        step(T_{});
        int t = 1;
        for (; t + 4 <= H; t += 4) { step(F_{}); step(F_{}); step(F_{}); step(F_{}); }
        for (; t < H; ++t) step(F_{});
    }
    if constexpr (NH > 0) {
        // ---- phases 2 and 3, the helper waves: rollouts h, h + NH, ... of the block's 16
        Mat34 Th[NRH];
        const int h = wid - NWD;
        if (wid >= NWD) {
#pragma unroll
            for (int i = 0; i < NRH; ++i) {
                const int r = h + i * NH;
                if (r < kAR && kb + r < K) arm(r, Th[i]);
            }
        }
        lds_barrier();   // the pose tile is complete
        if (wid >= NWD) {
#pragma unroll
            for (int i = 0; i < NRH; ++i) {
                const int r = h + i * NH;
                if (r < kAR && kb + r < K) finish(r, Th[i]);
            }
        }
    } else {
        // the four-wave form: each wave costs the 16 rollouts it stepped (its own LDS writes: in order)
        wave_lds_handoff();
        for (int i = 0; i < kAR; ++i) {
            const int r = wid * kAR + i;
            if (kb + r < K) {
                Mat34 T;
                arm(r, T);
                finish(r, T);
            }
        }
    }
    lds_barrier();   // the costs are in s_lds
    if (wid >= NWD) { drain_stores(); return; }

    // ---- phase 4: the online softmin over the block's rollouts (mppi.py:184-188) and its record, lane
    //      (r, j) again; each dynamics wave its own 16 rollouts (k_rollout_quad's tail for 11 dims)
    const int r = wid * kAR + (lane >> 2), j = lane & 3;
    const int k = kb + r;
    const bool kval = k < K;
    const float scoef = p.coef;
    const float S = kval ? s_lds[r] : INFINITY;
    const bool mine = kval && j == 0, bad = S != S;
    float rho = wave_fold_all((mine && !bad) ? S : INFINITY, OpMin());
    float nanf = wave_fold_all(mine && bad ? 1.0f : 0.0f, OpMax());
    if constexpr (NWD > 1) {
        if (lane == 0) { wred[wid][0] = rho; wred[wid][3] = nanf; }
        lds_barrier();
#pragma unroll
        for (int w = 0; w < NWD; ++w) { rho = fminf(rho, wred[w][0]); nanf = fmaxf(nanf, wred[w][3]); }
    }
    const float e = (mine && !bad && rho < INFINITY) ? __expf(scoef * (S - rho)) : 0.0f;
    float eta = wave_fold_all(e, OpAdd()), eta2 = wave_fold_all(e * e, OpAdd());
    if (j == 0) e_lds[r] = e;
    wave_lds_handoff();
    if (!(MPPI_KO & 1024)) {   // this wave's 16 costs as one write-through 64 B run (mppi_device.h st_dev_run)
        const int k0 = kb + wid * kAR, n = min(kAR, K - k0);
        if (lane < 4) st_dev_run(uniform_ptr(p.S + (size_t)v * K), (uint32_t)k0, s_lds + wid * kAR, n, lane);
    }
    // ---- record N[a][t] = sum_k e_k eps_k[t][a], lane = t
    float n[kAA];
#pragma unroll
    for (int a = 0; a < kAA; ++a) n[a] = 0.0f;
    if (lane < H) {
        const float* row = eps_t + lane * kPitch + wid * kAR * kAA;
#pragma unroll
        for (int rr = 0; rr < kAR; ++rr) {
            const float w = e_lds[wid * kAR + rr];
#pragma unroll
            for (int a = 0; a < kAA; ++a) n[a] = fmaf(w, row[rr * kAA + a], n[a]);
        }
    }
    if constexpr (NWD > 1) {
        if (lane == 0) { wred[wid][1] = eta; wred[wid][2] = eta2; }
        if (wid > 0 && lane < H) {
#pragma unroll
            for (int a = 0; a < kAA; ++a) part[wid][lane][a] = n[a];
        }
        lds_barrier();
        if (wid != 0) { drain_stores(); return; }
        eta = 0.0f; eta2 = 0.0f;
#pragma unroll
        for (int w = 0; w < NWD; ++w) { eta += wred[w][1]; eta2 += wred[w][2]; }
        if (lane < H) {
#pragma unroll
            for (int w = 1; w < NWD; ++w) {
#pragma unroll
                for (int a = 0; a < kAA; ++a) n[a] += part[w][lane][a];
            }
        }
    }
    if (lane == 0)
        wt_store4(uniform_ptr(p.hdr), ((uint32_t)v * (uint32_t)p.nb + (uint32_t)b) * 16u, make_float4(rho, eta, eta2, nanf));
    if (lane < H) {
        float* const rdata_v = uniform_ptr(p.rdata + (size_t)v * kAA * p.nb * H);
#pragma unroll
        for (int a = 0; a < kAA; ++a)
            wt_store(rdata_v, (((uint32_t)a * (uint32_t)p.nb + (uint32_t)b) * (uint32_t)H + (uint32_t)lane) * 4u, n[a]);
    }
    drain_stores();
}

template <bool VONE, bool LIT, int NWD, int NT>
__global__ void __launch_bounds__(NT) k_rollout_aerial(const uint32_t seed_lo, const uint32_t seed_hi,
                                                       const uint32_t step_arg, const uint32_t k_off,
                                                       const int32_t noise_arg, const int32_t H,
                                                       const float* __restrict__ u_prev, const DevParams pk) {
    rollout_aerial_body<VONE, LIT, NWD, NT>(seed_lo, seed_hi, step_arg, k_off, noise_arg, H, u_prev, pk);
}

// the bounded form (a new symbol): the limits buffer as an extra pointer before the trailing DevParams
template <bool VONE, bool LIT, int NWD, int NT>
__global__ void __launch_bounds__(NT) k_rollout_aerial_b(const uint32_t seed_lo, const uint32_t seed_hi,
                                                         const uint32_t step_arg, const uint32_t k_off,
                                                         const int32_t noise_arg, const int32_t H,
                                                         const float* __restrict__ u_prev,
                                                         const float* __restrict__ lim, const DevParams pk) {
    rollout_aerial_body<VONE, LIT, NWD, NT, true>(seed_lo, seed_hi, step_arg, k_off, noise_arg, H, u_prev, pk, lim);
}

// The launch: the argument check, the LDS size and the block -- 512 threads of one dynamics wave (few
// blocks), 256 of one, or 256 of four (p->iters = dynamics waves per block).  No quiet form: every step of a
// batch runs the full kernel.  LIM: the bounded kernel of the same template arguments (a unit instantiates the
// kernels of the form it launches: the plain ones in mppi_rollout_aerial.hip, the bounded ones in mppi_limits.hip).
template <bool LIM>
inline int launch_aerial(const DevParams* p, const float* lim, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int nwd = p->iters;
    // (the layout's own: nq = 7, C = 6 + 7 + 12, hp = H rounded up to 16 -- mppi_layout.cpp)
    if (p->H > 64 || p->H < 2 || p->A != kAA || p->chain_fast != 2 || (nwd != 1 && nwd != kAWaves) || p->nb * kAR * nwd < p->K)
        return -1;
    const size_t lds = (size_t)aerial_lds_floats(p->H, nwd) * sizeof(float);
    if (lds > (size_t)kAerialLdsMax) return -1;
    const bool wide = nwd == 1 && (size_t)p->nb * p->V <= 512;
    const int shape = wide ? 0 : nwd == 1 ? 1 : 2;
    return pick<true, false>(p->V == 1, [&](auto vone) {
        return pick<true, false>(p->q_literal_jinv != 0, [&](auto lit) {
            return pick<0, 1, 2>(shape, [&](auto sh) {
                constexpr int NW = sh() == 2 ? kAWaves : 1, NT = sh() == 0 ? kAThreadsWide : kAThreads;
                if constexpr (LIM) {
                    const auto k = k_rollout_aerial_b<vone(), lit(), NW, NT>;
                    static_assert(arg_offset<2>(decltype(k)()) == kRollStepOff, "the step counter is the third argument");
                    return go(k, dim3(p->nb, p->V), dim3(NT), lds, s, p->seed_lo, p->seed_hi, p->step_ctr,
                              (uint32_t)p->k_offset, p->noise_mode, p->H, p->u_prev, lim, *p);
                } else {
                    const auto k = k_rollout_aerial<vone(), lit(), NW, NT>;
                    static_assert(arg_offset<2>(decltype(k)()) == kRollStepOff, "the step counter is the third argument");
                    return go(k, dim3(p->nb, p->V), dim3(NT), lds, s, p->seed_lo, p->seed_hi, p->step_ctr,
                              (uint32_t)p->k_offset, p->noise_mode, p->H, p->u_prev, *p);
                }
            });
        });
    });
}

