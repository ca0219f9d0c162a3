// mppi_engine.cpp -- the engine object of libmppi_hip.so (include/mppi_hip.h): create / destroy
// (device buffers allocated once, no allocation in a step), the per-vehicle constants baked the way
// the reference builds its tensors, state / target / warm-start uploads, readbacks and kernel
// timing.  The control step itself is mppi_step.cpp; see mppi_engine.h for the file map and
// DESIGN.md for the data layout.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mppi_elites.h"
#include "mppi_engine.h"

using namespace mppi;

namespace mppi_host {

static FinTail tail_of(const FinParams& f, int32_t mode) {
    FinTail t;
    std::memset(&t, 0, sizeof(t));
    t.coef = f.coef; t.dt = f.dt; t.dt2 = f.dt2;
    t.mode = mode; t.model = f.model; t.qoff = f.qoff; t.nq = f.nq; t.state_f64 = f.state_f64;
    t.out_dim = f.out_dim; t.window = f.window;
    t.u_prev = f.u_prev; t.vc = f.vc;
    t.out = f.out; t.u0 = f.u0; t.stats = f.stats; t.flags = f.flags; t.wraw = f.wraw; t.wsmooth = f.wsmooth;
    t.dst = f.dst; t.xbase = f.xbase; t.xslot = f.xslot; t.nslots = f.nslots; t.myslot = f.myslot; t.P = f.P;
    t.xpeers = f.xpeers; t.xlocal = f.xlocal; t.xn = f.xn; t.xme = f.xme; t.xerr = f.xerr;
    t.xstall = f.xstall; t.xovl = f.xovl; t.xdec = f.xdec;
    std::memcpy(t.sg, f.sg, sizeof(t.sg));
    return t;
}

// a shard's PACK fields (mppi_rollout) into FinParams, and into the PACK tail copy
void pack_fields(const mppi_engine* e, FinParams& f) {
    const size_t slot = (size_t)e->V * e->dp.P;
    f.mode = 1;
    f.dst = e->d_exchange ? e->d_exchange + slot * e->cfg.shard_rank : nullptr;
    f.xbase = e->d_exchange; f.xslot = (int64_t)slot;
    f.nslots = e->cfg.shard_count; f.myslot = e->cfg.shard_rank;
}

Tails tails_of(const mppi_engine* e) {
    Tails r;
    // FINAL, the step's: it stores no readback copies of w_eps (mppi_get_weighted_noise recomputes
    // them from the last step's records, READBACK), so the step's tail carries no extra stores
    FinTail& fin = r.t[kTailFinal] = tail_of(e->fp, 0);
    fin.wraw = nullptr;
    fin.wsmooth = nullptr;
    FinParams pk = e->fp;
    pack_fields(e, pk);
    r.t[kTailPack] = tail_of(pk, 1);
    // SCRATCH: FINAL with its outputs and its sticky word in device scratch (mppi_kernel_timing, probes)
    FinTail& scr = r.t[kTailScratch] = fin;
    bind_outputs(scr, e->d_out, e);
    scr.xerr = (uint32_t*)(e->d_out + off_xerr(e));
    r.t[kTailReadback] = tail_of(e->fp, 2);
    return r;
}

mppi_status upload_tails(mppi_engine* e, unsigned slots) {
    const Tails r = tails_of(e);
    // a finalize of an earlier step may still be reading the old tail on the engine's stream
    // (a non-blocking torch stream: the blocking copies below are not ordered against it)
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int k = 0; k < kTailSlots; ++k)
        if (slots >> k & 1u) HIP_TRY(hipMemcpy(e->d_tail + k, &r.t[k], sizeof(FinTail), hipMemcpyHostToDevice));
    return MPPI_OK;
}

mppi_status download(mppi_engine* e, void* dst, const void* src, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return MPPI_OK;
}

// the models whose planes end in the EE's twelve stored entries, and the state channels ahead of them (ARM,
// WHOLEBODY: the action dims; AERIAL: xyz, rpy, q), else all of the channels
static bool model_has_ee(const mppi_engine* e) {
    return e->cfg.model == MPPI_MODEL_ARM || e->cfg.model == MPPI_MODEL_WHOLEBODY || e->cfg.model == MPPI_MODEL_AERIAL;
}
static int state_channels(const mppi_engine* e) { return model_has_ee(e) ? e->C - 12 : e->C; }

// n steps out of SoA planes (channel stride `plane` floats; step i at offset at(i) of each) into
// rows of mppi_traj_channels floats: the state channels, then (ARM, WHOLEBODY, AERIAL) the EE's twelve
// stored entries with the row 0 0 0 1 appended
template <class At>
static void planes_to_rows(const mppi_engine* e, const float* planes, size_t plane, size_t n, At at, float* rows) {
    const int Cr = mppi_traj_channels(&e->cfg);
    const bool has_ee = model_has_ee(e);
    const int nstate = state_channels(e);
    for (size_t i = 0; i < n; ++i) {
        float* dst = rows + i * Cr;
        const float* src = planes + at(i);
        for (int c = 0; c < nstate; ++c) dst[c] = src[c * plane];
        if (has_ee) {
            float* ee = dst + nstate;
            for (int r = 0; r < 12; ++r) ee[r] = src[(nstate + r) * plane];
            ee[12] = 0.0f; ee[13] = 0.0f; ee[14] = 0.0f; ee[15] = 1.0f;
        }
    }
}

// Native batches are not ordered with the engine's HIP stream: every entry point that touches
// the device (use_device) first waits for them.
mppi_status aql_join(mppi_engine* e) {
    if (e->aql && mppi_aql::step_busy(e->aql)) {
        std::string err;
        if (mppi_aql::step_wait(e->aql, 60000, &err) != 0) return fail(MPPI_ERR_HIP, "%s", err.c_str());
    }
    return MPPI_OK;
}

mppi_status use_device(mppi_engine* e) {
    HIP_TRY(hipSetDevice(e->cfg.device));
    return aql_join(e);
}

mppi_status build_vehicle_consts(mppi_engine* e) {
    const mppi_config& c = e->cfg;
    for (int v = 0; v < e->V; ++v) {
        VehicleConst& vc = e->h_vc[v];
        std::memset(&vc, 0, sizeof(vc));
        for (int j = 0; j < kMaxJ; ++j) { vc.qc[j] = c.q_center[j]; vc.qlo[j] = c.q_lower[j]; vc.qhi[j] = c.q_upper[j]; }
        const double* s = e->state.data() + (size_t)v * e->state_dim;
        std::memcpy(vc.tpos, &e->tpos[3 * v], 3 * sizeof(float));
        std::memcpy(&vc._pad[2], &e->x_epoch, sizeof(uint32_t));   // the exchange epoch (kVcEpochWord)
        quat_xyzw_to_R(&e->tquat[4 * v], vc.tR);
        if (c.model == MPPI_MODEL_DRONE) {
            for (int a = 0; a < 3; ++a) {
                vc.pos0f[a] = (float)s[a]; vc.vel0f[a] = (float)s[3 + a];
                vc.pos0[a] = vc.pos0f[a]; vc.vel0[a] = vc.vel0f[a];
            }
        } else if (c.model == MPPI_MODEL_QUADROTOR) {   // xyz rpy | v omega (float32 tensors)
            for (int a = 0; a < 6; ++a) {
                vc.pos0f[a] = (float)s[a]; vc.vel0f[a] = (float)s[6 + a];
                vc.pos0[a] = vc.pos0f[a]; vc.vel0[a] = vc.vel0f[a];
            }
        } else if (c.model == MPPI_MODEL_AERIAL) {   // xyz rpy q | v omega qd (float32 tensors)
            // indexed so that the finalize's joint branch reads pos0f[a] / vel0f[a] of action dim a = 4 + j
            const int nq = e->nq;
            for (int a = 0; a < 3; ++a) {
                vc.pos0f[a] = (float)s[a]; vc.vel0f[a] = (float)s[6 + nq + a];
                vc.pos0f[11 + a] = (float)s[3 + a]; vc.vel0f[11 + a] = (float)s[9 + nq + a];
            }
            for (int j = 0; j < nq; ++j) {
                vc.pos0f[4 + j] = (float)s[6 + j]; vc.vel0f[4 + j] = (float)s[12 + nq + j];
            }
            for (int a = 0; a < kMaxA; ++a) { vc.pos0[a] = vc.pos0f[a]; vc.vel0[a] = vc.vel0f[a]; }
            std::memcpy(vc.base, e->fixedM, sizeof(vc.base));   // M_fixed alone: [R(rpy) | p](k,t) is the rollout's
        } else if (c.model == MPPI_MODEL_ARM) {
            float T16[16];
            base_from_xyzquat(s, c.state_f64 != 0, T16);
            mul34(T16, e->fixedM, vc.base);
            for (int a = 0; a < e->nq; ++a) {
                const double q = s[7 + a], qd = s[7 + e->nq + a];
                vc.pos0f[a] = (float)q; vc.vel0f[a] = (float)qd;
                vc.pos0[a] = c.state_f64 ? q : (double)vc.pos0f[a];
                vc.vel0[a] = c.state_f64 ? qd : (double)vc.vel0f[a];
            }
        } else {   // whole-body: base pos(3) quat(4) q(nq) base vel(3) qd(nq)
            float qf[4] = {(float)s[3], (float)s[4], (float)s[5], (float)s[6]};
            float Rq[9], ypr[3], R[9];
            quat_xyzw_to_R(qf, Rq);
            euler_zyx(Rq, ypr);
            rpy_to_R(ypr[2], ypr[1], ypr[0], R);   // transformation_matrix.py:148-187
            float B[12] = {R[0], R[1], R[2], 0.0f, R[3], R[4], R[5], 0.0f, R[6], R[7], R[8], 0.0f};
            mul34(B, e->fixedM, vc.base);    // translation column: R * M_t; p(k,t) added on device
            for (int a = 0; a < 3; ++a) {
                vc.pos0f[a] = (float)s[a]; vc.vel0f[a] = (float)s[7 + e->nq + a];
            }
            for (int a = 0; a < e->nq; ++a) {
                vc.pos0f[3 + a] = (float)s[7 + a]; vc.vel0f[3 + a] = (float)s[7 + e->nq + 3 + a];
            }
            for (int a = 0; a < e->A; ++a) { vc.pos0[a] = vc.pos0f[a]; vc.vel0[a] = vc.vel0f[a]; }
        }
    }
    return MPPI_OK;
}

// QUADROTOR outputs: the model's first step (k_rollout_quad, t = 0) under the new u[0],
// in fp32 as the device / the reference's float32 tensors: x_des = (p, rpy) and
// v_des = (v, omega) after one step (the drone returns the same pair, drone_mppi.py:168-175).
void quad_outputs(const mppi_engine* e, const double* s, const float* u0, double* out) {
    const DevParams& p = e->dp;
    const float dt = p.dt;
    float x[12];
    for (int i = 0; i < 12; ++i) x[i] = (float)s[i];
    const float sr = std::sin(x[3]), cr = std::cos(x[3]), sp = std::sin(x[4]), cp = std::cos(x[4]);
    const float sy = std::sin(x[5]), cy = std::cos(x[5]);
    const float tp = sp / cp;
    const float r02 = cy * sp * cr + sy * sr, r12 = sy * sp * cr - cy * sr, r22 = cp * cr;
    const float wx = x[9], wy = x[10], wz = x[11];
    const float dr = wx + sr * tp * wy + cr * tp * wz;
    const float dpi = cr * wy - sr * wz;
    const float dya = sr / cp * wy + cr / cp * wz;
    out[0] = x[0] + dt * x[6]; out[1] = x[1] + dt * x[7]; out[2] = x[2] + dt * x[8];
    out[3] = x[3] + dt * dr; out[4] = x[4] + dt * dpi; out[5] = x[5] + dt * dya;
    const float thr = u0[0];
    out[6] = x[6] + dt * (p.q_inv_m * (r02 * thr - p.q_kd * x[6]));
    out[7] = x[7] + dt * (p.q_inv_m * (r12 * thr - p.q_kd * x[7]));
    out[8] = x[8] + dt * (-p.q_g + p.q_inv_m * (r22 * thr - p.q_kd * x[8]));
    out[9] = wx + dt * (p.q_iinv[0] * u0[1]);
    out[10] = wy + dt * (p.q_iinv[1] * u0[2]);
    out[11] = wz + dt * (p.q_iinv[2] * u0[3]);
}

// AERIAL outputs: the base's twelve as the QUADROTOR's (its state rows xyz rpy | v omega picked out of the
// aerial state); the joints' qdes, vdes behind them are the finalize's.
void aerial_outputs(const mppi_engine* e, const double* s, const float* u0, double* out) {
    const int nq = e->nq;
    double sq[12];
    for (int i = 0; i < 6; ++i) { sq[i] = s[i]; sq[6 + i] = s[6 + nq + i]; }
    quad_outputs(e, sq, u0, out);
}

mppi_status target_rows_begin(mppi_engine* e) {
    if (e->tt_pending) {   // the previous copy out of the staging rows must be done
        HIP_TRY(hipEventSynchronize(e->ev_tt));
        e->tt_pending = false;
    }
    return MPPI_OK;
}

void target_rows_fixed(mppi_engine* e, int v) {
    float row[12];
    std::memcpy(row, &e->tpos[3 * v], 3 * sizeof(float));
    quat_xyzw_to_R(&e->tquat[4 * v], row + 3);
    for (int t = 0; t < e->H; ++t) std::memcpy(&e->h_ttab[((size_t)v * e->H + t) * 12], row, sizeof(row));
}

// (after use_device: no native batch in flight.  The copy is stream-ordered behind the HIP-launched
// steps that still read the old rows; the next step -- a HIP launch on the stream, or a native
// submission, which drains the stream first and whose first packet acquires at agent scope what the
// stream wrote -- reads the new ones.)
mppi_status upload_target_rows(mppi_engine* e, int v) {
    const size_t n = (size_t)e->H * 12;
    HIP_TRY(hipMemcpyAsync(e->d_ttab + (size_t)v * n, e->h_ttab + (size_t)v * n, n * sizeof(float), hipMemcpyHostToDevice,
                           e->stream));
    HIP_TRY(hipEventRecord(e->ev_tt, e->stream));
    e->tt_pending = true;
    return MPPI_OK;
}

mppi_status upload_consts(mppi_engine* e) {
    if (e->vc_pending) {   // the previous copy out of the staging buffer must be done
        HIP_TRY(hipEventSynchronize(e->ev_vc));
        e->vc_pending = false;
    }
    mppi_status st = build_vehicle_consts(e);
    if (st != MPPI_OK) return st;
    if (e->V == 1) return MPPI_OK;   // passed by value in the kernel arguments
    HIP_TRY(hipMemcpyAsync(e->d_vc, e->h_vc, sizeof(VehicleConst) * e->V, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(e->ev_vc, e->stream));
    e->vc_pending = true;
    return MPPI_OK;
}

hipEvent_t pool_event(mppi_engine* e) {
    if (!e->ev_pool.empty()) {
        hipEvent_t ev = e->ev_pool.back();
        e->ev_pool.pop_back();
        return ev;
    }
    hipEvent_t ev = nullptr;
    (void)hipEventCreate(&ev);
    return ev;
}

mppi_status drain_timing(mppi_engine* e) {
    for (auto* vec : {&e->roll_pairs, &e->fin_pairs}) {
        for (auto& pr : *vec) {
            HIP_TRY(hipEventSynchronize(pr.second));
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
            if (vec == &e->roll_pairs) { e->roll_ms += ms; ++e->roll_n; }
            else { e->fin_ms += ms; ++e->fin_n; }
            e->ev_pool.push_back(pr.first);
            e->ev_pool.push_back(pr.second);
        }
        vec->clear();
    }
    return MPPI_OK;
}

// ---- mppi_create's device stages (a failure leaves a half-built engine for mppi_destroy)
// a scene engine's buffer: a self engine's carries the pair region behind it (mppi_self.h)
static int64_t scene_buffer_words(const mppi_engine* e) {
    return e->has_self ? self_words(e->V, e->K, e->H) : scene_words(e->V, e->K, e->H);
}

static mppi_status allocate(mppi_engine* e) {
    const mppi_config& c = e->cfg;
    const size_t VHA = (size_t)e->V * e->H * e->A, VK = (size_t)e->V * e->K, nb = e->dp.nb;
    HIP_TRY(hipSetDevice(c.device));
    HIP_TRY(hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
    e->stream = e->own_stream;
    HIP_TRY(hipEventCreateWithFlags(&e->ev_vc, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_out, hipEventDisableTiming));
    HIP_TRY(hipMalloc(&e->d_joints, sizeof(JointDev) * kMaxJ));
    HIP_TRY(hipMalloc(&e->d_vc, sizeof(VehicleConst) * e->V));
    HIP_TRY(hipMalloc(&e->d_u_prev, sizeof(float) * VHA));
    HIP_TRY(hipMalloc(&e->d_S, sizeof(float) * VK));
    HIP_TRY(hipMalloc(&e->d_w, sizeof(float) * VK));
    HIP_TRY(hipMalloc(&e->d_hdr, sizeof(float) * e->V * nb * 4));
    HIP_TRY(hipMalloc(&e->d_rdata, sizeof(float) * e->V * e->A * nb * e->H));
    HIP_TRY(hipMalloc(&e->d_wraw, sizeof(float) * VHA));
    HIP_TRY(hipMalloc(&e->d_wsmooth, sizeof(float) * VHA));
    if (c.store_trajectory) HIP_TRY(hipMalloc(&e->d_traj, sizeof(float) * traj_floats(e)));
    if (c.store_noise) HIP_TRY(hipMalloc(&e->d_noise_out, sizeof(float) * VK * e->H * e->A));
    HIP_TRY(hipMalloc(&e->d_out, e->out_bytes));
    HIP_TRY(hipHostMalloc((void**)&e->h_out, e->out_bytes, hipHostMallocMapped | hipHostMallocCoherent));
    HIP_TRY(hipHostGetDevicePointer((void**)&e->h_out_dev, e->h_out, 0));
    HIP_TRY(hipMalloc(&e->d_sigma, sizeof(float) * kMaxA * kMaxA));
    if ((c.cost_terms & MPPI_COST_TARGET_TRACK) || e->has_scene) {   // the target table, its pinned staging copy and the uploads' event
        HIP_TRY(hipMalloc(&e->d_ttab, sizeof(float) * (size_t)e->V * e->H * 12));
        HIP_TRY(hipHostMalloc((void**)&e->h_ttab, sizeof(float) * (size_t)e->V * e->H * 12, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_tt, hipEventDisableTiming));
    }
    if (e->has_scene) {   // the scene buffer, the vehicles' obstacle blocks' pinned staging copy, the uploads' event
        HIP_TRY(hipMalloc(&e->d_scene, sizeof(float) * (size_t)scene_buffer_words(e)));
        HIP_TRY(hipHostMalloc((void**)&e->h_scene, sizeof(float) * (size_t)e->V * kSceneObsW, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_scene, hipEventDisableTiming));
    }
    if (e->has_field) {   // the field buffer and its pinned staging copy (header and cells), the uploads' event
        const size_t bytes = sizeof(float) * (size_t)field_words(field_voxels(e->field));
        HIP_TRY(hipMalloc(&e->d_field, bytes));
        HIP_TRY(hipHostMalloc((void**)&e->h_field, bytes, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_field, hipEventDisableTiming));
    }
    if (e->has_limits) {   // the limits buffer, its pinned staging copy, the uploads' event
        HIP_TRY(hipMalloc(&e->d_limits, sizeof(float) * kLimitsW));
        HIP_TRY(hipHostMalloc((void**)&e->h_limits, sizeof(float) * kLimitsW, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&e->ev_limits, hipEventDisableTiming));
    }
    if (c.cost_terms & ~MPPI_COST_TARGET_TRACK) {   // Sigma^-1, gamma^t, tracking target
        HIP_TRY(hipMalloc(&e->d_sinv, sizeof(float) * e->A * e->A));
        HIP_TRY(hipMalloc(&e->d_gamma, sizeof(float) * e->H));
        HIP_TRY(hipMalloc(&e->d_jtraj, sizeof(float) * (size_t)e->V * e->H * std::max(1, e->nq)));
    }
    HIP_TRY(hipHostMalloc((void**)&e->h_vc, sizeof(VehicleConst) * e->V, hipHostMallocDefault));
#ifdef MPPI_STAMPS
    if (getenv("MPPI_STAMPS")) {   // (diagnostics: an engine that cannot have them runs without)
        const size_t nwaves = (size_t)e->V * nb * (e->threads / 64);
        if (hipMalloc(&e->d_stamps, nwaves * kStamps * 8) != hipSuccess) e->d_stamps = nullptr;
        e->stamp_sum.assign(kStamps, 0.0);
        // FINAL's blocks, then a shard's PACK blocks (mppi_debug_fstamps)
        if (hipMalloc(&e->d_fstamps, 2 * (size_t)e->V * e->A * ((e->H + 7) / 8) * kStamps * 8) != hipSuccess)
            e->d_fstamps = nullptr;
        e->fstamp_sum.assign(kStamps, 0.0);
    }
#endif
    if (e->overlap) HIP_TRY(hipMalloc(&e->d_ovl, (size_t)e->V * e->A * e->fin_ts * sizeof(uint32_t)));
    HIP_TRY(hipMalloc(&e->d_tail, sizeof(FinTail) * kTailSlots));
    return MPPI_OK;
}

// EngineLayout::limits into the pinned staging copy, in the buffer's order (mppi_limits.h: lo[4], hi[4])
static void limits_stage(mppi_engine* e) {
    std::memcpy(e->h_limits, e->limits.lo, sizeof(float) * kLimitsN);
    std::memcpy(e->h_limits + kLimitsN, e->limits.hi, sizeof(float) * kLimitsN);
}

// the device pointers of dp and fp (layout_of left them null)
static void bind(mppi_engine* e) {
    DevParams& p = e->dp;
    p.sigma = e->d_sigma; p.joints = e->d_joints;
    p.sinv = e->d_sinv; p.gamma_t = e->d_gamma; p.jtraj = e->d_jtraj;
    p.vc = e->d_vc; p.u_prev = e->d_u_prev;
    p.traj = e->d_traj; p.noise_out = e->d_noise_out; p.S = e->d_S; p.hdr = e->d_hdr; p.rdata = e->d_rdata;
    p.stamps = e->d_stamps;
    FinParams& f = e->fp;
    f.u_prev = e->d_u_prev; f.vc = e->d_vc;
    bind_outputs(f, e->h_out_dev, e);
    f.xerr = (uint32_t*)(e->h_out_dev + off_xerr(e));
    f.wraw = e->d_wraw; f.wsmooth = e->d_wsmooth;
    f.stamps = e->d_fstamps;
    if (e->overlap) {   // the finalize blocks' step counters, and their count per vehicle
        f.xovl = e->d_ovl;
        p.ovl = e->d_ovl;
        p.ovl_n = e->A * e->fin_ts;
    }
    f.tail = e->d_tail + kTailFinal;
}

static mppi_status upload(mppi_engine* e) {
    const mppi_config& c = e->cfg;
    std::memset(e->h_out, 0, e->out_bytes);
    HIP_TRY(hipMemcpy(e->d_sigma, c.sigma, sizeof(float) * e->A * e->A, hipMemcpyHostToDevice));
    if (e->d_ttab) {   // every vehicle's table clear: H copies of its fixed target
        e->ttab_set.assign((size_t)e->V, 0);
        for (int v = 0; v < e->V; ++v) target_rows_fixed(e, v);
        HIP_TRY(hipMemcpy(e->d_ttab, e->h_ttab, sizeof(float) * (size_t)e->V * e->H * 12, hipMemcpyHostToDevice));
        e->batch.ttab = e->call.ttab = e->d_ttab;
    }
    if (e->d_scene) {   // the body table; every vehicle without obstacles (zero words: n = 0)
        HIP_TRY(hipMemset(e->d_scene, 0, sizeof(float) * (size_t)scene_buffer_words(e)));
        HIP_TRY(hipMemcpy(e->d_scene, e->scene_body.data(), sizeof(float) * kSceneBodyW, hipMemcpyHostToDevice));
        if (e->has_self) {   // the pair region's header and tables (the body table's word kSelfWord holds its offset)
            HIP_TRY(hipMemcpy(e->d_scene + self_off(e->V, e->K, e->H), e->self_region.data(), sizeof(float) * kSelfHdrW, hipMemcpyHostToDevice));
            e->batch.self_members = e->call.self_members = e->self_members;
        }
        std::memset(e->h_scene, 0, sizeof(float) * (size_t)e->V * kSceneObsW);
        e->batch.scene = e->call.scene = e->d_scene;
    }
    if (e->d_field) {   // cleared: the header with the set flag off, zero cells
        std::memset(e->h_field, 0, sizeof(float) * (size_t)field_words(field_voxels(e->field)));
        field_header(e->field, e->field.origin, false, e->h_field);
        HIP_TRY(hipMemcpy(e->d_field, e->h_field, sizeof(float) * (size_t)field_words(field_voxels(e->field)), hipMemcpyHostToDevice));
        e->batch.field = e->call.field = e->d_field;
    }
    if (e->d_limits) {   // the bounds given at creation
        limits_stage(e);
        HIP_TRY(hipMemcpy(e->d_limits, e->h_limits, sizeof(float) * kLimitsW, hipMemcpyHostToDevice));
        e->batch.limits = e->call.limits = e->d_limits;
    }
    if (c.cost_terms & ~MPPI_COST_TARGET_TRACK) {
        HIP_TRY(hipMemcpy(e->d_sinv, e->sinv.data(), sizeof(float) * e->sinv.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->d_gamma, e->gamma_t.data(), sizeof(float) * e->gamma_t.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(e->d_jtraj, 0, sizeof(float) * (size_t)e->V * e->H * std::max(1, e->nq)));
    }
    if (e->d_ovl) HIP_TRY(hipMemset(e->d_ovl, 0, (size_t)e->V * e->A * e->fin_ts * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(e->d_joints, e->joints, sizeof(e->joints), hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(e->d_u_prev, 0, sizeof(float) * e->V * e->H * e->A, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_out, 0, e->out_bytes, e->stream));
    // the finalize's tail parameters, one device copy per launch kind (after the stream's memsets)
    return upload_tails(e, (1u << kTailSlots) - 1u);
}

}  // namespace mppi_host

using namespace mppi_host;

static mppi_status create_engine(const mppi_config* cfg, const mppi_scene* scene, const mppi_field_desc* field, mppi_engine** out,
                                 const mppi_self_collision* self = nullptr, const mppi_limits* limits = nullptr);

extern "C" {

mppi_status mppi_create(const mppi_config* cfg, mppi_engine** out) { return mppi_create_scene(cfg, nullptr, out); }

mppi_status mppi_create_scene(const mppi_config* cfg, const mppi_scene* scene, mppi_engine** out) {
    return create_engine(cfg, scene, nullptr, out);
}

mppi_status mppi_create_scene_field(const mppi_config* cfg, const mppi_scene* scene, const mppi_field_desc* field,
                                    mppi_engine** out) {
    if (!cfg || !out) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    mppi_status st = validate(*cfg);
    if (st != MPPI_OK) return st;
    mppi_scene use;
    if ((st = field_engine_validate(*cfg, scene, field, use)) != MPPI_OK) return st;
    return create_engine(cfg, &use, field, out);
}

mppi_status mppi_create_scene_self(const mppi_config* cfg, const mppi_scene* scene, const mppi_field_desc* field,
                                   const mppi_self_collision* self, mppi_engine** out) {
    if (!cfg || !out) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    mppi_status st = validate(*cfg);
    if (st != MPPI_OK) return st;
    mppi_scene use;
    if ((st = self_engine_validate(*cfg, scene, field, self, use)) != MPPI_OK) return st;
    return create_engine(cfg, &use, field, out, self);
}

// An engine with rotor limits (include/mppi_hip.h; NULL limits: mppi_create): QUADROTOR and AERIAL, the bounded kernels.
mppi_status mppi_create_limits(const mppi_config* cfg, const mppi_limits* limits, mppi_engine** out) {
    return create_engine(cfg, nullptr, nullptr, out, nullptr, limits);
}

// The bounds replaced: validated, staged and uploaded as a scene engine's obstacles are (mppi_set_obstacles:
// stream-ordered before the next step on both dispatch paths).  The kernels reach the buffer through the
// pointer fixed at creation, so no resident argument block changes.
mppi_status mppi_set_limits(mppi_engine* e, const mppi_limits* limits) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (!e->has_limits) return fail(MPPI_ERR_STATE, "engine created without limits (mppi_create_limits)");
    const mppi_status st = limits_values_validate(limits);
    if (st != MPPI_OK) return st;
    if (use_device(e)) return MPPI_ERR_HIP;
    if (e->limits_pending) {   // the previous copy out of the staging copy must be done
        HIP_TRY(hipEventSynchronize(e->ev_limits));
        e->limits_pending = false;
    }
    e->limits = *limits;
    limits_stage(e);
    HIP_TRY(hipMemcpyAsync(e->d_limits, e->h_limits, sizeof(float) * kLimitsW, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(e->ev_limits, e->stream));
    e->limits_pending = true;
    return MPPI_OK;
}

mppi_status mppi_get_limits(mppi_engine* e, int32_t* has, mppi_limits* limits) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (has) *has = e->has_limits ? 1 : 0;
    if (limits && e->has_limits) *limits = e->limits;
    return MPPI_OK;
}

static mppi_status create_engine(const mppi_config* cfg, const mppi_scene* scene, const mppi_field_desc* field, mppi_engine** out,
                                 const mppi_self_collision* self, const mppi_limits* limits) {
    if (!cfg || !out) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    mppi_status st = validate(*cfg);
    if (st != MPPI_OK) return st;
    if (limits && (st = limits_validate(*cfg, limits)) != MPPI_OK) return st;
    if (scene && (st = scene_validate(*cfg, *scene)) != MPPI_OK) return st;
    if (field && (st = field_validate(field)) != MPPI_OK) return st;
    if (self && !scene) return fail(MPPI_ERR_INVALID_ARG, "self: a self engine has a scene");
    if (self && (st = self_validate(*cfg, *scene, self)) != MPPI_OK) return st;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(MPPI_ERR_INVALID_ARG, "device %d not present (%d HIP devices)", cfg->device, ndev);
    EngineLayout lay{};
    // (a self engine's block is sized by its centre column: self_layout)
    if ((st = self ? self_layout(*cfg, self_member_count(*self), lay) : layout_of(*cfg, lay)) != MPPI_OK) return st;
    if (scene) {
        lay.has_scene = true;
        lay.scene_body.assign(kSceneBodyW, 0.0f);
        int order[MPPI_MAX_BODY_SPHERES] = {0};
        scene_body_table(lay, *scene, lay.scene_body.data(), order);
        if (self) {
            lay.has_self = true;
            lay.self_region.assign(kSelfHdrW, 0.0f);
            lay.self_members = self_table(lay, *scene, *self, order, lay.self_region.data());
            const int32_t off = (int32_t)self_off(lay.V, lay.K, lay.H);
            std::memcpy(lay.scene_body.data() + kSelfWord, &off, sizeof(off));
        }
    }
    if (field) {
        lay.has_field = true;
        lay.field = *field;
    }
    if (limits) {
        lay.has_limits = true;
        lay.limits = *limits;
    }

    mppi_engine* e = new mppi_engine();
    static_cast<EngineLayout&>(*e) = std::move(lay);
    const mppi_config& c = e->cfg;
    e->tpos.assign((size_t)3 * e->V, 0.0f);
    e->fk_O.assign((size_t)16 * std::max(0, (int)c.n_joints), 0.0f);
    e->fk_ax.assign((size_t)3 * std::max(0, (int)c.n_joints), 0.0f);
    fk_consts(c.joints, c.n_joints, e->fk_O.data(), e->fk_ax.data());
    e->tquat.assign((size_t)4 * e->V, 0.0f);
    for (int v = 0; v < e->V; ++v) e->tquat[4 * v + 3] = 1.0f;
    e->state.assign((size_t)e->state_dim * e->V, 0.0);
    // the run-time switches (the ones that change the layout: layout_of)
    if (const char* dbg = getenv("MPPI_FIN_DEBUG")) e->fp.dbg = atoi(dbg);
    e->event_wait = getenv("MPPI_EVENT_WAIT") && atoi(getenv("MPPI_EVENT_WAIT")) != 0;
    e->no_flag_dbg = e->event_wait && getenv("MPPI_DEBUG_NO_FLAG") && atoi(getenv("MPPI_DEBUG_NO_FLAG")) != 0;
    e->out_dbg = getenv("MPPI_DEBUG_OUT") ? atoi(getenv("MPPI_DEBUG_OUT")) : 0;
    if (const char* d = getenv("MPPI_DISPATCH")) e->aql_mode = !strcmp(d, "hip") ? 0 : !strcmp(d, "aql") ? 1 : 2;
    // experiment (MPPI_OVERLAP=1): overlapped native batches; k_rollout only (k_rollout_quad does not wait)
    e->overlap = getenv("MPPI_OVERLAP") && atoi(getenv("MPPI_OVERLAP")) != 0 && c.model != MPPI_MODEL_QUADROTOR &&
                 c.model != MPPI_MODEL_AERIAL;

    if ((st = allocate(e)) == MPPI_OK) {
        bind(e);
        st = upload(e);
    }
    if (st != MPPI_OK) {   // (mppi_destroy leaves the error message as it is)
        mppi_destroy(e);
        return st;
    }
    *out = e;
    return MPPI_OK;
}

void mppi_destroy(mppi_engine* e) {
    if (!e) return;
    prewarm_stop(e);   // the prewarm thread first: it writes packets into the native queue
    (void)hipSetDevice(e->cfg.device);
    // the native queue first: its last batch may still write the buffers freed below (stamps
    // included).  A queue that does not drain leaves them leaked rather than freed under it.
    if (e->aql && !mppi_aql::step_destroy(e->aql)) {
        fprintf(stderr, "[mppi] mppi_destroy: the engine's native queue did not drain; its device buffers are leaked\n");
        return;
    }
    e->aql = nullptr;
    if (e->d_stamps && e->stamp_n) {
        fprintf(stderr, "[mppi stamps] rollout avg cycles per wave over %lld waves:", (long long)e->stamp_n);
        for (size_t i = 1; i < kRollStampOrder.size(); ++i)
            fprintf(stderr, " %s=%.0f", kRollStampNames[i], e->stamp_sum[i] / e->stamp_n);
        fprintf(stderr, "\n[mppi stamps] finalize avg cycles per block over %lld blocks:", (long long)e->fstamp_n);
        for (size_t i = 1; i < kFinStampOrder.size(); ++i)
            fprintf(stderr, " %s=%.0f", kFinStampNames[i], e->fstamp_sum[i] / std::max<int64_t>(1, e->fstamp_n));
        fprintf(stderr, "\n");
    }
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (auto& pr : e->roll_pairs) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& pr : e->fin_pairs) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    exchange_release(e);   // the communicator and the other ranks' mapped regions
    void* dev[] = {e->d_xregion, e->d_xpeers, e->d_sigma, e->d_joints, e->d_vc, e->d_u_prev, e->d_noise_in, e->d_traj, e->d_noise_out,
                   e->d_S, e->d_hdr, e->d_rdata, e->d_out, e->d_wraw, e->d_wsmooth, e->d_w,
                   e->d_sinv, e->d_gamma, e->d_jtraj, e->d_ttab, e->d_scene, e->d_field, e->d_xown, e->d_tail, e->d_stamps, e->d_fstamps, e->d_xstall, e->d_ovl, e->d_xdec,
                   e->d_plan_vc, e->d_plan, e->d_elite_cand, e->d_elites, e->d_edt, e->d_depth, e->d_limits};
    for (void* p : dev) if (p) (void)hipFree(p);
    if (e->h_out) (void)hipHostFree(e->h_out);
    if (e->h_vc) (void)hipHostFree(e->h_vc);
    if (e->h_plan) (void)hipHostFree(e->h_plan);
    if (e->h_ttab) (void)hipHostFree(e->h_ttab);
    if (e->ev_tt) (void)hipEventDestroy(e->ev_tt);
    if (e->h_scene) (void)hipHostFree(e->h_scene);
    if (e->ev_scene) (void)hipEventDestroy(e->ev_scene);
    if (e->h_field) (void)hipHostFree(e->h_field);
    if (e->h_depth) (void)hipHostFree(e->h_depth);
    if (e->ev_field) (void)hipEventDestroy(e->ev_field);
    if (e->h_elites) (void)hipHostFree(e->h_elites);
    if (e->h_limits) (void)hipHostFree(e->h_limits);
    if (e->ev_limits) (void)hipEventDestroy(e->ev_limits);
    if (e->ev_vc) (void)hipEventDestroy(e->ev_vc);
    if (e->ev_out) (void)hipEventDestroy(e->ev_out);
    if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
    delete e;
}

mppi_status mppi_set_stream(mppi_engine* e, void* s) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (use_device(e)) return MPPI_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->stream = s ? (hipStream_t)s : e->own_stream;
    return MPPI_OK;
}

mppi_status mppi_set_joint_trajectory(mppi_engine* e, int32_t v, const float* traj) {
    if (!e || v < 0 || v >= e->V) return fail(MPPI_ERR_INVALID_ARG, "mppi_set_joint_trajectory: bad arguments");
    if (!e->d_jtraj) return fail(MPPI_ERR_STATE, "engine created without CostManager cost_terms");
    if (use_device(e)) return MPPI_ERR_HIP;
    const size_t n = (size_t)e->H * e->nq;
    float* dst = e->d_jtraj + (size_t)v * n;
    if (traj) HIP_TRY(hipMemcpyAsync(dst, traj, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    else HIP_TRY(hipMemsetAsync(dst, 0, n * sizeof(float), e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return MPPI_OK;
}

mppi_status mppi_set_target(mppi_engine* e, int32_t v, const float* pos, const float* quat) {
    if (!e || !pos || v < 0 || v >= e->V) return fail(MPPI_ERR_INVALID_ARG, "mppi_set_target: bad arguments");
    std::memcpy(&e->tpos[3 * v], pos, 3 * sizeof(float));
    if (quat) std::memcpy(&e->tquat[4 * v], quat, 4 * sizeof(float));
    if (e->d_ttab && !e->ttab_set[v]) {   // a tracking engine's clear table follows the fixed target
        if (use_device(e)) return MPPI_ERR_HIP;
        mppi_status st = target_rows_begin(e);
        if (st != MPPI_OK) return st;
        target_rows_fixed(e, v);
        if ((st = upload_target_rows(e, v)) != MPPI_OK) return st;
    }
    if (e->state_set) {
        if (use_device(e)) return MPPI_ERR_HIP;
        return upload_consts(e);
    }
    return MPPI_OK;
}

mppi_status mppi_set_target_trajectory(mppi_engine* e, int32_t v, const float* pos, const float* quat) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (!(e->cfg.cost_terms & MPPI_COST_TARGET_TRACK)) return fail(MPPI_ERR_STATE, "engine created without MPPI_COST_TARGET_TRACK");
    if (v < 0 || v >= e->V) return fail(MPPI_ERR_INVALID_ARG, "mppi_set_target_trajectory: vehicle %d of %d", v, e->V);
    if (use_device(e)) return MPPI_ERR_HIP;
    const mppi_status st = target_rows_begin(e);
    if (st != MPPI_OK) return st;
    target_rows_fixed(e, v);   // the clear state; the orientation rows of a NULL quat_h4
    if (pos) {
        float* rows = e->h_ttab + (size_t)v * e->H * 12;
        for (int t = 0; t < e->H; ++t) {
            std::memcpy(rows + 12 * t, pos + 3 * t, 3 * sizeof(float));
            if (quat) quat_xyzw_to_R(quat + 4 * t, rows + 12 * t + 3);   // fp32, as the fixed target's tR
        }
    }
    e->ttab_set[v] = pos != nullptr;
    return upload_target_rows(e, v);
}

mppi_status mppi_set_u_prev(mppi_engine* e, const float* u) {
    if (!e || !u) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    if (use_device(e)) return MPPI_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(e->d_u_prev, u, sizeof(float) * e->V * e->H * e->A, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return MPPI_OK;
}

mppi_status mppi_get_u_prev(mppi_engine* e, float* u) {
    if (!e || !u) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    if (use_device(e)) return MPPI_ERR_HIP;
    return download(e, u, e->d_u_prev, sizeof(float) * e->V * e->H * e->A);
}

mppi_status mppi_set_state(mppi_engine* e, const double* state) {
    if (!e || !state) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    if (use_device(e)) return MPPI_ERR_HIP;
    std::memcpy(e->state.data(), state, sizeof(double) * e->state.size());
    e->state_set = true;
    return upload_consts(e);
}

mppi_status mppi_set_step_counter(mppi_engine* e, uint32_t step) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (use_device(e)) return MPPI_ERR_HIP;
    e->step_ctr = step;
    if (e->peer) {   // a new exchange epoch: words left in the regions under the old counter never match
        ++e->x_epoch;
        return build_vehicle_consts(e);   // (V == 1: the constants ride in the kernel arguments)
    }
    return MPPI_OK;
}

mppi_status mppi_get_step_counter(mppi_engine* e, uint32_t* step) {
    if (!e || !step) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    *step = e->step_ctr;
    return MPPI_OK;
}

mppi_status mppi_kernel_timing_ex(mppi_engine* e, int32_t n, double* rollout_us, double* finalize_us,
                                  double* pair_us) {
    if (!e || n <= 0 || !rollout_us || !finalize_us)
        return fail(MPPI_ERR_INVALID_ARG, "mppi_kernel_timing: bad arguments");
    if (e->cfg.noise_mode != MPPI_NOISE_PHILOX) return fail(MPPI_ERR_STATE, "mppi_kernel_timing needs device noise");
    if (!e->state_set) return fail(MPPI_ERR_STATE, "mppi_kernel_timing before mppi_set_state");
    if (sharded(e) && !e->d_exchange)
        return fail(MPPI_ERR_STATE, "mppi_kernel_timing on a shard needs its exchange buffer");
    if (use_device(e)) return MPPI_ERR_HIP;
    const size_t ub = sizeof(float) * e->V * e->H * e->A;
    float* saved = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    mppi_status st = MPPI_OK;
    DevParams p = rollout_params(e, StepPath::Hip, nullptr, false);
    p.step_ctr = e->step_ctr;
    // the timing loop's outputs go to device scratch; u_prev is restored below (the trajectory
    // and S are overwritten)
    FinParams f = finalize_params(e, FinKind::Scratch);
    if (e->out_dbg == 2) f.tail = e->d_tail + kTailFinal;   // diagnostic: outputs into mapped host memory
    float ms0 = 0.0f, ms1 = 0.0f, ms2 = 0.0f;
    int rc = 0;
#define KT_TRY(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) { st = fail(MPPI_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); goto done; } \
    } while (0)
    KT_TRY(hipMalloc(&saved, ub));
    for (auto& x : ev) KT_TRY(hipEventCreate(&x));
    KT_TRY(hipMemcpyAsync(saved, e->d_u_prev, ub, hipMemcpyDeviceToDevice, e->stream));
    KT_TRY(hipEventRecord(ev[0], e->stream));
    for (int i = 0; i < n && rc == 0; ++i) rc = launch_rollout(p, e->d_ttab, e->threads, e->stream, e->d_scene, e->d_field, e->self_members, e->d_limits);
    KT_TRY(hipEventRecord(ev[1], e->stream));
    for (int i = 0; i < n && rc == 0; ++i) rc = mppi_launch_finalize(&f, e->stream);
    KT_TRY(hipEventRecord(ev[2], e->stream));
    // the kernels as a control step runs them: rollout after finalize (u_prev and the
    // records just written, cold in the other XCDs' L2)
    for (int i = 0; i < n && rc == 0 && pair_us; ++i) {
        rc = launch_rollout(p, e->d_ttab, e->threads, e->stream, e->d_scene, e->d_field, e->self_members, e->d_limits);
        if (rc == 0) rc = mppi_launch_finalize(&f, e->stream);
    }
    KT_TRY(hipEventRecord(ev[3], e->stream));
    KT_TRY(hipMemcpyAsync(e->d_u_prev, saved, ub, hipMemcpyDeviceToDevice, e->stream));
    KT_TRY(hipStreamSynchronize(e->stream));
    if (rc != 0) { st = fail(MPPI_ERR_HIP, "kernel launch failed (%d)", rc); goto done; }
    KT_TRY(hipEventElapsedTime(&ms0, ev[0], ev[1]));
    KT_TRY(hipEventElapsedTime(&ms1, ev[1], ev[2]));
    KT_TRY(hipEventElapsedTime(&ms2, ev[2], ev[3]));
    *rollout_us = 1e3 * ms0 / n;
    *finalize_us = 1e3 * ms1 / n;
    if (pair_us) *pair_us = 1e3 * ms2 / n;
#undef KT_TRY
done:
    for (auto x : ev) if (x) (void)hipEventDestroy(x);
    if (saved) (void)hipFree(saved);
    return st;
}

#ifdef MPPI_PROBE
// tools-only (MPPI_PROBE builds): average time of n repetitions of a kernel sequence
//   mode 0: rollout, empty kernel   1: rollout, rollout of one block   2: rollout, finalize
//   3: empty kernel                 4: rollout of one block            5: rollout
extern "C" int mppi_launch_boundary(float* scratch, int blocks, void* stream);
extern "C" mppi_status mppi_probe_sequence(mppi_engine* e, int32_t n, int32_t mode, double* us) {
    if (use_device(e)) return MPPI_ERR_HIP;
    DevParams p = rollout_params(e, StepPath::Hip, nullptr, false);
    p.step_ctr = e->step_ctr;
    DevParams p1 = p;
    p1.nb = 1;
    const FinParams f = finalize_params(e, FinKind::Scratch);
    const int fb = 8 * ((e->A + 7) / 8) * ((e->H + 7) / 8) * e->V;
    hipEvent_t a, b;
    (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    (void)hipEventRecord(a, e->stream);
    for (int i = 0; i < n; ++i) {
        if (mode <= 2 || mode == 5) launch_rollout(p, e->d_ttab, e->threads, e->stream, e->d_scene, e->d_field, e->self_members, e->d_limits);
        if (mode == 0 || mode == 3) mppi_launch_boundary((float*)e->d_out, fb, e->stream);
        if (mode == 1 || mode == 4) launch_rollout(p1, e->d_ttab, e->threads, e->stream, e->d_scene, e->d_field, e->self_members, e->d_limits);
        if (mode == 2) mppi_launch_finalize(&f, e->stream);
    }
    (void)hipEventRecord(b, e->stream);
    (void)hipEventSynchronize(b);
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, a, b);
    *us = 1e3 * ms / n;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    return MPPI_OK;
}
#endif

mppi_status mppi_kernel_timing(mppi_engine* e, int32_t n, double* rollout_us, double* finalize_us) {
    return mppi_kernel_timing_ex(e, n, rollout_us, finalize_us, nullptr);
}

mppi_status mppi_get_costs(mppi_engine* e, float* S) {
    if (!e || !S) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    if (use_device(e)) return MPPI_ERR_HIP;
    return download(e, S, e->d_S, sizeof(float) * e->V * e->K);
}

// The obstacles of one vehicle: validated, staged and uploaded as a tracking engine's target rows are
// (upload_target_rows: stream-ordered before the next step on both dispatch paths).
mppi_status mppi_set_obstacles(mppi_engine* e, int32_t v, int32_t n, const float* center, const float* radius, const float* vel) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (!e->d_scene) return fail(MPPI_ERR_STATE, "engine created without a scene (mppi_create_scene)");
    mppi_status st = obstacles_validate(e->V, v, n, center, radius, vel);
    if (st != MPPI_OK) return st;
    if (use_device(e)) return MPPI_ERR_HIP;
    if (e->scene_pending) {   // the previous copy out of the staging blocks must be done
        HIP_TRY(hipEventSynchronize(e->ev_scene));
        e->scene_pending = false;
    }
    float* const block = e->h_scene + (size_t)v * kSceneObsW;
    obstacles_fill(block, n, center, radius, vel);
    HIP_TRY(hipMemcpyAsync(e->d_scene + kSceneBodyW + (size_t)v * kSceneObsW, block, sizeof(float) * kSceneObsW,
                           hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(e->ev_scene, e->stream));
    e->scene_pending = true;
    return MPPI_OK;
}

// The engine's distance field: validated, packed into the pinned staging copy (header, then -- with data --
// the cells) and uploaded as the obstacles are.  A clear or an origin-only change moves the header alone.
mppi_status mppi_set_distance_field(mppi_engine* e, const float* origin3, const float* d_zyx) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (!e->d_field) return fail(MPPI_ERR_STATE, "engine created without a field (mppi_create_scene_field)");
    mppi_status st = field_data_validate(e->field, origin3, d_zyx);
    if (st != MPPI_OK) return st;
    if (use_device(e)) return MPPI_ERR_HIP;
    if (e->field_pending) {   // the previous copy out of the staging buffer must be done
        HIP_TRY(hipEventSynchronize(e->ev_field));
        e->field_pending = false;
    }
    if (origin3) std::memcpy(e->field.origin, origin3, sizeof(e->field.origin));
    field_header(e->field, e->field.origin, d_zyx != nullptr, e->h_field);
    if (d_zyx) field_pack(e->field, d_zyx, e->h_field + kFieldHdrW);
    const size_t words = d_zyx ? (size_t)field_words(field_voxels(e->field)) : (size_t)kFieldHdrW;
    HIP_TRY(hipMemcpyAsync(e->d_field, e->h_field, sizeof(float) * words, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(e->ev_field, e->stream));
    e->field_pending = true;
    return MPPI_OK;
}

// The field from an occupancy grid: the bytes go into the pinned staging copy behind the header (it holds
// 8 bytes per node, the occupancy needs one) and from there to the transform's scratch; the four launches
// of mppi_edt.hip write the cells, and the header's small copy -- set flag on -- is queued behind them.
// Ordered before the next step as an uploaded field is: the event guards the staging copy, and native
// dispatch drains the stream before its first packet.
mppi_status mppi_set_occupancy(mppi_engine* e, const float* origin3, const uint8_t* occ_zyx, float max_dist) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (!e->d_field) return fail(MPPI_ERR_STATE, "engine created without a field (mppi_create_scene_field)");
    mppi_status st = occupancy_validate(origin3, occ_zyx, max_dist);
    if (st != MPPI_OK) return st;
    if (use_device(e)) return MPPI_ERR_HIP;
    const int64_t nvox = field_voxels(e->field);
    if (!e->d_edt) HIP_TRY(hipMalloc(&e->d_edt, edt_scratch_bytes(nvox)));
    if (e->field_pending) {   // the previous copy out of the staging buffer must be done
        HIP_TRY(hipEventSynchronize(e->ev_field));
        e->field_pending = false;
    }
    if (origin3) std::memcpy(e->field.origin, origin3, sizeof(e->field.origin));
    field_header(e->field, e->field.origin, true, e->h_field);
    std::memcpy(e->h_field + kFieldHdrW, occ_zyx, (size_t)nvox);
    EdtParams p;
    std::memset(&p, 0, sizeof(p));
    p.g_occ = (int32_t*)e->d_edt;
    p.g_free = p.g_occ + nvox;
    uint8_t* const d_occ = (uint8_t*)(p.g_free + nvox);
    p.occ = d_occ;
    p.cells = e->d_field + kFieldHdrW;
    p.nx = e->field.dims[0]; p.ny = e->field.dims[1]; p.nz = e->field.dims[2];
    p.voxel = e->field.voxel;
    p.cap = edt_cap(e->field.dims, e->field.voxel, max_dist);
    p.window = edt_window(p.voxel, p.cap);
    HIP_TRY(hipMemcpyAsync(d_occ, e->h_field + kFieldHdrW, (size_t)nvox, hipMemcpyHostToDevice, e->stream));
    const int rc = mppi_launch_edt(&p, e->stream);
    if (rc != 0) return fail(MPPI_ERR_HIP, "occupancy transform launch failed (%d: %s)", rc,
                             rc > 0 ? hipGetErrorString((hipError_t)rc) : "no kernel for these dims");
    HIP_TRY(hipMemcpyAsync(e->d_field, e->h_field, sizeof(float) * kFieldHdrW, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(e->ev_field, e->stream));
    e->field_pending = true;
    return MPPI_OK;
}

// ---- The persistent occupancy map of a field engine: the bytes behind the transform's two int32 grids in
// d_edt, where mppi_set_occupancy uploads them.  map_ready allocates the scratch and zero-fills the map when
// no map call came before (stream-ordered); map_transform queues the transform from the map as it stands
// and the header's copy with the set flag on, exactly as mppi_set_occupancy does, and records ev_field.
static uint8_t* map_bytes(mppi_engine* e) { return (uint8_t*)e->d_edt + 2 * sizeof(int32_t) * (size_t)field_voxels(e->field); }

static mppi_status map_ready(mppi_engine* e) {
    if (e->d_edt) return MPPI_OK;
    const int64_t nvox = field_voxels(e->field);
    HIP_TRY(hipMalloc(&e->d_edt, edt_scratch_bytes(nvox)));
    HIP_TRY(hipMemsetAsync(map_bytes(e), 0, (size_t)nvox, e->stream));
    return MPPI_OK;
}

static mppi_status map_transform(mppi_engine* e, float max_dist) {
    const int64_t nvox = field_voxels(e->field);
    field_header(e->field, e->field.origin, true, e->h_field);
    EdtParams p;
    std::memset(&p, 0, sizeof(p));
    p.g_occ = (int32_t*)e->d_edt;
    p.g_free = p.g_occ + nvox;
    p.occ = map_bytes(e);
    p.cells = e->d_field + kFieldHdrW;
    p.nx = e->field.dims[0]; p.ny = e->field.dims[1]; p.nz = e->field.dims[2];
    p.voxel = e->field.voxel;
    p.cap = edt_cap(e->field.dims, e->field.voxel, max_dist);
    p.window = edt_window(p.voxel, p.cap);
    const int rc = mppi_launch_edt(&p, e->stream);
    if (rc != 0) return fail(MPPI_ERR_HIP, "occupancy transform launch failed (%d: %s)", rc,
                             rc > 0 ? hipGetErrorString((hipError_t)rc) : "no kernel for these dims");
    HIP_TRY(hipMemcpyAsync(e->d_field, e->h_field, sizeof(float) * kFieldHdrW, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(e->ev_field, e->stream));
    e->field_pending = true;
    return MPPI_OK;
}

// what mppi_integrate_depth queues once the image is in its staging buffer
static mppi_status depth_queue(mppi_engine* e, const mppi_depth_view& view, size_t pixels, float max_dist) {
    HIP_TRY(hipMemcpyAsync(e->d_depth, e->h_depth, sizeof(float) * pixels, hipMemcpyHostToDevice, e->stream));
    DepthParams p;
    depth_params(e->field, view, p);
    p.depth = e->d_depth;
    p.occ = map_bytes(e);
    const int rc = mppi_launch_depth(&p, e->stream);
    if (rc != 0) return fail(MPPI_ERR_HIP, "depth launch failed (%d: %s)", rc,
                             rc > 0 ? hipGetErrorString((hipError_t)rc) : "no kernel for this image");
    return map_transform(e, max_dist);
}

// One depth image into the map: the image goes to pinned staging of its own and from there to its device
// twin; k_depth_carve and k_depth_mark (mppi_depth.hip) update the map's bytes, the transform rebuilds the
// field from them.  Ordered before the next step as mppi_set_occupancy is.
mppi_status mppi_integrate_depth(mppi_engine* e, const mppi_depth_view* view, const float* depth_hw, float max_dist) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (!e->d_field) return fail(MPPI_ERR_STATE, "engine created without a field (mppi_create_scene_field)");
    mppi_status st = depth_validate(e->field, view, depth_hw);
    if (st != MPPI_OK) return st;
    if (std::isnan(max_dist) || (std::isinf(max_dist) && max_dist > 0.0f))
        return fail(MPPI_ERR_INVALID_ARG, "depth: max_dist %g (a finite cap, or <= 0 for none)", max_dist);
    if (use_device(e)) return MPPI_ERR_HIP;
    if (!e->h_depth) HIP_TRY(hipHostMalloc((void**)&e->h_depth, sizeof(float) * MPPI_DEPTH_MAX_PIXELS, hipHostMallocDefault));
    if (!e->d_depth) HIP_TRY(hipMalloc((void**)&e->d_depth, sizeof(float) * MPPI_DEPTH_MAX_PIXELS));
    if (e->field_pending) {   // the previous copies out of the staging buffers must be done
        HIP_TRY(hipEventSynchronize(e->ev_field));
        e->field_pending = false;
    }
    if ((st = map_ready(e)) != MPPI_OK) return st;
    const size_t pixels = (size_t)view->width * (size_t)view->height;
    std::memcpy(e->h_depth, depth_hw, sizeof(float) * pixels);
    st = depth_queue(e, *view, pixels, max_dist);
    // a failure behind the image's copy leaves no event to guard the staging buffers: wait for what was queued
    if (st != MPPI_OK) (void)hipStreamSynchronize(e->stream);
    return st;
}

// what mppi_shift_map queues.  The origin moves as soon as the shift is launched, so the bytes and the origin
// stay one map even where the transform behind them fails.
static mppi_status shift_queue(mppi_engine* e, ShiftParams& p, const float* origin, float max_dist) {
    const int64_t nvox = field_voxels(e->field);
    p.src = (const uint8_t*)e->d_edt;
    p.occ = map_bytes(e);
    HIP_TRY(hipMemcpyAsync(e->d_edt, p.occ, (size_t)nvox, hipMemcpyDeviceToDevice, e->stream));
    const int rc = mppi_launch_map_shift(&p, e->stream);
    if (rc != 0) return fail(MPPI_ERR_HIP, "map shift launch failed (%d: %s)", rc,
                             rc > 0 ? hipGetErrorString((hipError_t)rc) : "no kernel for these dims");
    std::memcpy(e->field.origin, origin, 3 * sizeof(float));
    return map_transform(e, max_dist);
}

// The window move: the map is copied into the transform's int32 scratch (which the transform that follows
// overwrites anyway), k_map_shift writes it back shifted, and the origin moves with it.
mppi_status mppi_shift_map(mppi_engine* e, const int32_t shift_xyz[3], float max_dist) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (!e->d_field) return fail(MPPI_ERR_STATE, "engine created without a field (mppi_create_scene_field)");
    ShiftParams p;
    float origin[3];
    mppi_status st = shift_validate(e->field, shift_xyz, max_dist, p, origin);
    if (st != MPPI_OK) return st;
    if (use_device(e)) return MPPI_ERR_HIP;
    if (e->field_pending) {
        HIP_TRY(hipEventSynchronize(e->ev_field));
        e->field_pending = false;
    }
    if ((st = map_ready(e)) != MPPI_OK) return st;
    st = shift_queue(e, p, origin, max_dist);
    if (st != MPPI_OK) (void)hipStreamSynchronize(e->stream);   // (as in mppi_integrate_depth)
    return st;
}

// The map as it stands on the device: its bytes into the pinned staging copy behind the header (once no
// upload reads it any more), one synchronise, and 0 or 1 handed out.
mppi_status mppi_get_occupancy(mppi_engine* e, uint8_t* occ_zyx) {
    if (!e || !occ_zyx) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    if (!e->d_field) return fail(MPPI_ERR_STATE, "engine created without a field (mppi_create_scene_field)");
    const int64_t nvox = field_voxels(e->field);
    if (!e->d_edt) {   // no map call yet: all free
        std::memset(occ_zyx, 0, (size_t)nvox);
        return MPPI_OK;
    }
    if (use_device(e)) return MPPI_ERR_HIP;
    if (e->field_pending) {
        HIP_TRY(hipEventSynchronize(e->ev_field));
        e->field_pending = false;
    }
    uint8_t* const stage = (uint8_t*)(e->h_field + kFieldHdrW);
    HIP_TRY(hipMemcpyAsync(stage, map_bytes(e), (size_t)nvox, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int64_t i = 0; i < nvox; ++i) occ_zyx[i] = stage[i] != 0;
    return MPPI_OK;
}

// The field as it stands on the device: the whole buffer into the pinned staging copy (once no upload
// reads it any more), one synchronise, and the first word of every x-pair handed out.
mppi_status mppi_get_distance_field(mppi_engine* e, int32_t* is_set, float* origin3, float* d_zyx) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (!e->d_field) return fail(MPPI_ERR_STATE, "engine created without a field (mppi_create_scene_field)");
    if (use_device(e)) return MPPI_ERR_HIP;
    if (e->field_pending) {
        HIP_TRY(hipEventSynchronize(e->ev_field));
        e->field_pending = false;
    }
    const int64_t nvox = field_voxels(e->field);
    const size_t words = d_zyx ? (size_t)field_words(nvox) : (size_t)kFieldHdrW;
    HIP_TRY(hipMemcpyAsync(e->h_field, e->d_field, sizeof(float) * words, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (is_set) std::memcpy(is_set, e->h_field + 7, sizeof(*is_set));
    if (origin3) std::memcpy(origin3, e->h_field, 3 * sizeof(float));
    const float* const cells = e->h_field + kFieldHdrW;
    for (int64_t i = 0; d_zyx && i < nvox; ++i) d_zyx[i] = cells[2 * i];
    return MPPI_OK;
}

mppi_status mppi_get_clearances(mppi_engine* e, float* clr) {
    if (!e || !clr) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    if (!e->d_scene) return fail(MPPI_ERR_STATE, "engine created without a scene (mppi_create_scene)");
    if (use_device(e)) return MPPI_ERR_HIP;
    return download(e, clr, e->d_scene + scene_clr_off(e->V), sizeof(float) * e->V * e->K);
}

mppi_status mppi_get_plan_clearance(mppi_engine* e, float* clr) {
    if (!e || !clr) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    if (!e->d_scene) return fail(MPPI_ERR_STATE, "engine created without a scene (mppi_create_scene)");
    const mppi_status st = mppi_get_plan(e, nullptr, nullptr, nullptr, nullptr);   // k_plan writes the steps' clearances
    if (st != MPPI_OK) return st;
    return download(e, clr, e->d_scene + scene_plan_off(e->V, e->K), sizeof(float) * e->V * e->H);
}

mppi_status mppi_get_self_clearances(mppi_engine* e, float* sclr) {
    if (!e || !sclr) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    if (!e->has_self) return fail(MPPI_ERR_STATE, "engine created without self-collision pairs (mppi_create_scene_self)");
    if (use_device(e)) return MPPI_ERR_HIP;
    return download(e, sclr, e->d_scene + self_clr_off(e->V, e->K, e->H), sizeof(float) * e->V * e->K);
}

mppi_status mppi_get_plan_self_clearance(mppi_engine* e, float* sclr) {
    if (!e || !sclr) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    if (!e->has_self) return fail(MPPI_ERR_STATE, "engine created without self-collision pairs (mppi_create_scene_self)");
    const mppi_status st = mppi_get_plan(e, nullptr, nullptr, nullptr, nullptr);   // k_plan writes the steps' self clearances
    if (st != MPPI_OK) return st;
    return download(e, sclr, e->d_scene + self_plan_off(e->V, e->K, e->H), sizeof(float) * e->V * e->H);
}

mppi_status mppi_get_weights(mppi_engine* e, float* w) {
    if (!e || !w) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    if (use_device(e)) return MPPI_ERR_HIP;
    int rc = mppi_launch_weights(e->d_S, e->fp.stats, e->d_w, e->V, e->K, e->dp.coef, e->stream);
    if (rc) return fail(MPPI_ERR_HIP, "weights launch failed (%d)", rc);
    return download(e, w, e->d_w, sizeof(float) * e->V * e->K);
}

mppi_status mppi_get_noise(mppi_engine* e, float* eps) {
    if (!e || !eps) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    if (!e->d_noise_out) return fail(MPPI_ERR_STATE, "engine created without store_noise");
    if (use_device(e)) return MPPI_ERR_HIP;
    return download(e, eps, e->d_noise_out, sizeof(float) * (size_t)e->V * e->K * e->H * e->A);
}

mppi_status mppi_get_trajectory(mppi_engine* e, float* traj) {
    if (!e || !traj) return fail(MPPI_ERR_INVALID_ARG, "null argument");
    if (!e->d_traj) return fail(MPPI_ERR_STATE, "engine created without store_trajectory");
    if (use_device(e)) return MPPI_ERR_HIP;
    const size_t KH = (size_t)e->K * e->H, n = traj_floats(e);
    const size_t hp = (size_t)traj_pitch(e), plane = n / ((size_t)e->V * e->C);   // padded plane
    std::vector<float> soa(n);
    if (download(e, soa.data(), e->d_traj, n * sizeof(float))) return MPPI_ERR_HIP;
    const size_t Cr = mppi_traj_channels(&e->cfg), H = e->H;
    const bool t_major = e->cfg.model == MPPI_MODEL_QUADROTOR;   // (V,C,H,K) planes (k_rollout_quad)
    for (size_t v = 0; v < (size_t)e->V; ++v)
        planes_to_rows(e, soa.data() + v * e->C * plane, plane, KH,
                       [&](size_t i) { return t_major ? (i % H) * hp + i / H : (i / H) * hp + i % H; },
                       traj + v * KH * Cr);
    return MPPI_OK;
}

mppi_status mppi_get_weighted_noise(mppi_engine* e, float* raw, float* smoothed) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (use_device(e)) return MPPI_ERR_HIP;
    const size_t n = sizeof(float) * e->V * e->H * e->A;
    // w_eps and its SavGol of the records the last step combined (its block records, or the
    // shard's all-reduced exchange slots): k_finalize in READBACK mode, which writes only these.
    // The step's own finalize stores no readback copies (no stores that only a readback needs on
    // the latency path, and none left dirty in an XCD's L2 across a native batch).
    const FinParams f = finalize_params(e, FinKind::Readback);
    const int rc = mppi_launch_finalize(&f, e->stream);
    if (rc != 0) return fail(MPPI_ERR_HIP, "weighted-noise readback launch failed (%d)", rc);
    if (raw) HIP_TRY(hipMemcpyAsync(raw, e->d_wraw, n, hipMemcpyDeviceToHost, e->stream));   // (both under one synchronise)
    if (smoothed) return download(e, smoothed, e->d_wsmooth, n);
    HIP_TRY(hipStreamSynchronize(e->stream));
    return MPPI_OK;
}

// The nominal plan: k_plan (mppi_plan.hip) on the engine's stream, ordered like the READBACK launch
// above (use_device joins a native batch first), then the copies and one synchronise.  The vehicle
// constants are the host's (build_vehicle_consts: the last state and targets set), copied into a
// buffer of the plan's own: vc[0] in device memory is whatever the last rollout handed over.
mppi_status mppi_get_plan(mppi_engine* e, float* traj, float* cost_t, float* pos_err, float* S) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (use_device(e)) return MPPI_ERR_HIP;
    const size_t V = (size_t)e->V, H = (size_t)e->H, C = (size_t)e->C;
    const size_t n_traj = V * C * H, n_vh = V * H;
    const size_t n_all = n_traj + 2 * n_vh + V;
    if (!e->h_plan) {
        if (!e->d_plan_vc) HIP_TRY(hipMalloc(&e->d_plan_vc, sizeof(VehicleConst) * V));
        if (!e->d_plan) HIP_TRY(hipMalloc(&e->d_plan, sizeof(float) * n_all));
        HIP_TRY(hipHostMalloc((void**)&e->h_plan, sizeof(float) * n_all, hipHostMallocDefault));
    }
    if (!e->state_set) {   // no state yet: the constants of the zero state and the targets as they stand
        mppi_status st = build_vehicle_consts(e);
        if (st != MPPI_OK) return st;
    }
    PlanParams pp;
    pp.vc = e->d_plan_vc;
    pp.ttab = e->d_ttab;
    pp.scene = e->d_scene;
    pp.field = e->d_field;
    pp.self_members = e->self_members;
    pp.traj = e->d_plan; pp.cost_t = pp.traj + n_traj; pp.pos_err = pp.cost_t + n_vh; pp.S = pp.pos_err + n_vh;
    HIP_TRY(hipMemcpyAsync(e->d_plan_vc, e->h_vc, sizeof(VehicleConst) * V, hipMemcpyHostToDevice, e->stream));
    // (a bounded engine: the plan of the clamped warm start, mppi_plan.hip k_plan_quad_b / k_plan_aerial_b)
    const int rc = e->d_limits ? mppi_launch_plan_b(&e->dp, &pp, e->d_limits, e->stream) : mppi_launch_plan(&e->dp, &pp, e->stream);
    if (rc != 0) return fail(MPPI_ERR_HIP, "plan launch failed (%d: %s)", rc,
                             rc > 0 ? hipGetErrorString((hipError_t)rc) : "no kernel for this model/A/H");
    // ONE copy of the block into pinned memory (each copy into the caller's pageable arrays cost
    // ~12 us of the call: profiles/r10/plan), from the first output asked for; handed out below
    const size_t first = traj ? 0 : n_traj;
    if (traj || cost_t || pos_err || S)
        HIP_TRY(hipMemcpyAsync(e->h_plan + first, e->d_plan + first, (n_all - first) * sizeof(float),
                               hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (cost_t) std::memcpy(cost_t, e->h_plan + n_traj, n_vh * sizeof(float));
    if (pos_err) std::memcpy(pos_err, e->h_plan + n_traj + n_vh, n_vh * sizeof(float));
    if (S) std::memcpy(S, e->h_plan + n_traj + 2 * n_vh, V * sizeof(float));
    // planes (V,C,H) -> (V,H,Cr), the per-(t) layout of mppi_get_trajectory
    for (size_t v = 0; traj && v < V; ++v)
        planes_to_rows(e, e->h_plan + v * C * H, H, H, [](size_t t) { return t; },
                       traj + v * H * mppi_traj_channels(&e->cfg));
    return MPPI_OK;
}

// The elites: the selection, sort and gather kernels (mppi_elites.hip) on the engine's stream, ordered
// like the plan's launch above (use_device joins a native batch first), then ONE copy of the output
// block -- idx, S, w and, when asked for, the rows, contiguous for this n -- into pinned memory, one
// synchronise, and the hand-out.  The buffers are sized for MPPI_MAX_ELITES at the first call.
mppi_status mppi_get_elites(mppi_engine* e, int32_t n, int32_t* idx, float* S, float* w, float* traj) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (n < 1 || n > MPPI_MAX_ELITES || n > e->K)
        return fail(MPPI_ERR_INVALID_ARG, "n = %d elites: 1 .. min(MPPI_MAX_ELITES = %d, K = %d)", n, MPPI_MAX_ELITES, e->K);
    if (traj && !e->d_traj) return fail(MPPI_ERR_STATE, "engine created without store_trajectory");
    if (use_device(e)) return MPPI_ERR_HIP;
    const size_t V = (size_t)e->V, H = (size_t)e->H, Cr = (size_t)mppi_traj_channels(&e->cfg);
    const size_t row = H * Cr;   // floats of one rollout
    if (!e->h_elites) {
        const size_t cap = V * MPPI_MAX_ELITES * (3 + (e->d_traj ? row : 0));
        int B;
        int64_t share;
        elite_split(e->K, &B, &share);
        if (!e->d_elite_cand) HIP_TRY(hipMalloc(&e->d_elite_cand, sizeof(unsigned long long) * V * (size_t)B * MPPI_MAX_ELITES));
        if (!e->d_elites) HIP_TRY(hipMalloc(&e->d_elites, sizeof(float) * cap));
        HIP_TRY(hipHostMalloc((void**)&e->h_elites, sizeof(float) * cap, hipHostMallocDefault));
    }
    const size_t vn = V * (size_t)n;
    const bool has_ee = model_has_ee(e);
    EliteParams p;
    std::memset(&p, 0, sizeof(p));
    p.S = e->d_S; p.stats = e->fp.stats; p.planes = traj ? e->d_traj : nullptr; p.cand = e->d_elite_cand;
    p.idx = (int32_t*)e->d_elites; p.So = e->d_elites + vn; p.w = e->d_elites + 2 * vn;
    p.rows = traj ? e->d_elites + 3 * vn : nullptr;
    p.V = e->V; p.K = e->K; p.H = e->H; p.n = n;
    p.C = e->C; p.nstate = state_channels(e); p.has_ee = has_ee; p.Cr = (int32_t)Cr;
    p.pitch = traj_pitch(e); p.t_major = e->cfg.model == MPPI_MODEL_QUADROTOR;
    p.coef = e->dp.coef;
    const int rc = mppi_launch_elites(&p, e->stream);
    if (rc != 0) return fail(MPPI_ERR_HIP, "elites launch failed (%d: %s)", rc,
                             rc > 0 ? hipGetErrorString((hipError_t)rc) : "no kernel for these shapes");
    const size_t n_all = 3 * vn + (traj ? vn * row : 0);
    HIP_TRY(hipMemcpyAsync(e->h_elites, e->d_elites, n_all * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (idx) std::memcpy(idx, e->h_elites, vn * sizeof(int32_t));
    if (S) std::memcpy(S, e->h_elites + vn, vn * sizeof(float));
    if (w) std::memcpy(w, e->h_elites + 2 * vn, vn * sizeof(float));
    if (traj) std::memcpy(traj, e->h_elites + 3 * vn, vn * row * sizeof(float));
    return MPPI_OK;
}

mppi_status mppi_enable_timing(mppi_engine* e, int32_t enable) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (use_device(e)) return MPPI_ERR_HIP;
    mppi_status st = drain_timing(e);
    if (st) return st;
    e->timing = enable != 0;
    e->roll_ms = e->fin_ms = 0.0;
    e->roll_n = e->fin_n = 0;
    return MPPI_OK;
}

mppi_status mppi_get_timing(mppi_engine* e, double* rms, double* fms, int64_t* rn, int64_t* fn) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (use_device(e)) return MPPI_ERR_HIP;
    mppi_status st = drain_timing(e);
    if (st) return st;
    if (rms) *rms = e->roll_ms;
    if (fms) *fms = e->fin_ms;
    if (rn) *rn = e->roll_n;
    if (fn) *fn = e->fin_n;
    return MPPI_OK;
}

mppi_status mppi_philox_normals(uint64_t seed, uint32_t step, int32_t vehicle, int64_t k0, int32_t K, int32_t H,
                                int32_t A, int32_t device, float* z, uint32_t* raw) {
    if (K < 1 || H < 1 || A < 1 || A > MPPI_MAX_ACTION || !z || !raw)
        return fail(MPPI_ERR_INVALID_ARG, "mppi_philox_normals: bad arguments");
    HIP_TRY(hipSetDevice(device));
    const size_t n = (size_t)K * H;
    const int nw = mppi_philox_words(A);   // raw Philox words per (k, t)
    float* dz = nullptr;
    uint32_t* dr = nullptr;
    HIP_TRY(hipMalloc(&dz, n * A * sizeof(float)));
    HIP_TRY(hipMalloc(&dr, n * nw * sizeof(uint32_t)));
    int rc = mppi_launch_philox(seed, step, vehicle, k0, K, H, A, dz, dr, nullptr);
    hipError_t e1 = hipMemcpy(z, dz, n * A * sizeof(float), hipMemcpyDeviceToHost);
    hipError_t e2 = hipMemcpy(raw, dr, n * nw * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(dz);
    (void)hipFree(dr);
    if (rc) return fail(MPPI_ERR_HIP, "philox launch failed (%d)", rc);
    if (e1 != hipSuccess || e2 != hipSuccess) return fail(MPPI_ERR_HIP, "philox copy failed");
    return MPPI_OK;
}

}  // extern "C"
