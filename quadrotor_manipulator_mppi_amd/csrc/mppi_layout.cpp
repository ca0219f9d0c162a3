// mppi_layout.cpp -- layout_of: the launch geometry, the baked tables and the kernels' parameter
// structs of a configuration, as far as they do not depend on a device address.  Pure host code (no
// HIP), so every decision that picks a kernel can be replayed without a GPU: mppi_debug_layout below
// reports them, with a hash over the two structs.  mppi_create (mppi_engine.cpp) allocates, binds the
// device pointers and uploads.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "mppi_layout.h"

using namespace mppi;

namespace mppi_host {

// L, R, nch, nb, iters and the block size into l.dp / l.threads
static mppi_status geometry(EngineLayout& l) {
    const mppi_config& c = l.cfg;
    const int H = l.H;
    const int L = (H > 32) ? 64 : 32;
    const int nch = (H + 63) / 64;
    if (nch != 1 && nch != 2 && nch != 4)
        return fail(MPPI_ERR_INVALID_ARG, "H=%d: supported horizons are <= 128 or 193..256", H);
    const int R = 64 / L;
    l.threads = c.block_threads ? c.block_threads : l.auto_threads;
    const int nw = l.threads / 64;
    const int groups = (l.K + nw * R - 1) / (nw * R);
    int nb = c.blocks_per_vehicle;
    // auto: one block per group (iters == 1: the single-group kernel) while the grid is at
    // most 512 blocks (2 per CU); above that >= 2 groups per block (the looping kernel; the
    // prologue and the block combine are amortised, fewer records for the finalize),
    // capped at 1024 blocks in total.  Re-measured on MI355X in round 5 (tools/probes.py geom,
    // profiles/r05/geom): WB K=8192 step pair 17.6 us at 512 looping blocks vs 19.5-20.7 at 1024
    // single-group blocks (whose finalize also reads twice the records) and 18.3 at 256; K=65536
    // best at 1024 (85.2-86.1 us pairs vs 87.6-92.9 at 512, 89.1+ with 256-thread blocks).
    if (nb <= 0) {
        nb = (groups * l.V <= 512) ? groups : std::min(std::max(1, groups / 2), std::max(1, 1024 / l.V));
    }
    nb = std::min(nb, groups);
    int iters = (groups + nb - 1) / nb;
    // a block's cost run (iters * nw * R samples) is staged in LDS for one write-through store
    // (k_rollout): at most kMaxCostRun floats, more blocks otherwise
    iters = std::min(iters, std::max(1, kMaxCostRun / cost_run_stride(nw * R)));
    nb = (groups + iters - 1) / iters;
    if (c.model == MPPI_MODEL_QUADROTOR) {   // k_rollout_quad: 16 rollouts (4 lanes each) per dynamics
        l.threads = 256;                      // wave; 1 dynamics wave per block up to 1024 blocks, else 4
        iters = ((l.K + 15) / 16 * l.V <= 1024) ? 1 : 4;   // (carried in DevParams::iters)
        nb = (l.K + 16 * iters - 1) / (16 * iters);
    }
    if (c.model == MPPI_MODEL_AERIAL) {      // k_rollout_aerial: the quadrotor's blocks; four dynamics waves only
        l.threads = 256;                      // where the block's tiles fit (mppi_dev.h aerial_lds_floats)
        iters = ((l.K + 15) / 16 * l.V <= 1024 || aerial_lds_floats(H, 4) * (int64_t)sizeof(float) > kAerialLdsMax) ? 1 : 4;
        nb = (l.K + 16 * iters - 1) / (16 * iters);
    }
    if (nb > 4096) return fail(MPPI_ERR_INVALID_ARG, "too many rollout blocks (%d)", nb);
    // the rollout kernels address one vehicle's trajectory planes through a buffer
    // resource (32-bit byte offsets) and the record bodies with 32-bit indices
    if (c.store_trajectory && (uint64_t)l.C * ((l.K + 15) & ~15) * ((H + 15) & ~15) * sizeof(float) > 0xFFFFFFFFull)
        return fail(MPPI_ERR_INVALID_ARG, "trajectory of one vehicle (C=%d x K=%d x H=%d floats) exceeds 4 GiB: "
                    "disable store_trajectory or shard the samples", l.C, l.K, H);
    if ((uint64_t)l.V * l.A * nb * H >= 0x80000000ull)
        return fail(MPPI_ERR_INVALID_ARG, "record bodies (V=%d x A=%d x %d blocks x H=%d = %llu floats) exceed 2^31",
                    l.V, l.A, nb, H, (unsigned long long)l.V * l.A * nb * H);
    l.dp.L = L; l.dp.R = R; l.dp.nch = nch; l.dp.nb = nb; l.dp.iters = iters;
    return MPPI_OK;
}

// Sigma^-1 (covar_cost.py:21) and gamma^t (action_cost.py:21)
static mppi_status cost_tables(EngineLayout& l) {
    const mppi_config& c = l.cfg;
    const int A = l.A, W2 = 2 * A;
    std::vector<double> m(A * W2, 0.0);
    for (int i = 0; i < A; ++i) {
        for (int j = 0; j < A; ++j) m[i * W2 + j] = c.sigma[i * A + j];
        m[i * W2 + A + i] = 1.0;
    }
    for (int col = 0; col < A; ++col) {   // Gauss-Jordan, partial pivoting, fp64
        int piv = col;
        for (int r = col + 1; r < A; ++r)
            if (std::fabs(m[r * W2 + col]) > std::fabs(m[piv * W2 + col])) piv = r;
        if (std::fabs(m[piv * W2 + col]) < 1e-30) return fail(MPPI_ERR_INVALID_ARG, "Sigma is singular");
        for (int j = 0; j < W2; ++j) std::swap(m[col * W2 + j], m[piv * W2 + j]);
        const double d = m[col * W2 + col];
        for (int j = 0; j < W2; ++j) m[col * W2 + j] /= d;
        for (int r = 0; r < A; ++r)
            if (r != col) {
                const double f2 = m[r * W2 + col];
                for (int j = 0; j < W2; ++j) m[r * W2 + j] -= f2 * m[col * W2 + j];
            }
    }
    l.sinv.resize(A * A);
    l.gamma_t.resize(l.H);
    for (int i = 0; i < A; ++i)
        for (int j = 0; j < A; ++j) l.sinv[i * A + j] = (float)m[i * W2 + A + j];
    for (int t = 0; t < l.H; ++t) l.gamma_t[t] = std::pow(c.cost_gamma, (float)t);
    return MPPI_OK;
}

// the baked joint table, the leading fixed joints folded into fixedM (dp.j0), and the FK path
// the unfolded chain allows (dp.chain_fast)
static void chain(EngineLayout& l) {
    const mppi_config& c = l.cfg;
    JointDev* jd = l.joints;
    std::memset(jd, 0, sizeof(l.joints));
    for (int j = 0; j < c.n_joints; ++j) bake_joint(c.joints[j], jd[j]);
    // fold the leading fixed joints of the chain into the per-vehicle base transform
    const float I12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::memcpy(l.fixedM, I12, sizeof(I12));
    int j0 = 0;
    while (c.model != MPPI_MODEL_DRONE && j0 < c.n_joints && jd[j0].type == MPPI_JOINT_FIXED) {
        mul34(l.fixedM, jd[j0].O, l.fixedM);
        ++j0;
    }
    l.dp.j0 = j0;
    // fast FK path: the unfolded chain is exactly nq revolute-z joints in q order
    bool fast = c.model != MPPI_MODEL_DRONE && (c.n_joints - j0) == l.nq;
    for (int j = j0; fast && j < c.n_joints; ++j)
        fast = jd[j].type == MPPI_JOINT_REVOLUTE && jd[j].axis_z && jd[j].q_index == j - j0;
    l.dp.chain_fast = fast;
    if (fast && l.nq == 7 && c.n_joints - j0 == 7) {   // Kinova origin table (mppi_dev.h kKinova)
        bool kin = true;
        for (int j = 0; kin && j < 7; ++j) {
            const float* O = jd[j0 + j].O;
            const KinOrigin& k = kKinova[j];
            for (int col = 0; kin && col < 3; ++col)
                for (int row = 0; kin && row < 3; ++row) {
                    const float want = (row == k.p[col]) ? (float)k.s[col] : 0.0f;
                    kin = std::fabs(O[4 * row + col] - want) <= 1e-6f;
                }
            for (int d = 0; kin && d < 3; ++d) kin = ((k.tmask >> d) & 1) ? true : (O[4 * d + 3] == 0.0f);
        }
        if (kin && !getenv("MPPI_NO_KINOVA_PATH")) l.dp.chain_fast = 2;
    }
}

mppi_status layout_of(const mppi_config& cfg, EngineLayout& l) {
    l.cfg = cfg;
    if (l.cfg.model == MPPI_MODEL_WHOLEBODY || l.cfg.model == MPPI_MODEL_AERIAL) l.cfg.state_f64 = 0;
    const mppi_config& c = l.cfg;
    l.K = c.n_samples; l.H = c.n_horizon; l.A = c.n_action; l.V = c.n_vehicles;
    l.nq = nq_of(c);
    l.qoff = (c.model == MPPI_MODEL_WHOLEBODY) ? 3 : (c.model == MPPI_MODEL_AERIAL) ? 4 : 0;
    l.state_dim = mppi_state_dim(&c);
    l.out_dim = mppi_output_dim(&c);
    l.C = (c.model == MPPI_MODEL_DRONE) ? 3 : (c.model == MPPI_MODEL_QUADROTOR) ? 6
          : (c.model == MPPI_MODEL_AERIAL) ? 6 + l.nq + 12 : l.A + 12;
    l.out_bytes = (int64_t)(off_xerr(&l) + 16);
    const int H = l.H, P = (kHdr + l.A * H + 3) & ~3;

    DevParams& p = l.dp;
    std::memset(&p, 0, sizeof(p));
    mppi_status st = geometry(l);
    if (st != MPPI_OK) return st;
    if (savgol_taps(c.savgol_window, c.savgol_order, l.sg_taps) != 0)
        return fail(MPPI_ERR_INVALID_ARG, "bad SavGol window/order");
    l.sinv.clear();
    l.gamma_t.clear();
    // (the extra CostManager terms' tables; the tracking bit alone needs none)
    if ((c.cost_terms & ~MPPI_COST_TARGET_TRACK) && (st = cost_tables(l)) != MPPI_OK) return st;
    chain(l);
    if (c.model == MPPI_MODEL_AERIAL && l.dp.chain_fast != 2)
        return fail(MPPI_ERR_INVALID_ARG, "AERIAL kernels are built for the Kinova chain (leading fixed joints, then the "
                    "seven revolute-z joints of the ARM kernels' origin table)");

    p.model = c.model; p.V = l.V; p.K = l.K; p.H = H; p.A = l.A;
    p.nq = l.nq; p.qoff = l.qoff; p.nj = c.n_joints;
    // (the vehicle offset in the high half: the rollouts' fleet-wide Philox vehicle key)
    p.noise_mode = c.noise_mode | (c.vehicle_offset << 16); p.state_f64 = c.state_f64;
    p.store_traj = c.store_trajectory; p.store_noise = c.store_noise;
    bool diag = true;
    for (int a = 0; a < l.A; ++a)
        for (int b = 0; b < l.A; ++b) {
            if (a == b) p.sdiag[a] = c.sigma[a * l.A + b];
            else if (c.sigma[a * l.A + b] != 0.0f) diag = false;
        }
    p.sigma_diag = diag;
    p.P = P; p.C = l.C; p.hp = traj_pitch(&l);
    p.seed_lo = (uint32_t)c.seed; p.seed_hi = (uint32_t)(c.seed >> 32);
    p.k_offset = (int64_t)c.shard_rank * l.K;
    p.dt = (float)c.dt; p.dt2 = (float)(c.dt * c.dt); p.dt_d = c.dt;
    p.coef = (float)(-1.0 / c.lambda_);
    p.w_sp = c.w_stage_pos; p.w_so = c.w_stage_ori; p.w_tp = c.w_term_pos; p.w_to = c.w_term_ori;
    p.cost_terms = c.cost_terms;
    p.w_cov = (float)((double)c.w_covar * (c.lambda_ * (1.0 - (double)c.cost_alpha)));   // covar_cost.py:15,24
    p.w_cen = c.w_center; p.w_jt = c.w_joint_track; p.w_act = c.w_action; p.lim_pen = c.joint_limit_penalty;
    p.q_inv_m = (float)(1.0 / (double)c.quad_mass);   // 1/self.m as a Python float, used in fp32
    for (int d = 0; d < 3; ++d) p.q_iinv[d] = (float)(1.0 / (double)c.quad_inertia[d]);
    p.q_kd = c.quad_kd; p.q_g = c.quad_gravity; p.q_literal_jinv = c.quad_literal_jinv ? 1 : 0;

    FinParams& f = l.fp;
    std::memset(&f, 0, sizeof(f));
    f.model = c.model; f.V = l.V; f.H = H; f.A = l.A; f.nq = l.nq; f.qoff = l.qoff;
    f.state_f64 = c.state_f64; f.P = P;
    // (diagnostics: MPPI_FIN_TSZ = t per finalize slice, for the slice-count / fetch trade-off
    // measured in profiles/r05/finalize_fetch; 8 is the measured best)
    l.fin_tsz = 8;
    if (const char* z = getenv("MPPI_FIN_TSZ")) {
        const int tz = atoi(z);
        if (tz >= 1 && tz + 2 * (c.savgol_window / 2) <= 64) l.fin_tsz = tz;
    }
    f.tsz = l.fin_tsz; f.ts = l.fin_ts = (H + l.fin_tsz - 1) / l.fin_tsz;
    f.window = c.savgol_window; f.half = c.savgol_window / 2;
    for (int j = 0; j < c.savgol_window; ++j) f.sg[j] = l.sg_taps[c.savgol_window - 1 - j];
    f.coef = p.coef; f.dt = p.dt; f.dt2 = p.dt2; f.dt_d = c.dt;
    f.out_dim = l.out_dim;
    int generic = 0;
    if (const char* g = getenv("MPPI_GENERIC_KERNELS"))   // 1: all of them; one part by name (A/B of the parts)
        generic = !strcmp(g, "finalize") ? 1 : !strcmp(g, "quiet") ? 2 : !strcmp(g, "rollout") ? 4
                  : !strcmp(g, "quiet_rollout") ? 8 : atoi(g) != 0 ? kGenericAll : 0;
    set_generic(l, generic);
    return MPPI_OK;
}

// ------------------------------------------------------------------ the sphere scene
mppi_status scene_validate(const mppi_config& c, const mppi_scene& s) {
    if (c.model == MPPI_MODEL_QUADROTOR)
        return fail(MPPI_ERR_INVALID_ARG, "a scene needs the ARM, WHOLEBODY or DRONE model (no QUADROTOR scene kernel)");
    if (c.model == MPPI_MODEL_AERIAL)
        return fail(MPPI_ERR_INVALID_ARG, "a scene needs the ARM, WHOLEBODY or DRONE model (no AERIAL scene, field or "
                    "self-collision kernel)");
    if (s.n_body < 0 || s.n_body > MPPI_MAX_BODY_SPHERES)
        return fail(MPPI_ERR_INVALID_ARG, "scene: n_body %d outside 0..%d", s.n_body, MPPI_MAX_BODY_SPHERES);
    const float w[3] = {s.w_obs, s.margin, s.penalty};
    for (const float x : w)
        if (!std::isfinite(x) || x < 0.0f) return fail(MPPI_ERR_INVALID_ARG, "scene: w_obs, margin and penalty are finite and >= 0");
    const int nj = c.model == MPPI_MODEL_DRONE ? 0 : c.n_joints;
    for (int b = 0; b < s.n_body; ++b) {
        const mppi_body_sphere& sp = s.body[b];
        if (sp.frame < -1 || sp.frame >= nj)
            return fail(MPPI_ERR_INVALID_ARG, "scene: body sphere %d on frame %d, outside [-1, %d)", b, sp.frame, nj);
        if (!std::isfinite(sp.offset[0]) || !std::isfinite(sp.offset[1]) || !std::isfinite(sp.offset[2]) ||
            !std::isfinite(sp.radius))
            return fail(MPPI_ERR_INVALID_ARG, "scene: body sphere %d has a non-finite value", b);
        if (!(sp.radius > 0.0f)) return fail(MPPI_ERR_INVALID_ARG, "scene: body sphere %d radius %g <= 0", b, sp.radius);
    }
    return MPPI_OK;
}

void scene_body_table(const EngineLayout& l, const mppi_scene& s, float* table, int* order) {
    std::memset(table, 0, sizeof(float) * kSceneBodyW);
    const auto put = [&](int i, int32_t x) { std::memcpy(table + i, &x, sizeof(x)); };
    const int j0 = l.cfg.model == MPPI_MODEL_DRONE ? 0 : l.dp.j0;
    int slot[MPPI_MAX_BODY_SPHERES];
    double off[MPPI_MAX_BODY_SPHERES][3];
    for (int b = 0; b < s.n_body; ++b) {
        const mppi_body_sphere& sp = s.body[b];
        for (int d = 0; d < 3; ++d) off[b][d] = sp.offset[d];
        if (sp.frame >= j0) { slot[b] = sp.frame - j0 + 1; continue; }
        // a frame the base swallowed: o' = (O_{f+1} .. O_{j0-1})^-1 (o, 1), the rigid inverses applied
        // from the left-most factor on, in double
        slot[b] = 0;
        for (int j = sp.frame + 1; j < j0; ++j) {
            const float* O = l.joints[j].O;
            const double d[3] = {off[b][0] - O[3], off[b][1] - O[7], off[b][2] - O[11]};
            for (int i = 0; i < 3; ++i) off[b][i] = (double)O[i] * d[0] + (double)O[4 + i] * d[1] + (double)O[8 + i] * d[2];
        }
    }
    int n = 0;
    for (int sl = 0; sl <= kSceneSlots; ++sl) {   // stable by slot; the last word: n_body
        put(kSceneRng + sl, n);
        for (int b = 0; b < s.n_body && sl < kSceneSlots; ++b)
            if (slot[b] == sl) {
                float* w = table + kSceneSph + 4 * n;
                for (int d = 0; d < 3; ++d) w[d] = (float)off[b][d];
                w[3] = s.body[b].radius;
                if (order) order[n] = b;
                ++n;
            }
    }
    put(0, s.n_body);
    table[1] = s.w_obs; table[2] = s.margin; table[3] = s.penalty;
    put(4, (int32_t)scene_clr_off(l.V));
    put(5, (int32_t)scene_plan_off(l.V, l.K));
    put(6, l.K);
}

mppi_status obstacles_validate(int n_vehicles, int vehicle, int n, const float* center, const float* radius, const float* vel) {
    if (vehicle < 0 || vehicle >= n_vehicles) return fail(MPPI_ERR_INVALID_ARG, "mppi_set_obstacles: vehicle %d of %d", vehicle, n_vehicles);
    if (n < 0 || n > MPPI_MAX_OBSTACLES) return fail(MPPI_ERR_INVALID_ARG, "mppi_set_obstacles: n %d outside 0..%d", n, MPPI_MAX_OBSTACLES);
    if (n > 0 && (!center || !radius)) return fail(MPPI_ERR_INVALID_ARG, "mppi_set_obstacles: null centres or radii");
    for (int o = 0; o < n; ++o) {
        bool fin = std::isfinite(radius[o]);
        for (int d = 0; d < 3; ++d) fin = fin && std::isfinite(center[3 * o + d]) && (!vel || std::isfinite(vel[3 * o + d]));
        if (!fin) return fail(MPPI_ERR_INVALID_ARG, "mppi_set_obstacles: obstacle %d has a non-finite value", o);
        if (!(radius[o] > 0.0f)) return fail(MPPI_ERR_INVALID_ARG, "mppi_set_obstacles: obstacle %d radius %g <= 0", o, radius[o]);
    }
    return MPPI_OK;
}

void obstacles_fill(float* block, int n, const float* center, const float* radius, const float* vel) {
    std::memset(block, 0, sizeof(float) * kSceneObsW);
    const int32_t n32 = n;
    std::memcpy(block, &n32, sizeof(n32));
    for (int o = 0; o < n; ++o) {
        float* r = block + 4 + 8 * o;
        for (int d = 0; d < 3; ++d) {
            r[d] = center[3 * o + d];
            r[4 + d] = vel ? vel[3 * o + d] : 0.0f;
        }
        r[3] = radius[o];
    }
}

// ------------------------------------------------------------------ the distance field
mppi_status field_validate(const mppi_field_desc* f) {
    if (!f) return fail(MPPI_ERR_INVALID_ARG, "field: null descriptor");
    int64_t nvox = 1;
    for (int d = 0; d < 3; ++d) {
        if (f->dims[d] < 2 || f->dims[d] > kFieldMaxDim)
            return fail(MPPI_ERR_INVALID_ARG, "field: dims[%d] = %d outside 2..%d", d, f->dims[d], kFieldMaxDim);
        nvox *= f->dims[d];
    }
    if (nvox > MPPI_FIELD_MAX_VOXELS)
        return fail(MPPI_ERR_INVALID_ARG, "field: %lld voxels, more than MPPI_FIELD_MAX_VOXELS", (long long)nvox);
    if (!std::isfinite(f->voxel) || !(f->voxel > 0.0f) || !std::isfinite(1.0f / f->voxel))
        return fail(MPPI_ERR_INVALID_ARG, "field: voxel %g is not finite and > 0", f->voxel);
    for (int d = 0; d < 3; ++d)
        if (!std::isfinite(f->origin[d])) return fail(MPPI_ERR_INVALID_ARG, "field: non-finite origin");
    if (f->reserved != 0) return fail(MPPI_ERR_INVALID_ARG, "field: reserved word %d is not 0", f->reserved);
    return MPPI_OK;
}

mppi_status field_engine_validate(const mppi_config& c, const mppi_scene* scene, const mppi_field_desc* f, mppi_scene& use) {
    if (!f) return fail(MPPI_ERR_INVALID_ARG, "field: null descriptor");
    if (scene) use = *scene;
    else mppi_scene_default(&use, &c);
    mppi_status st = scene_validate(c, use);
    if (st != MPPI_OK) return st;
    return field_validate(f);
}

mppi_status field_data_validate(const mppi_field_desc& f, const float* origin3, const float* d_zyx) {
    for (int d = 0; origin3 && d < 3; ++d)
        if (!std::isfinite(origin3[d])) return fail(MPPI_ERR_INVALID_ARG, "mppi_set_distance_field: non-finite origin");
    const int64_t nvox = field_voxels(f);
    for (int64_t i = 0; d_zyx && i < nvox; ++i)
        if (!std::isfinite(d_zyx[i]))
            return fail(MPPI_ERR_INVALID_ARG, "mppi_set_distance_field: non-finite value at voxel %lld", (long long)i);
    return MPPI_OK;
}

void field_header(const mppi_field_desc& f, const float* origin3, bool set, float* hdr) {
    std::memset(hdr, 0, sizeof(float) * kFieldHdrW);
    const auto put = [&](int i, int32_t x) { std::memcpy(hdr + i, &x, sizeof(x)); };
    for (int d = 0; d < 3; ++d) {
        hdr[d] = origin3[d];
        put(4 + d, f.dims[d]);
    }
    hdr[3] = 1.0f / f.voxel;
    put(7, set ? 1 : 0);
    put(8, f.dims[0]);
    put(9, f.dims[0] * f.dims[1]);
    put(10, (int32_t)field_voxels(f));
    hdr[11] = f.voxel;
}

void field_pack(const mppi_field_desc& f, const float* d_zyx, float* cells) {
    const int nx = f.dims[0];
    const int64_t rows = (int64_t)f.dims[1] * f.dims[2];
    for (int64_t r = 0; r < rows; ++r) {
        const float* src = d_zyx + r * nx;
        float* dst = cells + 2 * r * nx;
        for (int x = 0; x < nx; ++x) {
            dst[2 * x] = src[x];
            dst[2 * x + 1] = src[x + 1 < nx ? x + 1 : nx - 1];
        }
    }
}

// ------------------------------------------------------------------ self-collision pairs
int self_sep(const mppi_config& c, int fa, int fb) {
    const int lo = std::min(fa, fb), hi = std::max(fa, fb);
    int n = 0;
    for (int j = lo + 1; j <= hi && j < c.n_joints; ++j)
        if (j >= 0 && c.joints[j].type != MPPI_JOINT_FIXED) ++n;
    return n;
}

mppi_status self_validate(const mppi_config& c, const mppi_scene& s, const mppi_self_collision* sc) {
    if (!sc) return fail(MPPI_ERR_INVALID_ARG, "self: null pair list");
    if (c.model != MPPI_MODEL_ARM && c.model != MPPI_MODEL_WHOLEBODY)
        return fail(MPPI_ERR_INVALID_ARG, "self: self-collision pairs need the ARM or WHOLEBODY model (no chain: every pair is rigid)");
    if (sc->n_pairs < 0 || sc->n_pairs > MPPI_MAX_SELF_PAIRS)
        return fail(MPPI_ERR_INVALID_ARG, "self: n_pairs %d outside 0..%d", sc->n_pairs, MPPI_MAX_SELF_PAIRS);
    const float w[3] = {sc->w_self, sc->margin, sc->penalty};
    for (const float x : w)
        if (!std::isfinite(x) || x < 0.0f) return fail(MPPI_ERR_INVALID_ARG, "self: w_self, margin and penalty are finite and >= 0");
    for (int i = 0; i < sc->n_pairs; ++i) {
        const int a = sc->pair[i][0], b = sc->pair[i][1];
        if (a < 0 || a >= s.n_body || b < 0 || b >= s.n_body)
            return fail(MPPI_ERR_INVALID_ARG, "self: pair %d (%d, %d) has an index outside [0, %d)", i, a, b, s.n_body);
        if (a == b) return fail(MPPI_ERR_INVALID_ARG, "self: pair %d (%d, %d) pairs a sphere with itself", i, a, b);
        for (int k = 0; k < i; ++k)
            if ((sc->pair[k][0] == a && sc->pair[k][1] == b) || (sc->pair[k][0] == b && sc->pair[k][1] == a))
                return fail(MPPI_ERR_INVALID_ARG, "self: pair %d (%d, %d) repeats pair %d", i, a, b, k);
        if (self_sep(c, s.body[a].frame, s.body[b].frame) == 0)
            return fail(MPPI_ERR_INVALID_ARG, "self: pair %d (%d, %d) is rigid: no moving joint between frames %d and %d", i, a, b,
                        s.body[a].frame, s.body[b].frame);
    }
    return MPPI_OK;
}

mppi_status self_engine_validate(const mppi_config& c, const mppi_scene* scene, const mppi_field_desc* f,
                                 const mppi_self_collision* sc, mppi_scene& use) {
    if (scene) use = *scene;
    else mppi_scene_default(&use, &c);
    mppi_status st = scene_validate(c, use);
    if (st != MPPI_OK) return st;
    if (f && (st = field_validate(f)) != MPPI_OK) return st;
    return self_validate(c, use, sc);
}

int self_member_count(const mppi_self_collision& sc) {
    bool used[MPPI_MAX_BODY_SPHERES] = {false};
    for (int i = 0; i < sc.n_pairs; ++i)
        for (int e = 0; e < 2; ++e) used[sc.pair[i][e]] = true;
    return (int)std::count(used, used + MPPI_MAX_BODY_SPHERES, true);
}

int self_table(const EngineLayout& l, const mppi_scene& s, const mppi_self_collision& sc, const int* order, float* region) {
    std::memset(region, 0, sizeof(float) * kSelfHdrW);
    const auto put = [&](int i, int32_t x) { std::memcpy(region + i, &x, sizeof(x)); };
    int pos[MPPI_MAX_BODY_SPHERES] = {0};      // the caller's index -> the sorted position
    for (int n = 0; n < s.n_body; ++n) pos[order[n]] = n;
    bool used[MPPI_MAX_BODY_SPHERES] = {false};   // by sorted position
    for (int i = 0; i < sc.n_pairs; ++i)
        for (int e = 0; e < 2; ++e) used[pos[sc.pair[i][e]]] = true;
    int member[MPPI_MAX_BODY_SPHERES], members = 0;
    for (int n = 0; n < MPPI_MAX_BODY_SPHERES; ++n) {
        member[n] = (n < s.n_body && used[n]) ? members++ : -1;
        put(kSelfMem + n, member[n]);
    }
    for (int i = 0; i < sc.n_pairs; ++i) {
        const int a = sc.pair[i][0], b = sc.pair[i][1];
        put(kSelfPair + 3 * i, member[pos[a]]);
        put(kSelfPair + 3 * i + 1, member[pos[b]]);
        region[kSelfPair + 3 * i + 2] = s.body[a].radius + s.body[b].radius;
    }
    put(0, sc.n_pairs);
    region[1] = sc.w_self; region[2] = sc.margin; region[3] = sc.penalty;
    put(4, members);
    put(5, (int32_t)self_clr_off(l.V, l.K, l.H));
    put(6, (int32_t)self_plan_off(l.V, l.K, l.H));
    return members;
}

mppi_status self_layout(const mppi_config& c, int members, EngineLayout& l) {
    const auto bytes = [&]() { return self_dyn_lds(l.A, l.H, l.threads, l.dp.iters, members) + kSelfStaticLds; };
    mppi_status st;
    if (c.block_threads) {
        if ((st = layout_of(c, l)) != MPPI_OK) return st;
        if (l.threads < 64 || l.threads > 256 || l.threads % 64)
            return fail(MPPI_ERR_INVALID_ARG, "self: block_threads %d: the self kernels run blocks of 64, 128, 192 or 256 threads", l.threads);
        if (l.threads > 64 && bytes() > kSelfLdsTarget)
            return fail(MPPI_ERR_INVALID_ARG, "self: block_threads %d needs %lld B of LDS with %d paired spheres at H = %d, more than the %d B "
                        "a self block may hold: use a smaller block, or 0 for the largest that fits", l.threads, (long long)bytes(), members,
                        l.H, kSelfLdsTarget);
    } else {
        for (const int t : {256, 128, 64}) {
            l.auto_threads = t;
            if ((st = layout_of(c, l)) != MPPI_OK) return st;
            if (bytes() <= kSelfLdsTarget) break;
        }
    }
    if (bytes() > kSelfLdsMax)
        return fail(MPPI_ERR_INVALID_ARG, "self: a block of %d threads needs %lld B of LDS at H = %d, more than the CU holds", l.threads,
                    (long long)bytes(), l.H);
    return MPPI_OK;
}

// ------------------------------------------------------------------ occupancy grids
mppi_status occupancy_validate(const float* origin3, const uint8_t* occ_zyx, float max_dist) {
    if (!occ_zyx) return fail(MPPI_ERR_INVALID_ARG, "occupancy: null grid");
    for (int d = 0; origin3 && d < 3; ++d)
        if (!std::isfinite(origin3[d])) return fail(MPPI_ERR_INVALID_ARG, "occupancy: non-finite origin");
    if (std::isnan(max_dist) || (std::isinf(max_dist) && max_dist > 0.0f))
        return fail(MPPI_ERR_INVALID_ARG, "occupancy: max_dist %g (a finite cap, or <= 0 for none)", max_dist);
    return MPPI_OK;
}

// out[i] = min_j (in[j] + (i - j)^2) over one line of n nodes `stride` apart, for both grids at once: j
// walks outward from i and stops where (i - j)^2 reaches both running minima, as k_edt_axis does.
static void occupancy_line(int32_t* a, int32_t* b, int n, int64_t stride, int32_t* la, int32_t* lb) {
    for (int i = 0; i < n; ++i) { la[i] = a[i * stride]; lb[i] = b[i * stride]; }
    for (int i = 0; i < n; ++i) {
        int32_t ma = la[i], mb = lb[i];
        for (int d = 1; d < n; ++d) {
            const int32_t dd = d * d;
            if (dd >= ma && dd >= mb) break;
            if (i - d >= 0) { ma = std::min(ma, la[i - d] + dd); mb = std::min(mb, lb[i - d] + dd); }
            if (i + d < n) { ma = std::min(ma, la[i + d] + dd); mb = std::min(mb, lb[i + d] + dd); }
        }
        a[i * stride] = ma;
        b[i * stride] = mb;
    }
}

void occupancy_field(const mppi_field_desc& f, const uint8_t* occ, float max_dist, float* d_zyx) {
    const int nx = f.dims[0], ny = f.dims[1], nz = f.dims[2];
    const int64_t sy = nx, sz = (int64_t)nx * ny, nvox = field_voxels(f);
    const float cap = edt_cap(f.dims, f.voxel, max_dist);
    std::vector<int32_t> ga((size_t)nvox), gb((size_t)nvox), la(kEdtMaxLine), lb(kEdtMaxLine);
    // x: the distance to the nearest seed of each set on either side, one sweep each way
    for (int64_t r = 0; r < (int64_t)ny * nz; ++r) {
        const uint8_t* o = occ + r * nx;
        int32_t* a = ga.data() + r * nx;
        int32_t* b = gb.data() + r * nx;
        int lo = -1, lf = -1;
        for (int x = 0; x < nx; ++x) {
            if (o[x]) lo = x; else lf = x;
            a[x] = lo < 0 ? kEdtInf : (x - lo) * (x - lo);
            b[x] = lf < 0 ? kEdtInf : (x - lf) * (x - lf);
        }
        lo = lf = -1;
        for (int x = nx - 1; x >= 0; --x) {
            if (o[x]) lo = x; else lf = x;
            if (lo >= 0) a[x] = std::min(a[x], (lo - x) * (lo - x));
            if (lf >= 0) b[x] = std::min(b[x], (lf - x) * (lf - x));
        }
    }
    for (int z = 0; z < nz; ++z)
        for (int x = 0; x < nx; ++x)
            occupancy_line(ga.data() + z * sz + x, gb.data() + z * sz + x, ny, sy, la.data(), lb.data());
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x)
            occupancy_line(ga.data() + y * sy + x, gb.data() + y * sy + x, nz, sz, la.data(), lb.data());
    for (int64_t e = 0; e < nvox; ++e) d_zyx[e] = edt_value(ga[(size_t)e], gb[(size_t)e], f.voxel, cap);
}

// ------------------------------------------------------------------ depth images
static_assert(sizeof(mppi_depth_view) == 80, "mppi_depth_view is 80 bytes (include/mppi_hip.h)");
mppi_status depth_validate(const mppi_field_desc& f, const mppi_depth_view* v, const float* depth_hw) {
    if (!v) return fail(MPPI_ERR_INVALID_ARG, "depth: null view");
    if (!depth_hw) return fail(MPPI_ERR_INVALID_ARG, "depth: null image");
    if (v->width < 1 || v->height < 1 || (int64_t)v->width * v->height > (int64_t)MPPI_DEPTH_MAX_PIXELS)
        return fail(MPPI_ERR_INVALID_ARG, "depth: image %d x %d (each >= 1, at most MPPI_DEPTH_MAX_PIXELS pixels)", v->width, v->height);
    if (v->stride < 1) return fail(MPPI_ERR_INVALID_ARG, "depth: stride %d (>= 1)", v->stride);
    if (v->carve != 0 && v->carve != 1) return fail(MPPI_ERR_INVALID_ARG, "depth: carve %d (0 or 1)", v->carve);
    const float vals[] = {v->fx, v->fy, v->cx, v->cy, v->z_min, v->z_max, v->pos[0], v->pos[1], v->pos[2],
                          v->quat_xyzw[0], v->quat_xyzw[1], v->quat_xyzw[2], v->quat_xyzw[3]};
    for (const float x : vals)
        if (!std::isfinite(x)) return fail(MPPI_ERR_INVALID_ARG, "depth: non-finite view value");
    if (!(v->fx > 0.0f) || !(v->fy > 0.0f) || !std::isfinite(1.0f / v->fx) || !std::isfinite(1.0f / v->fy))
        return fail(MPPI_ERR_INVALID_ARG, "depth: focal lengths %g, %g (> 0)", v->fx, v->fy);
    if (!(v->z_min >= 0.0f) || !(v->z_min < v->z_max) || !(v->z_max / f.voxel <= 4096.0f))
        return fail(MPPI_ERR_INVALID_ARG, "depth: z range %g..%g (0 <= z_min < z_max, z_max / voxel <= 4096)", v->z_min, v->z_max);
    const float* q = v->quat_xyzw;
    const float n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (!(n2 >= 0.5f && n2 <= 2.0f)) return fail(MPPI_ERR_INVALID_ARG, "depth: quaternion of squared norm %g (0.5..2)", n2);
    for (const int32_t w : v->reserved)
        if (w != 0) return fail(MPPI_ERR_INVALID_ARG, "depth: reserved word %d is not 0", w);
    return MPPI_OK;
}

void depth_params(const mppi_field_desc& f, const mppi_depth_view& v, DepthParams& p) {
    std::memset(&p, 0, sizeof(p));
    p.nx = f.dims[0]; p.ny = f.dims[1]; p.nz = f.dims[2];
    p.width = v.width; p.height = v.height; p.stride = v.stride;
    p.cols = depth_used(v.width, v.stride); p.rows = depth_used(v.height, v.stride);
    p.carve = v.carve;
    p.inv_fx = 1.0f / v.fx; p.inv_fy = 1.0f / v.fy;
    p.cx = v.cx; p.cy = v.cy; p.z_min = v.z_min; p.z_max = v.z_max;
    p.inv_voxel = 1.0f / f.voxel;
    quat_xyzw_to_R(v.quat_xyzw, p.R);
    for (int d = 0; d < 3; ++d) { p.pos[d] = v.pos[d]; p.origin[d] = f.origin[d]; }
}

void depth_integrate(const DepthParams& p) {
    const int64_t nvox = (int64_t)p.nx * p.ny * p.nz;
    for (int64_t e = 0; e < nvox; ++e) p.occ[e] = p.occ[e] != 0;
    for (int pass = p.carve ? 0 : 1; pass < 2; ++pass)   // carve, then mark: occupied wins
        for (int j = 0; j < p.height; j += p.stride)
            for (int i = 0; i < p.width; i += p.stride) {
                DepthRay r;
                if (!depth_ray(p, i, j, p.depth[(size_t)j * (size_t)p.width + (size_t)i], r)) continue;
                if (pass == 1) {
                    if (r.end >= 0) p.occ[r.end] = 1;
                    continue;
                }
                for (int m = r.m_lo; m <= r.m_hi; ++m) {
                    const int64_t node = depth_sample(p, r, m);
                    if (node >= 0) p.occ[node] = 0;
                }
            }
}

mppi_status shift_validate(const mppi_field_desc& f, const int32_t* s, float max_dist, ShiftParams& p, float* origin_out) {
    if (!s) return fail(MPPI_ERR_INVALID_ARG, "shift: null shift");
    if (std::isnan(max_dist) || (std::isinf(max_dist) && max_dist > 0.0f))
        return fail(MPPI_ERR_INVALID_ARG, "shift: max_dist %g (a finite cap, or <= 0 for none)", max_dist);
    std::memset(&p, 0, sizeof(p));
    p.nx = f.dims[0]; p.ny = f.dims[1]; p.nz = f.dims[2];
    int32_t c[3];
    for (int d = 0; d < 3; ++d) {
        origin_out[d] = fmaf((float)s[d], f.voxel, f.origin[d]);
        if (!std::isfinite(origin_out[d])) return fail(MPPI_ERR_INVALID_ARG, "shift: %d nodes along axis %d take the origin out of range", s[d], d);
        c[d] = std::min(std::max(s[d], -f.dims[d]), f.dims[d]);   // (beyond the grid either way: every node is free)
    }
    p.sx = c[0]; p.sy = c[1]; p.sz = c[2];
    return MPPI_OK;
}

void map_shift(const ShiftParams& p) {
    const int64_t nvox = (int64_t)p.nx * p.ny * p.nz;
    for (int64_t e = 0; e < nvox; ++e) p.occ[e] = shift_value(p, e);
}

// ------------------------------------------------------------------ rotor limits
static const char* const kLimitDims[kLimitsN] = {"thrust", "tau_x", "tau_y", "tau_z"};
static const char* const kModelNames[] = {"DRONE", "ARM", "WHOLEBODY", "QUADROTOR", "AERIAL"};

mppi_status limits_values_validate(const mppi_limits* lim) {
    if (!lim) return fail(MPPI_ERR_INVALID_ARG, "limits: null argument");
    for (int a = 0; a < kLimitsN; ++a) {
        if (std::isnan(lim->lo[a]) || std::isnan(lim->hi[a]))
            return fail(MPPI_ERR_INVALID_ARG, "limits: dim %d (%s) has a NaN bound", a, kLimitDims[a]);
        if (lim->lo[a] > lim->hi[a])
            return fail(MPPI_ERR_INVALID_ARG, "limits: dim %d (%s) has lo %g > hi %g", a, kLimitDims[a], lim->lo[a], lim->hi[a]);
    }
    return MPPI_OK;
}

mppi_status limits_validate(const mppi_config& c, const mppi_limits* lim) {
    if (c.model != MPPI_MODEL_QUADROTOR && c.model != MPPI_MODEL_AERIAL)
        return fail(MPPI_ERR_INVALID_ARG, "limits need the QUADROTOR or AERIAL model (the %s model's outputs are formed in "
                    "the finalize, which limits do not touch)", kModelNames[c.model]);
    if (c.shard_count > 1)
        return fail(MPPI_ERR_INVALID_ARG, "limits: bounded engines are not sharded (shard_count %d)", c.shard_count);
    return limits_values_validate(lim);
}

void set_generic(EngineLayout& l, int generic) {
    l.generic = generic;
    l.fp.kern = (generic & 1) ? kFinKernGeneric : 0;
    l.dp.kern = (generic & 4) ? kRollKernGeneric : 0;   // (the quiet bits: per launch, mppi_launches.cpp)
}

}  // namespace mppi_host

using namespace mppi_host;

// The project's default scene (include/mppi_hip.h; the Python twin: robot/body_spheres.py): placeholders
// for the user's collision model -- 0.05 m at the frame origin of every actuated chain joint, 0.30 m on
// the base frame of a flying vehicle; w_obs = 100, margin = 0.05 m, penalty = 1e4.
extern "C" void mppi_scene_default(mppi_scene* s, const mppi_config* cfg) {
    if (!s) return;
    std::memset(s, 0, sizeof(*s));
    s->w_obs = 100.0f; s->margin = 0.05f; s->penalty = 1e4f;
    if (!cfg || cfg->model == MPPI_MODEL_QUADROTOR || cfg->model == MPPI_MODEL_AERIAL) return;
    const auto add = [&](int frame, float r) {
        if (s->n_body < MPPI_MAX_BODY_SPHERES) s->body[s->n_body++] = mppi_body_sphere{frame, {0.0f, 0.0f, 0.0f}, r};
    };
    if (cfg->model != MPPI_MODEL_ARM) add(-1, 0.30f);
    if (cfg->model != MPPI_MODEL_DRONE)
        for (int j = 0; j < cfg->n_joints && j < MPPI_MAX_JOINTS; ++j)
            if (cfg->joints[j].type != MPPI_JOINT_FIXED) add(j, 0.05f);
}

// The default rotor limits (include/mppi_hip.h): thrust within [0, 2 m g] (the fp32 product of quad_mass and
// quad_gravity, doubled), the torques unbounded.
extern "C" void mppi_limits_default(mppi_limits* lim, const mppi_config* cfg) {
    if (!lim) return;
    for (int a = 0; a < kLimitsN; ++a) { lim->lo[a] = -INFINITY; lim->hi[a] = INFINITY; }
    if (!cfg) return;
    lim->lo[0] = 0.0f;
    lim->hi[0] = 2.0f * (cfg->quad_mass * cfg->quad_gravity);
}

// Host replay of the limits' arithmetic (include/mppi_hip.h): the kernels' own inline over u (H,4), eps (K,H,4).
extern "C" mppi_status mppi_limits_apply(const mppi_limits* lim, const float* u_h4, const float* eps_kh4, int32_t K, int32_t H,
                                         float* eps_eff_kh4, float* ctl_kh4) {
    const mppi_status st = limits_values_validate(lim);
    if (st != MPPI_OK) return st;
    if (!u_h4 || !eps_kh4 || K < 0 || H < 0) return fail(MPPI_ERR_INVALID_ARG, "mppi_limits_apply: bad arguments");
    for (int64_t k = 0; k < K; ++k)
        for (int64_t t = 0; t < H; ++t)
            for (int a = 0; a < kLimitsN; ++a) {
                const int64_t i = (k * H + t) * kLimitsN + a;
                float e, c;
                mppi::limits_apply(u_h4[t * kLimitsN + a], eps_kh4[i], lim->lo[a], lim->hi[a], e, c);
                if (eps_eff_kh4) eps_eff_kh4[i] = e;
                if (ctl_kh4) ctl_kh4[i] = c;
            }
    return MPPI_OK;
}

// The project's default pair list (include/mppi_hip.h; the Python twin's weights: robot/body_spheres.py):
// every pair of the scene's spheres with at least three moving joints between their frames, in (a, b)
// order; w_self = 100, margin = 0.02 m, penalty = 1e4.
extern "C" void mppi_self_collision_default(mppi_self_collision* out, const mppi_config* cfg, const mppi_scene* scene) {
    if (!out) return;
    std::memset(out, 0, sizeof(*out));
    out->w_self = 100.0f; out->margin = 0.02f; out->penalty = 1e4f;
    if (!cfg || (cfg->model != MPPI_MODEL_ARM && cfg->model != MPPI_MODEL_WHOLEBODY)) return;
    mppi_scene use;
    if (scene) use = *scene;
    else mppi_scene_default(&use, cfg);
    const int nb = std::min(std::max(use.n_body, 0), MPPI_MAX_BODY_SPHERES);
    for (int a = 0; a < nb; ++a)
        for (int b = a + 1; b < nb && out->n_pairs < MPPI_MAX_SELF_PAIRS; ++b)
            if (self_sep(*cfg, use.body[a].frame, use.body[b].frame) >= 3) {
                out->pair[out->n_pairs][0] = a;
                out->pair[out->n_pairs][1] = b;
                ++out->n_pairs;
            }
}

// Diagnostic (no GPU): the argument check of mppi_create_scene_self (scene null: the default one; no
// field) and the layout it makes.  table: the body table with the region's offset in word kSelfWord
// (kSceneBodyW words); region: the pair region's header and tables (kSelfHdrW words); out (8 ints): the
// block's threads, the members, the dynamic LDS bytes of a rollout block, the region's offset, the
// buffer's words, nb, iters, the static LDS bound.  Any of the three may be null.  Returns the first
// failing status (the message in mppi_last_error).  tests/test_capi_self_collision_cpu.py.
extern "C" int32_t mppi_debug_self_layout(const mppi_config* cfg, const mppi_scene* scene, const mppi_self_collision* self,
                                          float* table, float* region, int32_t* out) {
    if (!cfg) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_self_layout: bad arguments");
    mppi_status st = validate(*cfg);
    if (st != MPPI_OK) return st;
    mppi_scene use;
    if ((st = self_engine_validate(*cfg, scene, nullptr, self, use)) != MPPI_OK) return st;
    EngineLayout l;
    if ((st = self_layout(*cfg, self_member_count(*self), l)) != MPPI_OK) return st;
    float t[kSceneBodyW], r[kSelfHdrW];
    int ord[MPPI_MAX_BODY_SPHERES] = {0};
    scene_body_table(l, use, t, ord);
    const int32_t off = (int32_t)self_off(l.V, l.K, l.H);
    std::memcpy(t + kSelfWord, &off, sizeof(off));
    const int members = self_table(l, use, *self, ord, r);
    if (table) std::memcpy(table, t, sizeof(t));
    if (region) std::memcpy(region, r, sizeof(r));
    if (out) {
        const int32_t w[8] = {l.threads, members, (int32_t)self_dyn_lds(l.A, l.H, l.threads, l.dp.iters, members), off,
                              (int32_t)self_words(l.V, l.K, l.H), l.dp.nb, l.dp.iters, kSelfStaticLds};
        std::memcpy(out, w, sizeof(w));
    }
    return MPPI_OK;
}

// The occupancy grid's distance field on the host (include/mppi_hip.h): mppi_set_occupancy's definition
// without a device.
extern "C" mppi_status mppi_occupancy_field(const mppi_field_desc* desc, const uint8_t* occ_zyx, float max_dist, float* d_zyx) {
    mppi_status st = field_validate(desc);
    if (st != MPPI_OK) return st;
    if ((st = occupancy_validate(nullptr, occ_zyx, max_dist)) != MPPI_OK) return st;
    if (!d_zyx) return fail(MPPI_ERR_INVALID_ARG, "mppi_occupancy_field: null output");
    occupancy_field(*desc, occ_zyx, max_dist, d_zyx);
    return MPPI_OK;
}

// One depth image into an occupancy map on the host (include/mppi_hip.h): mppi_integrate_depth's map update
// without a device.
extern "C" mppi_status mppi_depth_integrate_host(const mppi_field_desc* desc, const mppi_depth_view* view, const float* depth_hw,
                                                 uint8_t* occ_zyx_inout) {
    mppi_status st = field_validate(desc);
    if (st != MPPI_OK) return st;
    if ((st = depth_validate(*desc, view, depth_hw)) != MPPI_OK) return st;
    if (!occ_zyx_inout) return fail(MPPI_ERR_INVALID_ARG, "mppi_depth_integrate_host: null map");
    DepthParams p;
    depth_params(*desc, *view, p);
    p.depth = depth_hw;
    p.occ = occ_zyx_inout;
    depth_integrate(p);
    return MPPI_OK;
}

// mppi_integrate_depth's argument check alone (no GPU, no image): what a caller that queues frames for later
// runs before it queues one (mppi_solver/_base.py).  Returns the first failing status.
extern "C" int32_t mppi_debug_depth_validate(const mppi_field_desc* desc, const mppi_depth_view* view, float max_dist) {
    mppi_status st = field_validate(desc);
    if (st != MPPI_OK) return st;
    static const float pixel = 0.0f;   // (the image is checked for null only)
    if ((st = depth_validate(*desc, view, &pixel)) != MPPI_OK) return st;
    if (std::isnan(max_dist) || (std::isinf(max_dist) && max_dist > 0.0f))
        return fail(MPPI_ERR_INVALID_ARG, "depth: max_dist %g (a finite cap, or <= 0 for none)", max_dist);
    return MPPI_OK;
}

// Diagnostic (no GPU): mppi_shift_map's map and origin on the host through k_map_shift's own inline: occ_zyx
// (nz,ny,nx) in, out_zyx out (distinct arrays), origin_out the moved origin.  tests/test_capi_depth_cpu.py.
extern "C" int32_t mppi_debug_map_shift(const mppi_field_desc* desc, const int32_t* shift_xyz, const uint8_t* occ_zyx,
                                        uint8_t* out_zyx, float* origin_out) {
    mppi_status st = field_validate(desc);
    if (st != MPPI_OK) return st;
    if (!occ_zyx || !out_zyx || !origin_out || occ_zyx == out_zyx) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_map_shift: bad arguments");
    ShiftParams p;
    if ((st = shift_validate(*desc, shift_xyz, 0.0f, p, origin_out)) != MPPI_OK) return st;
    p.src = occ_zyx;
    p.occ = out_zyx;
    map_shift(p);
    return MPPI_OK;
}

// Diagnostic (no GPU): validate, scene_validate and the body table of a configuration and a scene.
// table: kSceneBodyW words; order: n_body ints (either may be null).  Returns the first failing status.
// tests/test_capi_obstacles_cpu.py.
extern "C" int32_t mppi_debug_scene_layout(const mppi_config* cfg, const mppi_scene* scene, float* table, int32_t* order) {
    if (!cfg || !scene) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_scene_layout: bad arguments");
    mppi_status st = validate(*cfg);
    if (st != MPPI_OK) return st;
    if ((st = scene_validate(*cfg, *scene)) != MPPI_OK) return st;
    EngineLayout l;
    if ((st = layout_of(*cfg, l)) != MPPI_OK) return st;
    float t[kSceneBodyW];
    int ord[MPPI_MAX_BODY_SPHERES] = {0};
    scene_body_table(l, *scene, t, ord);
    if (table) std::memcpy(table, t, sizeof(t));
    if (order) std::memcpy(order, ord, sizeof(int32_t) * (size_t)scene->n_body);
    return MPPI_OK;
}

// Diagnostic (no GPU): the errors of mppi_set_obstacles for an engine of n_vehicles, and (block non-null)
// the vehicle block the call would stage (kSceneObsW words).
extern "C" int32_t mppi_debug_obstacles(int32_t n_vehicles, int32_t vehicle, int32_t n, const float* center,
                                        const float* radius, const float* vel, float* block) {
    const mppi_status st = obstacles_validate(n_vehicles, vehicle, n, center, radius, vel);
    if (st == MPPI_OK && block) obstacles_fill(block, n, center, radius, vel);
    return st;
}

// Diagnostic (no GPU): the errors of mppi_create_scene_field's descriptor and mppi_set_distance_field's
// arrays (either may be null), and (words non-null) the buffer they make: field_words(nvox) words, the
// header -- set when d_zyx is given -- then the cells.  tests/test_capi_field_cpu.py.
extern "C" int32_t mppi_debug_field_layout(const mppi_config* cfg, const mppi_field_desc* field, const float* origin3,
                                           const float* d_zyx, float* words) {
    if (!cfg) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_field_layout: bad arguments");
    mppi_status st = validate(*cfg);
    if (st != MPPI_OK) return st;
    mppi_scene use;
    if ((st = field_engine_validate(*cfg, nullptr, field, use)) != MPPI_OK) return st;   // (as mppi_create_scene_field with a null scene)
    if ((st = field_data_validate(*field, origin3, d_zyx)) != MPPI_OK) return st;
    if (words) {
        field_header(*field, origin3 ? origin3 : field->origin, d_zyx != nullptr, words);
        if (d_zyx) field_pack(*field, d_zyx, words + kFieldHdrW);
        else std::memset(words + kFieldHdrW, 0, sizeof(float) * 2 * (size_t)field_voxels(*field));
    }
    return MPPI_OK;
}

// Diagnostic (no GPU): field_sample, the kernels' own inline, on n points (n, 3) over a packed buffer
// (mppi_debug_field_layout's words): the values (n) and the eight nodes' linear indices (n, 8).
extern "C" int32_t mppi_debug_field_sample(const float* words, int32_t n, const float* pts, float* val, int32_t* idx8) {
    if (!words || n < 0 || (n > 0 && (!pts || !val))) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_field_sample: bad arguments");
    for (int32_t i = 0; i < n; ++i)
        val[i] = mppi::field_sample(words, words + kFieldHdrW, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2],
                                    idx8 ? idx8 + 8 * (size_t)i : nullptr);
    return MPPI_OK;
}

// Diagnostic (not part of the public header): the layout of a configuration without a device.
// out[0..27]: threads, L, R, nch, nb, iters, P, C, hp, fin_tsz, fin_ts, j0, chain_fast, sigma_diag,
// nq, qoff, state_dim, out_dim, generic; the output buffer's offsets of u0, stats, flags and xerr and
// its size; the trajectory's float count (low, high word); a 64-bit FNV-1a over the bytes of the
// layout's DevParams, then its FinParams (low, high word).  Returns validate's or layout_of's
// status (the message in mppi_last_error).
extern "C" int32_t mppi_debug_layout(const mppi_config* cfg, int32_t* out, int32_t n) {
    constexpr int kWords = 28;
    if (!cfg || !out || n < kWords) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_layout: bad arguments");
    mppi_status st = validate(*cfg);
    if (st != MPPI_OK) return st;
    EngineLayout l;
    if ((st = layout_of(*cfg, l)) != MPPI_OK) return st;
    uint64_t h = 0xCBF29CE484222325ull;
    for (const auto& [b, nb] : {std::pair<const void*, size_t>{&l.dp, sizeof(l.dp)}, {&l.fp, sizeof(l.fp)}})
        for (size_t i = 0; i < nb; ++i) h = (h ^ ((const unsigned char*)b)[i]) * 0x100000001B3ull;
    const uint64_t tf = traj_floats(&l);
    const int32_t w[kWords] = {l.threads, l.dp.L, l.dp.R, l.dp.nch, l.dp.nb, l.dp.iters, l.dp.P, l.C, l.dp.hp,
                               l.fin_tsz, l.fin_ts, l.dp.j0, l.dp.chain_fast, l.dp.sigma_diag, l.nq, l.qoff,
                               l.state_dim, l.out_dim, l.generic,
                               (int32_t)off_u0(&l), (int32_t)off_stats(&l), (int32_t)off_flags(&l), (int32_t)off_xerr(&l),
                               (int32_t)l.out_bytes, (int32_t)(uint32_t)tf, (int32_t)(uint32_t)(tf >> 32),
                               (int32_t)(uint32_t)h, (int32_t)(uint32_t)(h >> 32)};
    std::memcpy(out, w, sizeof(w));
    return MPPI_OK;
}
