// mppi_debug.cpp -- the diagnostics entry points of libmppi_hip.so (mppi_debug_*; not part of the
// public header, reached by name from the tests and tools/): launches described without a GPU, the
// MPPI_STAMPS readbacks and the native queue's probes.  Nothing here is on the step's path.  See
// mppi_engine.h for the file map.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mppi_elites.h"
#include "mppi_engine.h"

using namespace mppi;

namespace mppi_host {

std::string fin_symbol(const FinParams& f, LaunchDesc* desc) {
    LaunchDesc d{};
    const int rc = describe(f, &d);
    if (desc) *desc = d;
    return rc == 0 ? d.symbol : "?";
}
std::string roll_symbol(const DevParams& p, int threads, LaunchDesc* desc, const float* ttab, float* scene, const float* field, int self_members,
                        const float* limits) {
    LaunchDesc d{};
    const int rc = describe(p, threads, &d, ttab, scene, field, self_members, limits);
    if (desc) *desc = d;
    return rc == 0 ? d.symbol : "?";
}

}  // namespace mppi_host

using namespace mppi_host;

extern "C" {

static thread_local int32_t g_fin_launch[6];    // (mppi_debug_finalize_launch)
static thread_local int32_t g_roll_launch[6];   // (mppi_debug_rollout_launch)
// the captured launches' geometry, as native dispatch would store it in its packets
static void note_launches(const LaunchDesc& a, const LaunchDesc& b, int32_t (&out)[6]) {
    const LaunchDesc* ds[2] = {&a, &b};
    for (int i = 0; i < 2; ++i) {
        out[3 * i] = (int32_t)ds[i]->block[0];
        out[3 * i + 1] = (int32_t)ds[i]->grid[0];
        out[3 * i + 2] = (int32_t)ds[i]->lds;
    }
}
// Diagnostic (not part of the public header; no GPU): the finalize kernels a batch's descriptions
// would name for a launch of this shape -- g = {A, H, tsz, half, ts, window, nrec, mode, peer
// exchange, MPPI_GENERIC_KERNELS}: the last step's into `full`, the earlier steps' into `quiet`
// (the same symbol where no quiet kernel applies).  tests/test_capi_specialized_cpu.py.
int32_t mppi_debug_finalize_kernels(const int32_t* g, char* full, char* quiet, int32_t len) {
    if (!g || !full || !quiet || len <= 0) return MPPI_ERR_INVALID_ARG;
    static const FinTail tail{};
    static unsigned long long* const peers[1] = {nullptr};
    FinParams f;
    std::memset(&f, 0, sizeof(f));
    f.V = 1; f.A = g[0]; f.H = g[1]; f.tsz = g[2]; f.half = g[3]; f.ts = g[4]; f.window = g[5]; f.nrec = g[6];
    f.mode = g[7];
    f.tail = &tail;
    if (g[8]) f.xpeers = peers;
    f.kern = g[9] ? kFinKernGeneric : 0;
    LaunchDesc da{}, db{};
    const std::string a = fin_symbol(f, &da);
    f.kern = quiet_fin_kern(f.kern, g[9] ? kGenericAll : 0, false);   // (not under MPPI_GENERIC_KERNELS)
    const std::string b = fin_symbol(f, &db);
    snprintf(full, (size_t)len, "%s", a.c_str());
    snprintf(quiet, (size_t)len, "%s", b.c_str());
    note_launches(da, db, g_fin_launch);   // (mppi_debug_finalize_launch below)
    return (a == "?" || b == "?") ? MPPI_ERR_INVALID_ARG : MPPI_OK;
}

// Diagnostic (no GPU): {block threads, grid.x, dynamic LDS bytes} of the two launches the calling
// thread's last mppi_debug_finalize_kernels described, the full one then the quiet one.
// tests/test_capi_finalize_quads_cpu.py.
void mppi_debug_finalize_launch(int32_t* out6) {
    if (out6) std::memcpy(out6, g_fin_launch, sizeof(g_fin_launch));
}

// Likewise the rollout kernels of a batch -- g = {model, A, H, L, nch, iters, block threads, V,
// state_f64, noise mode, store_noise, cost_terms, full Sigma, peer exchange, MPPI_GENERIC_KERNELS}:
// the last step's into `full`, the earlier steps' into `quiet` (the same symbol where the full
// kernel runs on every step).  tests/test_capi_quiet_rollout_cpu.py.
int32_t mppi_debug_rollout_kernels(const int32_t* g, char* full, char* quiet, int32_t len) {
    if (!g || !full || !quiet || len <= 0) return MPPI_ERR_INVALID_ARG;
    DevParams p;
    std::memset(&p, 0, sizeof(p));
    p.model = g[0]; p.A = g[1]; p.H = g[2]; p.L = g[3]; p.nch = g[4]; p.iters = g[5]; p.V = g[7];
    p.R = p.L > 0 ? 64 / p.L : 0;
    p.state_f64 = g[8]; p.noise_mode = g[9]; p.store_noise = g[10]; p.cost_terms = g[11]; p.sigma_diag = !g[12];
    p.nb = 16; p.K = 16; p.store_traj = 1;
    p.chain_fast = 2;
    p.kern = g[14] ? kRollKernGeneric : 0;
    LaunchDesc da{}, db{};
    const std::string a = roll_symbol(p, g[6], &da);
    p.kern = quiet_roll_kern(p.kern, g[14] ? kGenericAll : 0, false, g[13] != 0, false);   // (no peer exchange, not under MPPI_GENERIC_KERNELS)
    const std::string b = roll_symbol(p, g[6], &db);
    snprintf(full, (size_t)len, "%s", a.c_str());
    snprintf(quiet, (size_t)len, "%s", b.c_str());
    note_launches(da, db, g_roll_launch);   // (mppi_debug_rollout_launch below)
    return (a == "?" || b == "?") ? MPPI_ERR_INVALID_ARG : MPPI_OK;
}

// Diagnostic (no GPU): {block threads, grid.x, dynamic LDS bytes} of the two launches the calling
// thread's last mppi_debug_rollout_kernels described, the full one then the quiet one.
// tests/test_capi_launch_table_cpu.py.
void mppi_debug_rollout_launch(int32_t* out6) {
    if (out6) std::memcpy(out6, g_roll_launch, sizeof(g_roll_launch));
}

// Likewise the plan kernel (mppi_plan.hip; mppi_get_plan) -- g = {model, A, H, V, state_f64,
// quad_literal_jinv}: "<symbol> grid <blocks> block <threads>" of its launch into `sym`.
// tests/test_capi_plan_cpu.py.
int32_t mppi_debug_plan_kernel(const int32_t* g, char* sym, int32_t len) {
    if (!g || !sym || len <= 0) return MPPI_ERR_INVALID_ARG;
    DevParams p;
    std::memset(&p, 0, sizeof(p));
    p.model = g[0]; p.A = g[1]; p.H = g[2]; p.V = g[3]; p.state_f64 = g[4]; p.q_literal_jinv = g[5];
    PlanParams pp;
    std::memset(&pp, 0, sizeof(pp));
    pp.self_members = -1;   // (not a self engine: no dynamic LDS)
    LaunchDesc d{};
    {   const mppi_aql::Capture c(&d);
        if (mppi_launch_plan(&p, &pp, nullptr) != 0) return MPPI_ERR_INVALID_ARG; }
    snprintf(sym, (size_t)len, "%s grid %u block %u", d.symbol, d.grid[0], d.block[0]);
    return MPPI_OK;
}

// Likewise the elite readback's launches (mppi_elites.hip; mppi_get_elites) -- g = {model, K, H, V, n}:
// "<symbol> grid <x>x<y> block <threads>" per launch, joined by "; ", the selection over the shares
// (when K takes more than one block) first.  tests/test_capi_elites_cpu.py.
int32_t mppi_debug_elite_kernel(const int32_t* g, char* sym, int32_t len) {
    if (!g || !sym || len <= 0) return MPPI_ERR_INVALID_ARG;
    EliteParams p;
    std::memset(&p, 0, sizeof(p));
    const int model = g[0];
    const bool has_ee = model == MPPI_MODEL_ARM || model == MPPI_MODEL_WHOLEBODY;
    p.K = g[1]; p.H = g[2]; p.V = g[3]; p.n = g[4];
    p.nstate = model == MPPI_MODEL_DRONE ? 3 : model == MPPI_MODEL_QUADROTOR ? 6 : model == MPPI_MODEL_ARM ? 7 : 10;
    p.has_ee = has_ee; p.C = p.nstate + (has_ee ? 12 : 0); p.Cr = p.nstate + (has_ee ? 16 : 0);
    p.t_major = model == MPPI_MODEL_QUADROTOR;
    p.pitch = ((p.t_major ? p.K : p.H) + 15) & ~15;
    static const float nowhere = 0.0f;   // the launches are described, not run: any non-null planes and rows
    p.planes = &nowhere; p.rows = const_cast<float*>(&nowhere);
    std::string all;
    for (int stage = 0; stage < 3; ++stage) {
        LaunchDesc d{};
        int rc;
        {   const mppi_aql::Capture c(&d);
            rc = mppi_launch_elites_stage(&p, stage, nullptr); }
        if (rc == 1) continue;
        if (rc != 0) return MPPI_ERR_INVALID_ARG;
        char one[256];
        snprintf(one, sizeof(one), "%s%s grid %ux%u block %u", all.empty() ? "" : "; ", d.symbol, d.grid[0], d.grid[1], d.block[0]);
        all += one;
    }
    if ((int)all.size() >= len) return MPPI_ERR_INVALID_ARG;
    snprintf(sym, (size_t)len, "%s", all.c_str());
    return MPPI_OK;
}

// Likewise the occupancy transform's launches (mppi_edt.hip; mppi_set_occupancy) -- g = {nx, ny, nz}:
// "<symbol> grid <x>x<y> block <threads> lds <bytes>" per launch, joined by "; ": the x pass, the y pass,
// the z pass, the finish.  tests/test_capi_occupancy_cpu.py.
int32_t mppi_debug_edt_kernels(const int32_t* g, char* sym, int32_t len) {
    if (!g || !sym || len <= 0) return MPPI_ERR_INVALID_ARG;
    static uint8_t nowhere8 = 0;   // the launches are described, not run: any non-null pointers
    static int32_t nowhere32 = 0;
    static float nowheref = 0.0f;
    EdtParams p;
    std::memset(&p, 0, sizeof(p));
    p.occ = &nowhere8; p.g_occ = p.g_free = &nowhere32; p.cells = &nowheref;
    p.nx = g[0]; p.ny = g[1]; p.nz = g[2];
    p.voxel = 1.0f; p.cap = 1.0f; p.window = 2;
    std::string all;
    for (int stage = 0; stage < 4; ++stage) {
        LaunchDesc d{};
        int rc;
        {   const mppi_aql::Capture c(&d);
            rc = mppi_launch_edt_stage(&p, stage, nullptr); }
        if (rc != 0) return MPPI_ERR_INVALID_ARG;
        char one[256];
        snprintf(one, sizeof(one), "%s%s grid %ux%u block %u lds %u", all.empty() ? "" : "; ", d.symbol, d.grid[0], d.grid[1],
                 d.block[0], d.lds);
        all += one;
    }
    if ((int)all.size() >= len) return MPPI_ERR_INVALID_ARG;
    snprintf(sym, (size_t)len, "%s", all.c_str());
    return MPPI_OK;
}

// Diagnostic (GPU): a field engine's whole field buffer as it stands on the device -- field_words(nvox)
// words, the header and both words of every x-pair (mppi_get_distance_field hands out the first of each).
// tests/test_gpu_occupancy.py.
int32_t mppi_debug_field_words(mppi_engine* e, float* words) {
    if (!e || !words || !e->d_field) return MPPI_ERR_INVALID_ARG;
    if (use_device(e)) return MPPI_ERR_HIP;
    return download(e, words, e->d_field, sizeof(float) * (size_t)field_words(field_voxels(e->field)));
}

// The host twin of the elites' order: the n first sample indices of S (K) under mppi_elites.h's key,
// the one the kernels select and sort by.  tests/test_capi_elites_cpu.py.
int32_t mppi_debug_elite_order(const float* S, int32_t K, int32_t n, int32_t* idx) {
    if (!S || !idx || K < 1 || n < 1 || n > K) return MPPI_ERR_INVALID_ARG;
    std::vector<unsigned long long> keys((size_t)K);
    for (int32_t k = 0; k < K; ++k) {
        uint32_t bits;
        std::memcpy(&bits, S + k, sizeof(bits));
        keys[(size_t)k] = elite_key(bits, (uint32_t)k);
    }
    std::partial_sort(keys.begin(), keys.begin() + n, keys.end());
    for (int32_t j = 0; j < n; ++j) idx[j] = (int32_t)(uint32_t)keys[(size_t)j];
    return MPPI_OK;
}

// Diagnostic (not part of the public header): mppi_aql step_touch on the engine's own queue
// (tools/probes.py rate_split).  Same thread as the control calls.
int32_t mppi_debug_queue_touch(mppi_engine* e) {
    if (!e || !e->aql) return MPPI_ERR_INVALID_ARG;
    std::string err;
    const int r = mppi_aql::step_touch(e->aql, false, &err);
    return r == 0 ? MPPI_OK : fail(MPPI_ERR_HIP, "queue touch: %s", err.c_str());
}

// Diagnostic (MPPI_STAMPS builds; not part of the public header): the raw per-wave stamps
// of the last rollout launch, kStamps uint64 per wave.  Returns the wave count (0 when the
// engine has no stamps) or a negative status.
int64_t mppi_debug_stamps(mppi_engine* e, unsigned long long* out, int64_t max_waves) {
    if (!e || !out) return MPPI_ERR_INVALID_ARG;
    if (!e->d_stamps) return 0;
    if (use_device(e)) return MPPI_ERR_HIP;
    const int64_t nwaves = std::min<int64_t>(max_waves, (int64_t)e->V * e->dp.nb * (e->threads / 64));
    if (hipStreamSynchronize(e->stream) != hipSuccess ||
        hipMemcpy(out, e->d_stamps, (size_t)nwaves * kStamps * 8, hipMemcpyDeviceToHost) != hipSuccess)
        return MPPI_ERR_HIP;
    return nwaves;
}

// Diagnostic (MPPI_STAMPS builds): the raw stamps of the last FINAL (which = 0) or PACK
// (which = 1) launch, kStamps uint64 per (vehicle, dim, t-slice) block.  Returns the block count.
int64_t mppi_debug_fstamps(mppi_engine* e, unsigned long long* out, int64_t max_blocks, int32_t which) {
    if (!e || !out || which < 0 || which > 1) return MPPI_ERR_INVALID_ARG;
    if (!e->d_fstamps) return 0;
    if (use_device(e)) return MPPI_ERR_HIP;
    const int64_t nb = (int64_t)e->V * e->A * e->fin_ts;
    const int64_t n = std::min<int64_t>(max_blocks, nb);
    if (hipStreamSynchronize(e->stream) != hipSuccess ||
        hipMemcpy(out, e->d_fstamps + (size_t)which * nb * kStamps, (size_t)n * kStamps * 8, hipMemcpyDeviceToHost) !=
            hipSuccess)
        return MPPI_ERR_HIP;
    return n;
}

// Diagnostic: mppi_aql step_ring (the doorbell again, no packet).  Refused while the prewarm thread
// runs: step_ring must come from the thread that writes the packets (mppi_aql.h).
int32_t mppi_debug_queue_ring(mppi_engine* e) {
    if (!e || !e->aql) return MPPI_ERR_INVALID_ARG;
    if (e->pw_us.load()) return fail(MPPI_ERR_STATE, "mppi_debug_queue_ring: the prewarm thread also writes packets");
    mppi_aql::step_ring(e->aql);
    return MPPI_OK;
}

// Diagnostic (no GPU): the launches a step path hands to the launchers, for a configuration and
// sw = {path (0 mppi_run_steps through HIP, 1 mppi_step through HIP -- or, as on a shard without
// a communicator, the split phases -- 2 the native batch, 3 the native control call), n steps (a call: 1), peer exchange connected, engine-owned communicator,
// per-launch timing, MPPI_GENERIC_KERNELS bits, MPPI_DEBUG_OUT}.  The engine is built on the host
// from layout_of: its device pointers are null but for the two the step offsets (d_tail, a shard's
// d_exchange: fixed stand-in addresses, like the peer regions, the communicator and an INJECTED
// noise buffer), the state is the zero state, and nothing is launched or allocated on a device.
// One line per launch into buf -- "<early|last> <rollout|pack|finalize> <symbol> grid <x> block <x>
// lds <bytes> args <bytes> fnv <FNV-1a 64 of the argument bytes>" -- for a step before the last
// (n > 1) and for the last step.  A path the engine would not take is refused (mppi_last_error says
// why).  tests/test_capi_step_launches_cpu.py.
static int32_t step_launches(const mppi_config* cfg, const int32_t* sw, char* buf, int32_t len, const mppi_scene* scene,
                             const mppi_field_desc* field = nullptr, uint64_t* field_arg = nullptr,
                             const mppi_self_collision* self = nullptr, const mppi_limits* limits = nullptr) {
    if (!cfg || !sw || !buf || len <= 0 || sw[0] < 0 || sw[0] > 3 || sw[1] < 1)
        return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_step_launches: bad arguments");
    mppi_status st = validate(*cfg);
    if (st != MPPI_OK) return st;
    if (limits && (st = limits_validate(*cfg, limits)) != MPPI_OK) return st;
    const auto eng = std::make_unique<mppi_engine>();
    mppi_engine* e = eng.get();
    if (self) {   // a self engine's (mppi_create_scene_self; with a scene): its block and its paired spheres
        if (!scene) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_self_step_launches: a self engine has a scene");
        if ((st = scene_validate(*cfg, *scene)) != MPPI_OK || (st = self_validate(*cfg, *scene, self)) != MPPI_OK) return st;
        if ((st = self_layout(*cfg, self_member_count(*self), *e)) != MPPI_OK) return st;
        e->has_self = true;
        e->self_members = self_member_count(*self);
    } else if ((st = layout_of(*cfg, *e)) != MPPI_OK) {
        return st;
    }
    const int path = sw[0], n = path == 1 || path == 3 ? 1 : sw[1];
    const auto stand_in = [](uintptr_t a) { return (void*)a; };
    set_generic(*e, sw[5]);
    e->timing = sw[4] != 0;
    e->out_dbg = sw[6];
    e->d_tail = (FinTail*)stand_in(0x1000);
    e->fp.tail = e->d_tail + kTailFinal;
    if (sw[3]) e->comm = (ncclComm_t)stand_in(0x10);
    if (sw[2]) {   // (as mppi_peer_open / peer_bind)
        if (e->V != 1) return fail(MPPI_ERR_STATE, "peer exchange: one vehicle per engine (V = %d)", e->V);
        e->peer = true;
        e->fp.xpeers = (unsigned long long* const*)stand_in(0x2000);
        e->fp.xlocal = (unsigned long long*)stand_in(0x3000);
        e->fp.xn = e->cfg.shard_count; e->fp.xme = e->cfg.shard_rank;
        e->fp.xdec = (unsigned long long*)stand_in(0x4000);
    }
    if (sharded(e)) e->d_exchange = (float*)stand_in(0x100000);
    if (e->cfg.cost_terms & MPPI_COST_TARGET_TRACK) e->d_ttab = (float*)stand_in(0x6000);
    if (scene) {   // a scene engine's (mppi_create_scene): its buffer and, always, a target table
        if ((st = scene_validate(e->cfg, *scene)) != MPPI_OK) return st;
        e->has_scene = true;
        e->d_ttab = (float*)stand_in(0x6000);
        e->d_scene = (float*)stand_in(0x7000);
    }
    if (field) {   // a field engine's (mppi_create_scene_field; with a scene): its field buffer
        if (!scene) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_field_step_launches: a field engine has a scene");
        if ((st = field_validate(field)) != MPPI_OK) return st;
        e->has_field = true;
        e->field = *field;
        e->d_field = (float*)stand_in(0x8000);
    }
    if (limits) {   // a bounded engine's (mppi_create_limits): its limits buffer
        e->has_limits = true;
        e->limits = *limits;
        e->d_limits = (float*)stand_in(0x9000);
    }
    std::vector<VehicleConst> vc((size_t)e->V);
    e->h_vc = vc.data();
    e->tpos.assign((size_t)3 * e->V, 0.0f);
    e->tquat.assign((size_t)4 * e->V, 0.0f);
    e->state.assign((size_t)e->state_dim * e->V, 0.0);
    for (int v = 0; v < e->V; ++v) {
        e->tquat[4 * v + 3] = 1.0f;
        if (e->cfg.model == MPPI_MODEL_ARM || e->cfg.model == MPPI_MODEL_WHOLEBODY) e->state[(size_t)v * e->state_dim + 6] = 1.0;
    }
    build_vehicle_consts(e);
    const bool philox = e->cfg.noise_mode == MPPI_NOISE_PHILOX;
    const float* noise = philox ? nullptr : (const float*)stand_in(0x5000);
    // the paths' own conditions (mppi_run_steps, mppi_step, run_steps_aql, control_call_aql)
    if (path != 1 && !philox) return fail(MPPI_ERR_STATE, "mppi_run_steps and native dispatch need device noise");
    if (path == 2)
        if (const char* why = aql_ineligible(e, true)) return fail(MPPI_ERR_STATE, "native dispatch: %s", why);
    if (path == 3) {
        if (e->V != 1 || sharded(e)) return fail(MPPI_ERR_STATE, "native control call: one vehicle, not sharded");
        if (const char* why = aql_ineligible(e)) return fail(MPPI_ERR_STATE, "native dispatch: %s", why);
    }
    std::string all;
    int bad = 0;
    const auto report = [&](bool last, const char* kind, int rc, const LaunchDesc& d) {
        if (rc != 0) { bad = rc; return; }
        uint64_t h = 0xCBF29CE484222325ull;
        for (uint32_t i = 0; i < d.arg_bytes; ++i) h = (h ^ d.args[i]) * 0x100000001B3ull;
        char one[320];
        snprintf(one, sizeof(one), "%s %s %s grid %u block %u lds %u args %u fnv %016llx\n", last ? "last" : "early", kind,
                 d.symbol, d.grid[0], d.block[0], d.lds, d.arg_bytes, (unsigned long long)h);
        all += one;
    };
    LaunchDesc d{};
    for (int i = n > 1 ? n - 2 : n - 1; i < n; ++i) {   // a step before the last, then the last
        const bool last = i == n - 1;
        const StepPath sp = path < 2 ? StepPath::Hip : path == 2 ? StepPath::Batch : StepPath::Call;
        DevParams p = rollout_params(e, sp, noise, !last);
        if (sp == StepPath::Hip) p.step_ctr = (uint32_t)i;   // (rollout_impl: the launch's own)
        report(last, "rollout", describe(p, e->threads, &d, e->d_ttab, e->d_scene, e->d_field, e->self_members, e->d_limits), d);
        if (field_arg) std::memcpy(field_arg, d.args + kRollFieldOff, sizeof(*field_arg));   // (the last rollout's)
        if (sp == StepPath::Hip && sharded(e)) {
            const FinParams f = finalize_params(e, FinKind::Pack);
            report(last, "pack", describe(f, &d), d);
        }
        FinParams f = finalize_params(e, FinKind::Final, sp, !last);
        if (sp == StepPath::Hip) {   // (finalize_impl: the launch's own)
            if (last) f.seq = 1u;    // the first fresh sequence number
            if (e->out_dbg == 1 && !last) f.tail = e->d_tail + kTailScratch;
        }
        report(last, "finalize", describe(f, &d), d);
    }
    if (bad) return fail(MPPI_ERR_INVALID_ARG, "no kernel for a launch of this step (%d)", bad);
    if ((int)all.size() >= len) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_step_launches: %zu bytes needed", all.size() + 1);
    snprintf(buf, (size_t)len, "%s", all.c_str());
    return MPPI_OK;
}
int32_t mppi_debug_step_launches(const mppi_config* cfg, const int32_t* sw, char* buf, int32_t len) {
    return step_launches(cfg, sw, buf, len, nullptr);
}
// Diagnostic (no GPU): the outputs the host forms for a QUADROTOR or AERIAL configuration -- the base's first step
// under u0 (quad_outputs; AERIAL: aerial_outputs picks the base rows out of its state) -- into out12, and (vc non-null)
// the vehicle constants build_vehicle_consts makes of `state` for vehicle 0: pos0f then vel0f (2 x 16 floats), then base
// (12).  The engine is built on the host from layout_of, as in step_launches.  tests/test_capi_aerial_cpu.py.
int32_t mppi_debug_base_outputs(const mppi_config* cfg, const double* state, const float* u0, double* out12, float* vc44) {
    if (!cfg || !state || !u0 || !out12) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_base_outputs: bad arguments");
    mppi_status st = validate(*cfg);
    if (st != MPPI_OK) return st;
    if (cfg->model != MPPI_MODEL_QUADROTOR && cfg->model != MPPI_MODEL_AERIAL)
        return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_base_outputs: the QUADROTOR and AERIAL models form outputs on the host");
    const auto eng = std::make_unique<mppi_engine>();
    mppi_engine* e = eng.get();
    if ((st = layout_of(*cfg, *e)) != MPPI_OK) return st;
    std::vector<VehicleConst> vc((size_t)e->V);
    e->h_vc = vc.data();
    e->tpos.assign((size_t)3 * e->V, 0.0f);
    e->tquat.assign((size_t)4 * e->V, 0.0f);
    e->state.assign((size_t)e->state_dim * e->V, 0.0);
    std::memcpy(e->state.data(), state, sizeof(double) * (size_t)e->state_dim);
    for (int v = 0; v < e->V; ++v) e->tquat[4 * v + 3] = 1.0f;
    build_vehicle_consts(e);
    if (cfg->model == MPPI_MODEL_AERIAL) aerial_outputs(e, e->state.data(), u0, out12);
    else quad_outputs(e, e->state.data(), u0, out12);
    if (vc44) {
        std::memcpy(vc44, vc[0].pos0f, sizeof(float) * 16);
        std::memcpy(vc44 + 16, vc[0].vel0f, sizeof(float) * 16);
        std::memcpy(vc44 + 32, vc[0].base, sizeof(float) * 12);
    }
    e->h_vc = nullptr;
    return MPPI_OK;
}
// Likewise for an engine of mppi_create_scene(cfg, scene) (a null scene: mppi_debug_step_launches).
// tests/test_capi_obstacles_cpu.py.
int32_t mppi_debug_scene_step_launches(const mppi_config* cfg, const mppi_scene* scene, const int32_t* sw, char* buf,
                                       int32_t len) {
    return step_launches(cfg, sw, buf, len, scene);
}

// Likewise for an engine of mppi_create_scene_field(cfg, scene, field); field_arg (may be null): the 8 bytes
// at the field pointer's offset (kRollFieldOff) of the last rollout's argument block -- the stand-in
// field buffer is at 0x8000.  tests/test_capi_field_cpu.py.
int32_t mppi_debug_field_step_launches(const mppi_config* cfg, const mppi_scene* scene, const mppi_field_desc* field,
                                       const int32_t* sw, char* buf, int32_t len, uint64_t* field_arg) {
    if (!scene || !field) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_field_step_launches: bad arguments");
    return step_launches(cfg, sw, buf, len, scene, field, field_arg);
}

// Likewise for an engine of mppi_create_scene_self(cfg, scene, field, self) (field may be null).
// tests/test_capi_self_collision_cpu.py.
int32_t mppi_debug_self_step_launches(const mppi_config* cfg, const mppi_scene* scene, const mppi_field_desc* field,
                                      const mppi_self_collision* self, const int32_t* sw, char* buf, int32_t len) {
    if (!scene || !self) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_self_step_launches: bad arguments");
    return step_launches(cfg, sw, buf, len, scene, field, nullptr, self);
}

// Likewise for an engine of mppi_create_limits(cfg, limits) (null limits: mppi_debug_step_launches); the stand-in
// limits buffer is at 0x9000.  tests/test_capi_limits_cpu.py.
int32_t mppi_debug_limits_step_launches(const mppi_config* cfg, const mppi_limits* limits, const int32_t* sw, char* buf,
                                        int32_t len) {
    return step_launches(cfg, sw, buf, len, nullptr, nullptr, nullptr, nullptr, limits);
}

// Diagnostic (no GPU): mppi_set_limits' status on an engine built on the host from layout_of -- a plain one (bounded
// 0), or one marked bounded: the call's argument and state checks, which come before it touches a device (a
// bounded engine with valid bounds would go on to the device: MPPI_OK is returned for it here without the call).
int32_t mppi_debug_limits_set(const mppi_config* cfg, int32_t bounded, const mppi_limits* limits) {
    if (!cfg) return fail(MPPI_ERR_INVALID_ARG, "mppi_debug_limits_set: bad arguments");
    mppi_status st = validate(*cfg);
    if (st != MPPI_OK) return st;
    const auto eng = std::make_unique<mppi_engine>();
    if ((st = layout_of(*cfg, *eng)) != MPPI_OK) return st;
    eng->has_limits = bounded != 0;
    if (eng->has_limits && limits_values_validate(limits) == MPPI_OK) return MPPI_OK;
    return mppi_set_limits(eng.get(), limits);
}

// Likewise the bounded plan kernel (mppi_debug_plan_kernel's g): "<symbol> grid <blocks> block <threads>".
int32_t mppi_debug_limits_plan_kernel(const int32_t* g, char* sym, int32_t len) {
    if (!g || !sym || len <= 0) return MPPI_ERR_INVALID_ARG;
    DevParams p;
    std::memset(&p, 0, sizeof(p));
    p.model = g[0]; p.A = g[1]; p.H = g[2]; p.V = g[3]; p.state_f64 = g[4]; p.q_literal_jinv = g[5];
    PlanParams pp;
    std::memset(&pp, 0, sizeof(pp));
    pp.self_members = -1;
    static const float nowhere[kLimitsW] = {};   // described, not run: any non-null buffer
    LaunchDesc d{};
    {   const mppi_aql::Capture c(&d);
        if (mppi_launch_plan_b(&p, &pp, nowhere, nullptr) != 0) return MPPI_ERR_INVALID_ARG; }
    snprintf(sym, (size_t)len, "%s grid %u block %u", d.symbol, d.grid[0], d.block[0]);
    return MPPI_OK;
}

static int32_t scene_rollout_kernels(const int32_t* g, char* full, char* quiet, int32_t len, bool field, int self_members = -1);
// mppi_debug_rollout_kernels for a scene engine's launches (same g): the scene kernel into both.
int32_t mppi_debug_scene_rollout_kernels(const int32_t* g, char* full, char* quiet, int32_t len) {
    return scene_rollout_kernels(g, full, quiet, len, false);
}
// and for a field engine's: the field kernel into both.
int32_t mppi_debug_field_rollout_kernels(const int32_t* g, char* full, char* quiet, int32_t len) {
    return scene_rollout_kernels(g, full, quiet, len, true);
}
// and for a self engine's (g[15]: with a field; g[16]: the paired spheres): the self kernel into both.
int32_t mppi_debug_self_rollout_kernels(const int32_t* g, char* full, char* quiet, int32_t len) {
    if (!g || g[16] < 0) return MPPI_ERR_INVALID_ARG;
    return scene_rollout_kernels(g, full, quiet, len, g[15] != 0, g[16]);
}
static int32_t scene_rollout_kernels(const int32_t* g, char* full, char* quiet, int32_t len, bool field, int self_members) {
    if (!g || !full || !quiet || len <= 0) return MPPI_ERR_INVALID_ARG;
    DevParams p;
    std::memset(&p, 0, sizeof(p));
    p.model = g[0]; p.A = g[1]; p.H = g[2]; p.L = g[3]; p.nch = g[4]; p.iters = g[5]; p.V = g[7];
    p.R = p.L > 0 ? 64 / p.L : 0;
    p.state_f64 = g[8]; p.noise_mode = g[9]; p.store_noise = g[10]; p.cost_terms = g[11]; p.sigma_diag = !g[12];
    p.nb = 16; p.K = 16; p.store_traj = 1;
    p.chain_fast = 2;
    p.kern = g[14] ? kRollKernGeneric : 0;
    static float nowhere[4];   // described, not run: any non-null table and scene
    LaunchDesc da{}, db{};
    const std::string a = roll_symbol(p, g[6], &da, nowhere, nowhere, field ? nowhere : nullptr, self_members);
    p.kern = quiet_roll_kern(p.kern, g[14] ? kGenericAll : 0, false, g[13] != 0, false);
    const std::string b = roll_symbol(p, g[6], &db, nowhere, nowhere, field ? nowhere : nullptr, self_members);
    snprintf(full, (size_t)len, "%s", a.c_str());
    snprintf(quiet, (size_t)len, "%s", b.c_str());
    note_launches(da, db, g_roll_launch);
    return (a == "?" || b == "?") ? MPPI_ERR_INVALID_ARG : MPPI_OK;
}

}  // extern "C"
