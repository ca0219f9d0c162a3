// mppi_launches.cpp -- what every launch of the step's kernels is handed (mppi_engine.h): the two
// launch-parameter builders with the quiet rule, the launches described instead of made, and the
// native paths' description cache.  No device call: mppi_debug_step_launches runs all of it on an
// engine built on the host (tests/test_capi_step_launches_cpu.py).
#include <cstddef>
#include <cstring>

#include "mppi_engine.h"

using namespace mppi;

namespace mppi_host {

// the rollout's per-block partial records (DevParams::hdr / rdata layout)
static void block_records(const mppi_engine* e, FinParams& f) {
    const int64_t nb = e->dp.nb, H = e->H;
    f.nrec = (int32_t)nb;
    f.hdr = e->d_hdr; f.hdr_vs = nb * 4; f.hdr_rs = 4;
    f.dat = e->d_rdata; f.d_vs = (int64_t)e->A * nb * H; f.d_as = nb * H; f.d_rs = H;
}

// The finalize's record source: the rollout blocks' records, or the exchange slots of a shard.
static void final_records(const mppi_engine* e, FinParams& f) {
    if (sharded(e)) {   // slots [shard][v][P]: header then N[a][t]
        const int64_t P = e->dp.P;
        f.nrec = e->cfg.shard_count;
        f.hdr = e->d_exchange; f.hdr_vs = P; f.hdr_rs = (int64_t)e->V * P;
        f.dat = e->d_exchange + kHdr; f.d_vs = P; f.d_as = e->H; f.d_rs = (int64_t)e->V * P;
    } else {
        block_records(e, f);
    }
}

// the engine's side of the quiet rule (mppi_engine.h quiet_fin_kern): diagnostics that read every step
static bool step_diagnostics(const mppi_engine* e) {
    return e->timing || e->d_stamps || e->d_fstamps || e->out_dbg || e->no_flag_dbg || e->overlap;
}

DevParams rollout_params(const mppi_engine* e, StepPath path, const float* d_noise, bool quiet) {
    DevParams p = e->dp;
    p.noise_in = d_noise;
    p.vc0 = e->h_vc[0];
    if (path != StepPath::Hip) {
        p.step_ctr = 0u;
        p.noise_mode |= kNoiseStepFromId;
    }
    if (quiet) p.kern = quiet_roll_kern(p.kern, e->generic, step_diagnostics(e), e->peer, sharded(e));
    return p;
}

FinParams finalize_params(const mppi_engine* e, FinKind kind, StepPath path, bool quiet) {
    FinParams f = e->fp;
    if (kind == FinKind::Pack) {
        pack_fields(e, f);
        f.tail = e->d_tail + kTailPack;
        if (f.stamps) f.stamps += (size_t)e->V * e->A * e->fin_ts * kStamps;   // diagnostics: PACK's own blocks
        block_records(e, f);
        return f;
    }
    f.mode = kind == FinKind::Readback ? 2 : 0;
    f.seq = path == StepPath::Call ? kSeqFromVc : 0u;   // (0: no completion flag, and no fence)
    final_records(e, f);
    if (kind == FinKind::Scratch) {
        bind_outputs(f, e->d_out, e);
        f.wraw = nullptr;
        f.wsmooth = nullptr;
        f.tail = e->d_tail + kTailScratch;
    } else if (kind == FinKind::Readback) {
        f.tail = e->d_tail + kTailReadback;
    } else if (quiet) {
        f.kern = quiet_fin_kern(f.kern, e->generic, step_diagnostics(e));
    }
    return f;
}

int describe(const DevParams& p, int threads, LaunchDesc* d, const float* ttab, float* scene, const float* field, int self_members,
             const float* limits) {
    const mppi_aql::Capture c(d);
    return launch_rollout(p, ttab, threads, nullptr, scene, field, self_members, limits);
}
int describe(const FinParams& f, LaunchDesc* d) {
    const mppi_aql::Capture c(d);
    return mppi_launch_finalize(&f, nullptr);
}

}  // namespace mppi_host

using namespace mppi_host;

bool DescCache::matches(const DevParams& p_, const FinParams& f_, int threads_, bool ignore_vc0) const {
    constexpr size_t kVo = offsetof(DevParams, vc0), kVe = kVo + sizeof(VehicleConst);
    if (!valid || threads != threads_ || std::memcmp(&f_, &f, sizeof(f)) != 0) return false;
    if (!ignore_vc0) return std::memcmp(&p_, &p, sizeof(p)) == 0;
    return std::memcmp(&p_, &p, kVo) == 0 &&
           std::memcmp((const char*)&p_ + kVe, (const char*)&p + kVe, sizeof(DevParams) - kVe) == 0;
}

int DescCache::refresh(const DevParams& p_, const FinParams& f_, int threads_, const DevParams* p_quiet,
                       const FinParams* f_quiet) {
    valid = false;
    int rc;
    if ((rc = describe(p_, threads_, &roll, ttab, scene, field, self_members, limits)) != 0 ||
        (p_quiet && (rc = describe(*p_quiet, threads_, &roll_quiet, ttab, scene, field, self_members, limits)) != 0) ||
        (rc = describe(f_, &fin)) != 0 || (f_quiet && (rc = describe(*f_quiet, &fin_quiet)) != 0))
        return rc;
    p = p_;
    f = f_;
    threads = threads_;
    valid = true;
    return 0;
}
