// mppi_step.cpp -- the control step of libmppi_hip.so (include/mppi_hip.h): the rollout and
// finalize launches on the engine's stream, the tagged output records and their wait, mppi_step /
// mppi_run_steps, and the native dispatch of both (raw AQL packets, mppi_aql.cpp).  See
// mppi_engine.h for the file map and DESIGN.md §2 for the dispatch and completion protocols.
#include <emmintrin.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mppi_elites.h"
#include "mppi_engine.h"

using namespace mppi;

namespace mppi_host {

const char* aql_ineligible(const mppi_engine* e, bool batch) {
    if (e->aql_mode == 0) return "MPPI_DISPATCH=hip";
    if (sharded(e)) return "sharded step (its collective runs on the HIP stream)";
    if (e->timing) return "per-launch timing events (mppi_enable_timing)";
    if (e->d_stamps && !batch) return "stamps diagnostics";
    if (e->out_dbg || (e->no_flag_dbg && !batch)) return "output diagnostics";
    return nullptr;
}

}  // namespace mppi_host

using namespace mppi_host;

// True when every output record of the pending read step carries its sequence number (the
// tag is each record's last word; k_finalize writes a record with one 16 B store).
static bool records_tagged(const mppi_engine* e, uint32_t want) {
    const volatile uint32_t* r = (const volatile uint32_t*)(e->h_out + off_flags(e));
    const size_t n = rec_count(e);
    for (size_t i = 0; i < n; ++i)
        if (r[4 * i + 3] != want) return false;
    return true;
}

// Polls until every record carries `want` (true).  Every 256 polls the backstop is asked: when it
// returns true the wait ends there (false), with the backstop's status in *st.
template <class Backstop>
static bool poll_records(const mppi_engine* e, uint32_t want, mppi_status* st, Backstop stop) {
    *st = MPPI_OK;
    for (uint64_t it = 1;; ++it) {
        if (records_tagged(e, want)) return true;
        if ((it & 255u) == 0 && stop(st)) return false;
        __builtin_ia32_pause();
    }
}

static mppi_status rollout_impl(mppi_engine* e, const float* d_noise, bool quiet) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (!e->state_set) return fail(MPPI_ERR_STATE, "mppi_rollout before mppi_set_state");
    if (e->cfg.noise_mode == MPPI_NOISE_INJECTED && !d_noise)
        return fail(MPPI_ERR_INVALID_ARG, "INJECTED noise mode needs a device noise buffer");
    if (sharded(e) && !e->d_exchange)
        return fail(MPPI_ERR_STATE, "shard_count > 1 needs mppi_bind_exchange or mppi_comm_init");
    if (use_device(e)) return MPPI_ERR_HIP;
    DevParams p = rollout_params(e, StepPath::Hip, d_noise, quiet);
    p.step_ctr = e->step_ctr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (e->timing) { e0 = pool_event(e); e1 = pool_event(e); HIP_TRY(hipEventRecord(e0, e->stream)); }
    int rc = launch_rollout(p, e->d_ttab, e->threads, e->stream, e->d_scene, e->d_field, e->self_members, e->d_limits);
    if (rc != 0) return fail(MPPI_ERR_HIP, "rollout launch failed (%d: %s)", rc,
                             rc > 0 ? hipGetErrorString((hipError_t)rc) : "no kernel for this model/A/H");
    if (e->timing) {
        HIP_TRY(hipEventRecord(e1, e->stream));
        e->roll_pairs.emplace_back(e0, e1);
        if (e->roll_pairs.size() >= 2048) { mppi_status st = drain_timing(e); if (st) return st; }
    }
    if (sharded(e)) {   // fold this shard's block records into its exchange slot
        const FinParams f = finalize_params(e, FinKind::Pack);
        rc = mppi_launch_finalize(&f, e->stream);
        if (rc != 0) return fail(MPPI_ERR_HIP, "pack launch failed (%d)", rc);
    }
    return MPPI_OK;
}

extern "C" {

mppi_status mppi_rollout(mppi_engine* e, const float* d_noise) { return rollout_impl(e, d_noise, false); }

static std::string kernels_text(const std::string& roll, const std::string& fin, const std::string* quiet,
                                const std::string* roll_quiet = nullptr) {
    std::string s = "rollout " + roll + ", finalize " + fin;
    if (quiet) s += ", quiet finalize " + (*quiet == fin ? std::string("none") : *quiet);
    if (roll_quiet) s += ", quiet rollout " + (*roll_quiet == roll ? std::string("none") : *roll_quiet);
    return s;
}

// record_out: mark the outputs' completion with ev_out (read_outputs waits on it).
// Back-to-back steps (mppi_run_steps) mark only the last one: an event record is
// a queue packet of its own, ~1 us of device time per step.
// quiet: a step of a batch before its last (never read): the quiet FINAL where one applies.
static mppi_status finalize_impl(mppi_engine* e, bool record_out, bool quiet = false) {
    if (use_device(e)) return MPPI_ERR_HIP;
    FinParams f = finalize_params(e, FinKind::Final, StepPath::Hip, quiet && !record_out);   // (no completion flag yet)
    if (record_out && !e->no_flag_dbg) {   // a fresh value per read step, never 0 (the flags start zeroed):
                                           // the flags the previous read step left can never satisfy this
                                           // step's wait
        f.seq = ++e->seq_ctr & 0x7FFFFFFFu;   // (bit 31: native control calls' numbers)
        if (f.seq == 0u) f.seq = ++e->seq_ctr & 0x7FFFFFFFu;
    }
    if (e->out_dbg == 1 && !record_out) f.tail = e->d_tail + kTailScratch;   // diagnostic (MPPI_DEBUG_OUT)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (e->timing) { e0 = pool_event(e); e1 = pool_event(e); HIP_TRY(hipEventRecord(e0, e->stream)); }
    int rc = mppi_launch_finalize(&f, e->stream);
    if (rc != 0) return fail(MPPI_ERR_HIP, "finalize launch failed (%d)", rc);
    if (e->timing) { HIP_TRY(hipEventRecord(e1, e->stream)); e->fin_pairs.emplace_back(e0, e1); }
    if (record_out) e->out_seq = f.seq;
    if (record_out) HIP_TRY(hipEventRecord(e->ev_out, e->stream));   // outputs land in mapped host memory
    ++e->step_ctr;
    e->pending = record_out ? Pending::Hip : Pending::None;
    return MPPI_OK;
}

mppi_status mppi_finalize(mppi_engine* e) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    return finalize_impl(e, true);
}

// One output record, read with one aligned 16 B load (atomic on x86-64 processors with AVX),
// so its values and its tag come from the same store.  false: the tag is not this step's.
static inline bool load_record(const mppi_engine* e, size_t i, uint32_t want, uint32_t (&w)[4]) {
    const __m128i x = _mm_load_si128((const __m128i*)(e->h_out + off_flags(e)) + i);
    _mm_storeu_si128((__m128i*)w, x);
    return w[3] == want;
}

// Wait for the finalised step's outputs.  k_finalize writes them into mapped host memory
// as tagged records (the step's sequence number in each), so the host sees completion by
// polling host memory instead of waking on the output event (which also trails the kernel
// by one queue packet).  The event stays the backstop: it is queried every few hundred
// polls, which also surfaces a faulted queue as an error.
static mppi_status wait_outputs(mppi_engine* e) {
    mppi_status st;
    switch (e->pending) {
    case Pending::None: return MPPI_OK;
    case Pending::Batch: return aql_join(e);   // its completion signal (system-scope release)
    case Pending::Hip: break;                  // (below)
    case Pending::Call: {   // its flags, the queue's error state as the backstop
        const auto t0 = std::chrono::steady_clock::now();
        if (!poll_records(e, e->out_seq, &st, [&](mppi_status* s) {
                if (const int q = mppi_aql::step_error(e->aql)) *s = fail(MPPI_ERR_HIP, "native queue error %d", q);
                else if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60))
                    *s = fail(MPPI_ERR_HIP, "native control call: no outputs after 60 s");
                return *s != MPPI_OK;
            }))
            return st;
        std::atomic_thread_fence(std::memory_order_acquire);
        mppi_aql::step_call_read(e->aql);
        e->call_wait_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        return MPPI_OK;
    }
    }
    if (!e->event_wait) {
        if (poll_records(e, e->out_seq, &st, [&](mppi_status* s) {   // true: the event has fired, or failed
                const hipError_t q = hipEventQuery(e->ev_out);
                if (q != hipSuccess && q != hipErrorNotReady) *s = fail(MPPI_ERR_HIP, "waiting for the step: %s", hipGetErrorString(q));
                return q != hipErrorNotReady;
            })) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return MPPI_OK;
        }
        if (st != MPPI_OK) return st;
    }
    HIP_TRY(hipEventSynchronize(e->ev_out));
    return MPPI_OK;
}

// Diagnostic (MPPI_STAMPS): n blocks' (or waves') stamps added to their phase sums, in program order.
static mppi_status add_stamps(const unsigned long long* d_stamps, size_t n, const std::vector<int>& order,
                              std::vector<double>& sum, int64_t& count) {
    std::vector<unsigned long long> st(n * kStamps);
    HIP_TRY(hipMemcpy(st.data(), d_stamps, st.size() * 8, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < n; ++b) {
        const unsigned long long* x = &st[b * kStamps];
        for (size_t i = 1; i < order.size(); ++i) sum[i] += (double)(x[order[i]] - x[order[i - 1]]);
    }
    count += (int64_t)n;
    return MPPI_OK;
}

// The read step's outputs from its records into host staging in the plain arrays' layout
// (qdes/vdes or x/v per dim, u0, stats).  The plain arrays are the base (the quadrotor's
// outputs are formed on the host from u0).
static mppi_status assemble_records(mppi_engine* e) {
    const int V = e->V, A = e->A, od = e->out_dim, model = e->cfg.model, qoff = e->qoff, nq = e->nq;
    const uint32_t want = e->out_seq;
    e->rec_out.assign((const double*)e->h_out, (const double*)e->h_out + (size_t)V * od);
    e->rec_u0.resize((size_t)V * A);
    e->rec_stats.resize((size_t)V * 4);
    uint32_t w[4];
    for (int v = 0; v < V; ++v) {
        const size_t r0 = (size_t)v * (2 * A + 1);
        for (int a = 0; a < A; ++a) {
            double o1, o2;
            if (!load_record(e, r0 + 2 * a, want, w)) return fail(MPPI_ERR_STATE, "output record (%d,%d) not tagged", v, a);
            std::memcpy(&o1, w, 8);
            std::memcpy(&e->rec_u0[(size_t)v * A + a], &w[2], 4);
            if (!load_record(e, r0 + 2 * a + 1, want, w)) return fail(MPPI_ERR_STATE, "output record (%d,%d) not tagged", v, a);
            std::memcpy(&o2, w, 8);
            {   // the step's nan / exchange-timeout flag: the largest over every dim's record (a
                // peer-exchange block that gave the step up flags its own dim: any dim counts)
                float nf;
                std::memcpy(&nf, &w[2], 4);
                float& st3 = e->rec_stats[(size_t)v * 4 + 3];
                st3 = (a == 0 || nf > st3 || std::isnan(nf)) ? nf : st3;
            }
            double* ov = e->rec_out.data() + (size_t)v * od;
            if (model == MPPI_MODEL_QUADROTOR || (model == MPPI_MODEL_AERIAL && a < 4)) continue;   // (host-formed)
            if (model == MPPI_MODEL_DRONE || (model == MPPI_MODEL_WHOLEBODY && a < 3)) {
                ov[a] = o1; ov[3 + a] = o2;
            } else {
                const int base = (model == MPPI_MODEL_WHOLEBODY) ? 6 : (model == MPPI_MODEL_AERIAL) ? 12 : 0, j = a - qoff;
                ov[base + j] = o1; ov[base + nq + j] = o2;
            }
        }
        if (!load_record(e, r0 + 2 * A, want, w)) return fail(MPPI_ERR_STATE, "stats record %d not tagged", v);
        std::memcpy(&e->rec_stats[(size_t)v * 4], w, 12);
    }
    return MPPI_OK;
}

mppi_status mppi_read_outputs(mppi_engine* e, double* out, float* u0, mppi_stats* stats) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    switch (e->pending) {
    case Pending::None: return fail(MPPI_ERR_STATE, "no finalised step to read");
    case Pending::Call: HIP_TRY(hipSetDevice(e->cfg.device)); break;   // (its flags, not the queue's drain)
    case Pending::Hip:
    case Pending::Batch: if (use_device(e)) return MPPI_ERR_HIP;
    }
    {   mppi_status st = wait_outputs(e);
        if (st != MPPI_OK) return st; }
    if (e->d_stamps) {   // diagnostic: average phase cycles over all waves, all finalize blocks
        mppi_status st = add_stamps(e->d_stamps, (size_t)e->V * e->dp.nb * (e->threads / 64), kRollStampOrder, e->stamp_sum, e->stamp_n);
        if (st == MPPI_OK) st = add_stamps(e->d_fstamps, (size_t)e->V * e->A * e->fin_ts, kFinStampOrder, e->fstamp_sum, e->fstamp_n);
        if (st != MPPI_OK) return st;
    }
    const double* o = (const double*)e->h_out;
    const float* uu = (const float*)(e->h_out + off_u0(e));
    const float* st = (const float*)(e->h_out + off_stats(e));
    if (e->pending != Pending::Batch && e->out_seq != 0u) {   // a read step: its values from its tagged records
        mppi_status rs = assemble_records(e);
        if (rs != MPPI_OK) return rs;
        o = e->rec_out.data();
        uu = e->rec_u0.data();
        st = e->rec_stats.data();
    }
    // A bounded engine hands out u0 clamped on its rotor dims (u_prev stays the raw warm start: SavGol's negative
    // taps can carry row 0 past a bound), and the base's outputs below are formed from that clamped u0.  The
    // stats' finiteness check further down reads the raw row.
    const float* uo = uu;
    if (e->has_limits) {
        e->lim_u0.assign(uu, uu + (size_t)e->V * e->A);
        for (int v = 0; v < e->V; ++v)
            for (int a = 0; a < kLimitsN; ++a) {
                float& x = e->lim_u0[(size_t)v * e->A + a];
                x = x < e->limits.lo[a] ? e->limits.lo[a] : x > e->limits.hi[a] ? e->limits.hi[a] : x;   // (a NaN stays)
            }
        uo = e->lim_u0.data();
    }
    if (out) std::memcpy(out, o, sizeof(double) * e->V * e->out_dim);
    if (out && e->cfg.model == MPPI_MODEL_QUADROTOR)
        for (int v = 0; v < e->V; ++v)
            quad_outputs(e, e->state.data() + (size_t)v * e->state_dim, uo + (size_t)v * e->A, out + (size_t)v * e->out_dim);
    if (out && e->cfg.model == MPPI_MODEL_AERIAL)
        for (int v = 0; v < e->V; ++v)
            aerial_outputs(e, e->state.data() + (size_t)v * e->state_dim, uo + (size_t)v * e->A, out + (size_t)v * e->out_dim);
    if (u0) std::memcpy(u0, uo, sizeof(float) * e->V * e->A);
    bool nonfinite = false;
    for (int v = 0; v < e->V; ++v) {
        int reach = 0;
        if (e->cfg.check_reach && e->cfg.model == MPPI_MODEL_ARM) {   // mppi.py:95-120 (host FK)
            const double* s = e->state.data() + (size_t)v * e->state_dim;
            const double* qdes = o + (size_t)v * e->out_dim;
            float T16[16];
            host_fk_c(e->cfg.joints, e->cfg.n_joints, e->fk_O.data(), e->fk_ax.data(), qdes, s, e->cfg.state_f64 != 0,
                      T16);
            // (a tracking engine: row 0 of the vehicle's table, the pose wanted one step ahead, where qdes is)
            const float* tp = e->d_ttab ? &e->h_ttab[(size_t)v * e->H * 12] : &e->tpos[3 * v];
            const float err = std::fabs(T16[3] - tp[0]) + std::fabs(T16[7] - tp[1]) + std::fabs(T16[11] - tp[2]);
            reach = err < e->cfg.reach_tol;
        }
        // 2: a peer-exchange step given up (a rank's timeout: u_prev kept) -- this step's flag or
        // any step's since the exchange was last reset (the sticky word: every block, every step)
        const int nf = (st[4 * v + 3] >= 2.0f || (e->peer && sticky_timeout(e) != 0u)) ? 2
                       : ((st[4 * v + 3] > 0.0f) || !std::isfinite(st[4 * v]) || !std::isfinite(uu[(size_t)v * e->A]));
        nonfinite |= nf;
        if (stats) {
            stats[v].rho = st[4 * v];
            stats[v].eta = st[4 * v + 1];
            stats[v].ess = st[4 * v + 2];
            stats[v].nonfinite = nf;
            stats[v].reach = reach;
            stats[v]._pad = 0;
        }
    }
    (void)nonfinite;   // the reference propagates NaN silently; callers read stats.nonfinite
    return MPPI_OK;
}

static mppi_status control_call_aql(mppi_engine* e, const double* state, bool* used);

mppi_status mppi_step(mppi_engine* e, const double* state, const float* h_noise, double* out, float* u0,
                      mppi_stats* stats) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    note_call(e);
    if (sharded(e) && !e->comm)
        return fail(MPPI_ERR_STATE, "mppi_step on a shard needs mppi_comm_init (or use the split phases)");
    mppi_status st;
    if (e->cfg.noise_mode == MPPI_NOISE_PHILOX && e->V == 1 && !sharded(e)) {   // one vehicle: native packets
        bool used = false;
        static mppi_aql::PhaseClock pc{"[mppi aql] per call (us):", {"before the doorbell", "flag wait", "outputs + check_reach"}, 3, 1000};
        pc.start();
        if ((st = control_call_aql(e, state, &used)) != MPPI_OK) return st;
        e->calls_native = used;
        e->pw_native.store(used, std::memory_order_release);
        if (used) {
            pc.mark();
            st = mppi_read_outputs(e, out, u0, stats);
            pc.mark_split(e->call_wait_us);
            pc.done();
            return st;
        }
    }
    e->calls_native = false;
    e->pw_native.store(false, std::memory_order_relaxed);   // (HIP launches: nothing to prewarm)
    if (state && (st = mppi_set_state(e, state)) != MPPI_OK) return st;
    const float* dn = nullptr;
    if (e->cfg.noise_mode == MPPI_NOISE_INJECTED) {
        if (!h_noise) return fail(MPPI_ERR_INVALID_ARG, "INJECTED noise mode needs noise");
        const size_t n = (size_t)e->V * e->K * e->H * e->A;
        if (use_device(e)) return MPPI_ERR_HIP;
        if (!e->d_noise_in) HIP_TRY(hipMalloc(&e->d_noise_in, n * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(e->d_noise_in, h_noise, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
        dn = e->d_noise_in;
    }
    if ((st = mppi_rollout(e, dn)) != MPPI_OK) return st;
    if (e->comm && (st = mppi_exchange(e)) != MPPI_OK) return st;
    if ((st = mppi_finalize(e)) != MPPI_OK) return st;
    if (!e->kern_call_hip || e->kern_call_peer != e->peer) {   // (mppi_kernel_info; described once)
        e->kern_call = kernels_text(roll_symbol(rollout_params(e, StepPath::Hip, dn, false), e->threads, nullptr, e->d_ttab, e->d_scene, e->d_field, e->self_members, e->d_limits),
                                    fin_symbol(finalize_params(e, FinKind::Final)), nullptr);
        e->kern_call_hip = true;
        e->kern_call_peer = e->peer;
    }
    return mppi_read_outputs(e, out, u0, stats);
}

// the engine's native queue, created on first use; false when native dispatch is off for it
static bool aql_ready(mppi_engine* e) {
    if (e->aql_off) return false;
    if (!e->aql && !e->aql_tried) {
        e->aql_tried = true;
        std::string why;
        if (hipSetDevice(e->cfg.device) == hipSuccess) e->aql = mppi_aql::step_create(e->cfg.device, &why);
        else why = "hipSetDevice failed";
        if (!e->aql) e->aql_why = why;
    }
    if (!e->aql) e->aql_off = true;
    return e->aql != nullptr;
}

// Native dispatch is unavailable for this step (why: recorded in aql_why; null: as aql_ready left
// it; off: and for every later one): an error in aql mode, and in auto mode MPPI_OK, on which the
// caller runs the step through HIP.
static mppi_status aql_unavailable(mppi_engine* e, const char* why, bool off) {
    if (why) e->aql_why = why;
    if (off) e->aql_off = true;
    return e->aql_mode == 1 ? fail(MPPI_ERR_STATE, "native dispatch: %s", e->aql_why.c_str()) : MPPI_OK;
}

// HIP work still queued on the engine's stream (uploads, an earlier HIP-path step) goes first: native
// packets are not ordered with it (0.1 us when there is none)
static mppi_status drain_stream(mppi_engine* e) {
    const hipError_t q = hipStreamQuery(e->stream);
    if (q == hipErrorNotReady) HIP_TRY(hipStreamSynchronize(e->stream));
    else if (q != hipSuccess) return fail(MPPI_ERR_HIP, "engine stream: %s", hipGetErrorString(q));
    return MPPI_OK;
}

// n steps as native AQL packets (mppi_aql.cpp).  *used = false: the caller runs them through
// HIP (auto mode, native dispatch unavailable for this engine; e->aql_why says why).
static mppi_status run_steps_aql(mppi_engine* e, int32_t n, bool* used) {
    *used = false;
    if (const char* why = aql_ineligible(e, true)) { e->aql_why = why; return MPPI_OK; }
    if (!aql_ready(e)) return aql_unavailable(e, nullptr, false);
    HIP_TRY(hipSetDevice(e->cfg.device));
    static mppi_aql::PhaseClock pc{"[mppi aql] per batch (us):", {"stream query", "capture", "prepare", "packets"}, 4, 200};
    pc.start();
    mppi_status st = drain_stream(e);
    if (st != MPPI_OK) return st;
    pc.mark();
    // the two launches exactly as the HIP path makes them, described instead of launched (and the
    // descriptions reused while nothing in them changed); every step's but the last are the quiet ones
    const bool ovl = e->overlap && n > 1;   // (experiment, MPPI_OVERLAP=1)
    const auto roll_params = [&](bool quiet) {
        DevParams p = rollout_params(e, StepPath::Batch, nullptr, quiet);
        if (ovl) p.noise_mode |= kNoiseOverlap;
        return p;
    };
    DescCache& c = e->batch;
    {   const DevParams p = roll_params(false);
        const FinParams f = finalize_params(e, FinKind::Final, StepPath::Batch);
        if (!c.matches(p, f, e->threads, false)) {
            e->kern_batch_state = 0;
            const DevParams pq = roll_params(true);
            const FinParams fq = finalize_params(e, FinKind::Final, StepPath::Batch, true);
            if (const int rc = c.refresh(p, f, e->threads, &pq, &fq))
                return fail(MPPI_ERR_HIP, "describing the step's launches failed (%d)", rc);
        } }
    std::string err;
    pc.mark();
    const auto guard = mppi_aql::step_guard(e->aql);   // (no prewarm touch between prepare and dispatch)
    const int pr = mppi_aql::step_prepare(e->aql, c.roll, c.roll_quiet, c.fin, c.fin_quiet, e->step_ctr, kRollStepOff, &err);
    pc.mark();
    // not dispatchable natively (a kernel the code objects lack, hidden arguments)
    if (pr == -2) return aql_unavailable(e, err.c_str(), true);
    if (pr == 0 && ovl) {   // every finalize block's counter at the batch's first step (queue drained:
                            // step_prepare above waited for it or found it idle)
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)e->d_ovl, (int)e->step_ctr, (size_t)e->V * e->A * e->fin_ts,
                                  e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    if (pr != 0 || mppi_aql::step_dispatch(e->aql, n, &err, ovl) != 0)
        return fail(MPPI_ERR_HIP, "native dispatch: %s", err.c_str());
    pc.mark();
    pc.done();
    e->step_ctr += (uint32_t)n;
    e->pending = Pending::Batch;
    e->aql_why.clear();
    if (e->kern_batch_state != (n > 1 ? 2 : 1)) {   // (mppi_kernel_info; a one-step batch runs no quiet kernels)
        const std::string q = n > 1 ? c.fin_quiet.symbol : c.fin.symbol, rq = n > 1 ? c.roll_quiet.symbol : c.roll.symbol;
        e->kern_batch = kernels_text(c.roll.symbol, c.fin.symbol, &q, &rq);
        e->kern_batch_state = n > 1 ? 2 : 1;
    }
    *used = true;
    return MPPI_OK;
}

// One control call (V == 1) as a native (rollout, finalize) pair: the state goes into the
// rollout's arguments in pinned host memory (its vehicle constants), the finalize's arguments
// stay resident, and the call's completion flags carry a bit-31 sequence number the host
// wrote next to the constants (mppi_aql.h step_call).  *used = false: the HIP path runs it.
static mppi_status control_call_aql(mppi_engine* e, const double* state, bool* used) {
    *used = false;
    if (aql_ineligible(e) || e->event_wait) return MPPI_OK;
    if (!aql_ready(e)) return aql_unavailable(e, nullptr, false);
    static mppi_aql::PhaseClock pc{"[mppi aql] call setup (us):", {"hipSetDevice", "vehicle constants", "stream query", "capture"}, 4, 1000};
    pc.start();
    HIP_TRY(hipSetDevice(e->cfg.device));
    pc.mark();
    mppi_status st;
    if (state) {   // mppi_set_state's work for one vehicle: host-side constants only
        std::memcpy(e->state.data(), state, sizeof(double) * e->state.size());
        e->state_set = true;
        if ((st = build_vehicle_consts(e)) != MPPI_OK) return st;
    }
    if (!e->state_set) return fail(MPPI_ERR_STATE, "mppi_step before mppi_set_state");
    pc.mark();
    if ((st = drain_stream(e)) != MPPI_OK) return st;
    pc.mark();
    // The launch descriptions of the previous call are reused when only the state changed: the
    // state lives in the vehicle constants (DevParams::vc0, inside the rollout's last argument),
    // which are patched in; anything else that differs re-captures.
    DescCache& c = e->call;
    bool hit;
    {   const DevParams p = rollout_params(e, StepPath::Call, nullptr, false);
        const FinParams f = finalize_params(e, FinKind::Final, StepPath::Call);
        hit = c.matches(p, f, e->threads, true);
        if (hit) std::memcpy(c.roll.args + roll_vc0_off(c.roll), &p.vc0, sizeof(VehicleConst));
        else if (const int rc = c.refresh(p, f, e->threads))
            return fail(MPPI_ERR_HIP, "describing the step's launches failed (%d)", rc);
    }
    pc.mark();
    pc.done();
    std::string err;
    uint32_t seq = 0;
    const int pr = mppi_aql::step_call(e->aql, c.roll, c.fin, e->step_ctr, kRollStepOff, roll_seq_off(c.roll), &seq, &err);
    if (pr == -2) return aql_unavailable(e, err.c_str(), true);
    if (pr != 0) return fail(MPPI_ERR_HIP, "native dispatch: %s", err.c_str());
    ++e->step_ctr;
    e->out_seq = seq;
    e->pending = Pending::Call;
    if (!hit || e->kern_call_hip) e->kern_call = kernels_text(c.roll.symbol, c.fin.symbol, nullptr);
    e->kern_call_hip = false;
    *used = true;
    return MPPI_OK;
}

mppi_status mppi_run_steps(mppi_engine* e, int32_t n) {
    if (!e || n < 0) return fail(MPPI_ERR_INVALID_ARG, "mppi_run_steps: bad arguments");
    if (sharded(e) && !e->comm) return fail(MPPI_ERR_STATE, "mppi_run_steps on a shard needs mppi_comm_init");
    if (e->cfg.noise_mode != MPPI_NOISE_PHILOX) return fail(MPPI_ERR_STATE, "mppi_run_steps needs device noise");
    if (!e->state_set) return fail(MPPI_ERR_STATE, "mppi_run_steps before mppi_set_state");
    if (n == 0) return MPPI_OK;
    bool used = false;
    mppi_status st = run_steps_aql(e, n, &used);
    if (st != MPPI_OK || used) return st;
    for (int i = 0; i < n; ++i) {
        mppi_status st = rollout_impl(e, nullptr, i < n - 1);
        if (st != MPPI_OK) return st;
        if (e->comm && (st = mppi_exchange(e)) != MPPI_OK) return st;
        if ((st = finalize_impl(e, i == n - 1, true)) != MPPI_OK) return st;
    }
    {   // (mppi_kernel_info) the launches above, described
        const auto roll = [&](bool quiet) { return roll_symbol(rollout_params(e, StepPath::Hip, nullptr, quiet), e->threads, nullptr, e->d_ttab, e->d_scene, e->d_field, e->self_members, e->d_limits); };
        const auto fin = [&](bool quiet) { return fin_symbol(finalize_params(e, FinKind::Final, StepPath::Hip, quiet)); };
        const std::string q = fin(n > 1), rq = roll(n > 1);
        e->kern_batch = kernels_text(roll(false), fin(false), &q, &rq);
        e->kern_batch_state = 0;
    }
    return MPPI_OK;
}

// The kernels the last mppi_run_steps and the last mppi_step ran: for each, the rollout's and the
// finalize's symbols (the instantiations' Itanium names, as the code objects hold them), and for a
// batch the quiet finalize of its steps before the last ("none": every step ran the full one).
// A batch also names the quiet rollout of those steps, likewise.
// "; MPPI_GENERIC_KERNELS" at the end when the engine was created with that switch.
mppi_status mppi_kernel_info(mppi_engine* e, char* buf, int32_t len) {
    if (!e || !buf || len <= 0) return fail(MPPI_ERR_INVALID_ARG, "mppi_kernel_info: bad arguments");
    snprintf(buf, (size_t)len, "batch: %s; call: %s%s", e->kern_batch.c_str(), e->kern_call.c_str(),
             e->generic == kGenericAll ? "; MPPI_GENERIC_KERNELS" : e->generic ? "; MPPI_GENERIC_KERNELS (in part)" : "");
    return MPPI_OK;
}

mppi_status mppi_dispatch_info(mppi_engine* e, char* buf, int32_t len) {
    if (!e || !buf || len <= 0) return fail(MPPI_ERR_INVALID_ARG, "mppi_dispatch_info: bad arguments");
    snprintf(buf, (size_t)len, "%s%s; calls: %s%s%s", e->aql_why.empty() ? "aql" : "hip: ", e->aql_why.c_str(),
             e->calls_native ? "aql (arguments in " : "hip", e->calls_native ? mppi_aql::step_call_memory(e->aql) : "",
             e->calls_native ? ")" : "");
    return MPPI_OK;
}


mppi_status mppi_synchronize(mppi_engine* e) {
    if (!e) return fail(MPPI_ERR_INVALID_ARG, "null engine");
    if (use_device(e)) return MPPI_ERR_HIP;
    // The last finalised step's completion flag is polled first (mapped host memory, a
    // few hundred ns behind the kernel); hipStreamSynchronize alone wakes the host
    // microseconds after the stream drains, which a short timed batch pays in full.
    switch (e->pending) {
    case Pending::Hip:
    case Pending::Call:
        if (!e->event_wait) {
            mppi_status st = wait_outputs(e);
            if (st != MPPI_OK) return st;
        }
        break;
    case Pending::None:
    case Pending::Batch: break;   // (a batch: use_device above has joined it)
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->peer)
        if (const uint32_t t = sticky_timeout(e))
            return fail(MPPI_ERR_PEER_TIMEOUT, "peer exchange: a step was given up (tag %08x): this rank's "
                                               "warm start may differ from its peers' until mppi_peer_reset", t);
    return MPPI_OK;
}


}  // extern "C"
