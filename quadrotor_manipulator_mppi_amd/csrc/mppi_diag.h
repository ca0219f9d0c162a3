// mppi_diag.h -- the rollout kernels' diagnostic macros: the timing knockouts (MPPI_KO) and the phase
// stamps and listing sections of the diagnostic builds.  All compiled out of the production build.
// (STAMP / STAMPW / STAMPRT expand inside rollout_body and use its locals.)
#pragma once

// Timing knockouts for tools/ experiments only (MPPI_HIPCC_EXTRA=-DMPPI_KO=n; results are
// wrong in such a build): 1 drops the integrator scans, 2 the Philox draw, 4 the FK chain,
// 8 the pose cost, 16 the trajectory stores, 32 Box-Muller, 64 the block record body,
// 128 the u_prev loads (H*A <= 4 * block threads), 256 the prologue's block barrier (LDS
// staging read unsynchronised), 512 the end-of-wave store drain (the hand-off unordered),
// 1024 the cost vector S (its LDS staging and store runs), 2048 block 0's vehicle-constant
// hand-off (16 + 1024 + 2048 on every launch: the upper bound of the quiet rollout).
#ifndef MPPI_KO
#define MPPI_KO 0
#endif

// Diagnostic phase stamps (build with -DMPPI_STAMPS; see tools/stamps.md):
// s_memtime per wave between scheduling barriers.  Compiled out otherwise.
#if defined(MPPI_STAMPS) && !defined(MPPI_TIMELINE)
#define STAMP(i)                                                                                      \
    do {                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                            \
        if (pk.stamps && lane == 0) {                                                                 \
            const size_t w_ = ((size_t)blockIdx.y * p.nb + blockIdx.x) * nw + wid;        \
            pk.stamps[w_ * kStamps + (i)] = __builtin_amdgcn_s_memtime();                             \
        }                                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                            \
    } while (0)
// STAMPW first drains this wave's outstanding memory operations, so the stamp
// after a load phase measures its latency (diagnostic builds perturb overlap).
#define STAMPW(i)                                                                  \
    do {                                                                           \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                \
        STAMP(i);                                                                  \
    } while (0)
// STAMPRT: the 100 MHz real-time counter (s_memrealtime), slots 13/14 = wave start/end:
// wall-clock wave lifetimes, the shader clock (memtime / realtime) and the grid's timeline
#define STAMPRT(i)                                                                                    \
    do {                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                            \
        if (pk.stamps && lane == 0) {                                                                 \
            const size_t w_ = ((size_t)blockIdx.y * p.nb + blockIdx.x) * nw + wid;        \
            pk.stamps[w_ * kStamps + (i)] = __builtin_amdgcn_s_memrealtime();                         \
            if ((i) == 13) /* where the wave ran: XCC_ID (hwreg 20) << 32 | HW_ID (hwreg 4) */        \
                pk.stamps[w_ * kStamps + 15] = ((unsigned long long)__builtin_amdgcn_s_getreg(0xF814) << 32) | \
                                               (unsigned)__builtin_amdgcn_s_getreg(0xF804);           \
        }                                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                            \
    } while (0)
#elif defined(MPPI_STAMPS)   // MPPI_TIMELINE: wall-clock time at wave start / end and at three phase
                             // boundaries (after the first group's Philox: slot 10, after the
                             // prologue's barrier: slot 1, after the rollout groups: slot 5), no
                             // waits: the kernel's own schedule; -DMPPI_TIMELINE_FINE=1 stamps every
                             // phase boundary (tools/probes.py timeline prints the per-phase medians)
#ifndef MPPI_TIMELINE_FINE
#define MPPI_TIMELINE_FINE 0
#endif
#define STAMP(i)                                                                                      \
    do {                                                                                              \
        if (((i) == 1 || (i) == 5 || (i) == 10 || MPPI_TIMELINE_FINE) && pk.stamps && lane == 0) {    \
            const size_t w_ = ((size_t)blockIdx.y * p.nb + blockIdx.x) * nw + wid;        \
            pk.stamps[w_ * kStamps + (i)] = __builtin_amdgcn_s_memrealtime();                         \
        }                                                                                             \
    } while (0)
#define STAMPW(i) STAMP(i)
#define STAMPRT(i)                                                                                    \
    do {                                                                                              \
        if (pk.stamps && lane == 0) {                                                                 \
            const size_t w_ = ((size_t)blockIdx.y * p.nb + blockIdx.x) * nw + wid;        \
            pk.stamps[w_ * kStamps + (i)] = __builtin_amdgcn_s_memrealtime();                         \
            if ((i) == 13)                                                                            \
                pk.stamps[w_ * kStamps + 15] = ((unsigned long long)__builtin_amdgcn_s_getreg(0xF814) << 32) | \
                                               (unsigned)__builtin_amdgcn_s_getreg(0xF804);           \
        }                                                                                             \
    } while (0)
#else
#define STAMP(i) do { } while (0)
#define STAMPW(i) do { } while (0)
#define STAMPRT(i) do { } while (0)
#endif

// Static instruction-mix sections (diagnostic builds, -DMPPI_SECTIONS; tools/isa_sections.py):
// a named comment in the listing with scheduling barriers on both sides, so no instruction moves
// across it.  Compiled out otherwise.
#ifdef MPPI_SECTIONS
#define SECTION(name)                                        \
    do {                                                     \
        __builtin_amdgcn_sched_barrier(0);                   \
        asm volatile("; MPPI_SECTION " name ::: "memory");   \
        __builtin_amdgcn_sched_barrier(0);                   \
    } while (0)
#else
#define SECTION(name) do { } while (0)
#endif
