// mppi_elites.h -- what the elite readback's kernels (mppi_elites.hip), its host entry point
// (mppi_get_elites, mppi_engine.cpp) and the host twin of its order (mppi_debug_elite_order) share:
// the sort key, the launch parameters and the launchers.  Internal: not part of the public ABI.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPPI_ELITE_HD __host__ __device__
#else
#define MPPI_ELITE_HD
#endif

namespace mppi {

// The order of the elites is ascending in this key, and keys of different samples differ: the high
// word orders the costs (-0 as +0, +inf after every finite cost, every NaN after +inf, whatever its
// sign and payload), the low word is the sample index, so equal costs go by the lower index first:
// np.argsort(S, kind="stable").  Bits only -- no arithmetic a device could round or flush.
MPPI_ELITE_HD inline uint32_t elite_cost_word(uint32_t bits) {
    if ((bits & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;   // NaN
    if (bits == 0x80000000u) bits = 0u;                           // -0
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
MPPI_ELITE_HD inline unsigned long long elite_key(uint32_t cost_bits, uint32_t k) {
    return ((unsigned long long)elite_cost_word(cost_bits) << 32) | k;
}
// What a lane past K and an unused candidate slot carry: after every key of a sample (k < 2^31).
constexpr unsigned long long kEliteSentinel = ~0ull;

constexpr int kEliteMax = 64;           // MPPI_MAX_ELITES
constexpr int kEliteThreads = 256;      // threads of a selection block
constexpr int kEliteShare = 4096;       // S_A: the samples of one stage-A block while K <= kEliteShare * kEliteMaxBlocks
constexpr int kEliteMaxBlocks = 256;    // stage-A blocks per vehicle at most (beyond, the shares grow)

// stage-A blocks per vehicle and the samples of each (the last block's share may be shorter)
inline void elite_split(int64_t K, int* blocks, int64_t* share) {
    int64_t b = (K + kEliteShare - 1) / kEliteShare;
    if (b > kEliteMaxBlocks) b = kEliteMaxBlocks;
    if (b < 1) b = 1;
    *blocks = (int)b;
    *share = (K + b - 1) / b;
}

struct EliteParams {
    const float* S;            // (V,K) the last rollout's costs
    const float* stats;        // (V,4) rho, eta, ... (FinParams::stats, as k_weights reads them)
    const float* planes;       // the trajectory planes (null: no rows)
    unsigned long long* cand;  // (V,B,n) stage A's candidates
    int32_t* idx;              // outputs: (V,n) sample indices, best first
    float* So;                 //          (V,n) their costs
    float* w;                  //          (V,n) their weights
    float* rows;               //          (V,n,H,Cr) their rollouts (null: none)
    int32_t V, K, H, n;
    int32_t C, nstate, has_ee, Cr;   // planes per vehicle; state channels; EE rows follow; floats per row
    int32_t pitch, t_major;          // mppi_layout.h traj_pitch; (C,H,Kp) planes (k_rollout_quad)
    float coef;
};

}  // namespace mppi

extern "C" {
// One launch of the readback: stage 0 the per-share selection (skipped when one block holds K),
// 1 the final selection, sort and idx / S / w, 2 the gather of the rows (skipped without rows).
// 0 launched (or described into the capture target), 1 skipped, -1 no kernel for these shapes,
// > 0 a HIP error.
int mppi_launch_elites_stage(const mppi::EliteParams* p, int stage, void* stream);
// All of them, in order.
int mppi_launch_elites(const mppi::EliteParams* p, void* stream);
}
