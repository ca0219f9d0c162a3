// mppi_elites.hip -- the elite readback (mppi_get_elites): the n <= 64 lowest-cost samples of the
// last rollout of every vehicle, selected, sorted and gathered on the device.  Not part of the
// control step: it reads the costs (V,K), the finalize's rho and eta and the trajectory planes, and
// writes only its own buffers.
//
// Order: ascending in the 64-bit key of mppi_elites.h (cost word, sample index).  Keys of different
// samples differ, so "the n smallest" has an exact threshold T: the n-th smallest key.
//
// k_elite_select, one block of 256 threads over M keys (a share of the costs, or stage A's
// candidates), finds T by radix descent from the key's top byte: an LDS histogram of the byte among
// the keys that match the prefix so far, one wave's scan of it for the bin the rank falls in, and so
// on down the key -- stopping at the byte from which the whole bin is taken.  It then compacts the
// keys <= T.  A share of up to 4096 keys stays in registers (16 per thread) over the passes; a
// larger one (K beyond 2^20: the shares grow instead of the candidates) is read again each pass.
//   stage A   grid (B,V)   share b of vehicle v -> its n smallest keys into cand (V,B,n), padded
//                          with the sentinel where the share holds fewer than n samples
//   stage B   grid (1,V)   the n smallest of the B*n candidates; wave 0 sorts them (bitonic over
//                          __shfl_xor) and writes idx, S and w = expf(coef * (S - rho)) / eta,
//                          k_weights' expression
// With B = 1 stage B selects from the costs itself and stage A is not launched.
// k_elite_gather, grid (n,V): elite j's rollout out of the planes into rows (H,Cr), the layout of
// mppi_get_trajectory: the state channels, then (ARM, WHOLEBODY) the EE's twelve entries and 0 0 0 1.
//
// Bounds.  A key's low word is a sample index < K by construction; a sentinel (index word all ones)
// can be selected only if fewer than n samples exist, which the launcher refuses (n <= K).  Both
// writers of an index still compare it with K and the slot with 64 before they use either.
#include "mppi_device.h"
#include "mppi_elites.h"

namespace {

constexpr int kItems = kEliteShare / kEliteThreads;   // keys a thread keeps in registers
static_assert(kEliteThreads == 256, "one thread per histogram bin");
static_assert(kItems * kEliteThreads == kEliteShare, "a share fills the block's registers exactly");

struct EliteLds {
    uint32_t hist[256];
    unsigned long long sel[kEliteMax];
    unsigned long long prefix, thresh;
    uint32_t rem, cnt, done;
};

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long x, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, m, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), m, 64);
    return ((unsigned long long)hi << 32) | lo;
}

}  // namespace

// FROM_COSTS: the keys are made from this block's share of S; else they are stage A's candidates.
// FINAL: sort and write the outputs; else write the selected keys as candidates.
template <bool FROM_COSTS, bool FINAL>
__global__ __launch_bounds__(kEliteThreads) void k_elite_select(EliteParams p, int32_t B, int64_t share) {
    __shared__ EliteLds L;
    const int tid = threadIdx.x, v = blockIdx.y, n = p.n;
    const float* const Sv = p.S + (size_t)v * (size_t)p.K;
    // this block's keys: i in [0, M)
    const int64_t lo = FROM_COSTS ? (int64_t)blockIdx.x * share : 0;
    int64_t M = FROM_COSTS ? (int64_t)p.K - lo : (int64_t)B * n;
    if (FROM_COSTS && M > share) M = share;
    if (M < 0) M = 0;
    const unsigned long long* const cand = p.cand + (size_t)v * (size_t)B * (size_t)n;
    auto key_at = [&](int64_t i) -> unsigned long long {
        if constexpr (FROM_COSTS) return elite_key(__float_as_uint(Sv[lo + i]), (uint32_t)(lo + i));
        else return cand[i];
    };
    const bool cached = M <= (int64_t)kEliteShare;
    unsigned long long keys[kItems];
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        const int64_t i = tid + j * kEliteThreads;
        keys[j] = (cached && i < M) ? key_at(i) : kEliteSentinel;
    }
    auto for_each_key = [&](auto&& f) {
        if (cached) {
#pragma unroll
            for (int j = 0; j < kItems; ++j)
                if ((int64_t)(tid + j * kEliteThreads) < M) f(keys[j]);
        } else {
            for (int64_t i = tid; i < M; i += kEliteThreads) f(key_at(i));
        }
    };

    if (tid == 0) {
        L.prefix = 0ull; L.thresh = 0ull; L.cnt = 0u; L.done = 0u;
        L.rem = (uint32_t)(M < (int64_t)n ? M : (int64_t)n);   // (candidates: at least n of them are samples)
    }
    for (int pass = 7; pass >= 0; --pass) {
        const int shift = 8 * pass;
        L.hist[tid] = 0u;
        __syncthreads();
        if (L.done) break;   // (uniform)
        const unsigned long long pre = L.prefix;
        for_each_key([&](unsigned long long key) {
            const unsigned long long head = pass == 7 ? 0ull : key >> (shift + 8);
            // (one LDS add per key: folding a wave's adds to one bin into a single add measured no
            //  faster, profiles/r11/elites/README.txt)
            if (head == pre) atomicAdd(&L.hist[(uint32_t)(key >> shift) & 255u], 1u);
        });
        __syncthreads();
        if (tid < 64) {   // wave 0: lane l scans bins 4l .. 4l+3
            uint32_t c[4], s = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) { c[q] = L.hist[4 * tid + q]; s += c[q]; }
            uint32_t incl = s;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
                if (tid >= d) incl += t;
            }
            const uint32_t rem = L.rem, excl = incl - s;
            if (excl < rem && rem <= incl) {   // the rank falls in this lane's bins: one lane at most
                uint32_t r = rem - excl, digit = 0u, cd = 0u;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (cd == 0u) {
                        if (r <= c[q]) { digit = 4u * tid + q; cd = c[q]; }
                        else r -= c[q];
                    }
                }
                const unsigned long long np = (pre << 8) | digit;
                L.prefix = np;
                L.rem = r;
                if (r == cd) {   // the whole bin is taken: every key up to the bin's last
                    L.thresh = shift ? ((np << shift) | ((1ull << shift) - 1ull)) : np;
                    L.done = 1u;
                }
            }
        }
        __syncthreads();
    }
    const unsigned long long T = L.thresh;
    for_each_key([&](unsigned long long key) {
        if (key <= T) {
            const uint32_t slot = atomicAdd(&L.cnt, 1u);
            if (slot < (uint32_t)kEliteMax) L.sel[slot] = key;
        }
    });
    __syncthreads();
    const uint32_t got = L.cnt < (uint32_t)n ? L.cnt : (uint32_t)n;
    if constexpr (!FINAL) {
        if (tid < n)
            p.cand[((size_t)v * gridDim.x + blockIdx.x) * (size_t)n + tid] = (uint32_t)tid < got ? L.sel[tid] : kEliteSentinel;
    } else {
        if (tid >= 64) return;
        unsigned long long key = (uint32_t)tid < got ? L.sel[tid] : kEliteSentinel;
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                const unsigned long long other = shfl_xor_u64(key, j);
                const bool keep_min = ((tid & j) == 0) == ((tid & k) == 0);
                key = keep_min ? (other < key ? other : key) : (other > key ? other : key);
            }
        }
        if (tid < n) {
            const uint32_t k = (uint32_t)key;
            const size_t o = (size_t)v * n + tid;
            if (key != kEliteSentinel && k < (uint32_t)p.K) {
                const float s = Sv[k];
                const float rho = p.stats[v * 4], eta = p.stats[v * 4 + 1];
                p.idx[o] = (int32_t)k;
                p.So[o] = s;
                p.w[o] = expf(p.coef * (s - rho)) / eta;
            } else {   // (unreachable with n <= K)
                p.idx[o] = -1;
                p.So[o] = __uint_as_float(0x7FC00000u);
                p.w[o] = 0.0f;
            }
        }
    }
}

__global__ __launch_bounds__(kEliteThreads) void k_elite_gather(EliteParams p) {
    const int j = blockIdx.x, v = blockIdx.y;
    const uint32_t k = (uint32_t)p.idx[(size_t)v * p.n + j];
    if (k >= (uint32_t)p.K) return;
    const size_t pitch = (size_t)p.pitch;
    const size_t plane = p.t_major ? pitch * (size_t)p.H : (size_t)p.K * pitch;
    const float* const src = p.planes + (size_t)v * (size_t)p.C * plane;
    float* const dst = p.rows + ((size_t)v * p.n + j) * (size_t)p.H * (size_t)p.Cr;
    const int total = p.H * p.Cr;
    for (int i = threadIdx.x; i < total; i += kEliteThreads) {
        const int t = i / p.Cr, c = i - t * p.Cr;
        const size_t at = p.t_major ? (size_t)t * pitch + k : (size_t)k * pitch + (size_t)t;
        float x;
        if (c < p.nstate) x = src[(size_t)c * plane + at];
        else if (p.has_ee && c < p.nstate + 12) x = src[(size_t)c * plane + at];   // the EE planes follow the state's
        else x = (c == p.nstate + 15) ? 1.0f : 0.0f;
        dst[i] = x;
    }
}

extern "C" int mppi_launch_elites_stage(const EliteParams* p, int stage, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    if (!p || p->n < 1 || p->n > kEliteMax || p->K < 1 || p->n > p->K || p->V < 1 || p->V > 65535 || p->H < 1) return -1;
    int B;
    int64_t share;
    elite_split(p->K, &B, &share);
    const dim3 block(kEliteThreads);
    switch (stage) {
        case 0:
            if (B == 1) return 1;
            return go(k_elite_select<true, false>, dim3(B, p->V), block, 0, s, *p, (int32_t)B, share);
        case 1:
            if (B == 1) return go(k_elite_select<true, true>, dim3(1, p->V), block, 0, s, *p, (int32_t)1, (int64_t)p->K);
            return go(k_elite_select<false, true>, dim3(1, p->V), block, 0, s, *p, (int32_t)B, share);
        case 2:
            if (!p->rows) return 1;
            if (!p->planes || p->Cr < 1 || p->C < 1 || p->nstate < 1 || p->nstate > p->C || p->pitch < 1 ||
                (p->has_ee ? (p->C != p->nstate + 12 || p->Cr != p->nstate + 16) : p->Cr != p->nstate) ||
                (int64_t)p->H * p->Cr > 0x7FFFFFFF || p->pitch < (p->t_major ? p->K : p->H))
                return -1;
            return go(k_elite_gather, dim3(p->n, p->V), block, 0, s, *p);
    }
    return -1;
}

extern "C" int mppi_launch_elites(const EliteParams* p, void* stream) {
    for (int stage = 0; stage < 3; ++stage) {
        const int rc = mppi_launch_elites_stage(p, stage, stream);
        if (rc != 0 && rc != 1) return rc;
    }
    return 0;
}
