// sload_latency.hip -- warm scalar-load latency on gfx950 (tools/, not shipped).
//
//   hipcc --offload-arch=gfx950 -O3 -o tools/_bin/sload_latency tools/sload_latency.hip && tools/_bin/sload_latency
//
// One wave walks a chain of dependent s_load_dword through a 1 KiB block (16 lines of 64 B, the size
// of a rollout's kernel-argument segment): word 0 of each line holds the byte offset of the next line,
// so every load waits for the one before it, as a kernel-argument read waited for at its use does.
// Per trial, s_memtime (shader clock) around
//   empty   the timing pair alone,
//   l2      the chain after the block was read with VECTOR loads only (lines in L2, not in the scalar cache),
//   warm    the same chain again (lines in the scalar cache),
//   long    64 rounds of the warm chain, with s_memrealtime (100 MHz) around it for the clock ratio.
// Prints the median cycles per load of each and the shader clock the ratio implies.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

constexpr int kLines = 16, kTrials = 64, kLong = 64;

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));              \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

__device__ __forceinline__ uint32_t chain(const uint32_t* blk, uint32_t off) {
#pragma unroll
    for (int i = 0; i < kLines; ++i)
        asm volatile("s_load_dword %0, %1, %0\n\ts_waitcnt lgkmcnt(0)" : "+s"(off) : "s"(blk) : "memory");
    return off;
}

// blk: kTrials blocks of 1 KiB, one per trial (a fresh block is in neither cache level of this CU's
// scalar cache); out: kTrials x 8 counters
__global__ void __launch_bounds__(64) k_sload(const uint32_t* blk_all, unsigned long long* out, uint32_t* sink) {
    uint32_t acc = 0;
    for (int tr = 0; tr < kTrials; ++tr) {
        const uint32_t* blk = blk_all + tr * (kLines * 16);
        // vector loads of every line: L2 (and the vector L1), not the scalar cache
        const uint32_t vw = *(const volatile uint32_t*)(blk + (threadIdx.x & (kLines - 1)) * 16);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        acc += vw;
        const unsigned long long t0 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        uint32_t off = chain(blk, 0u);
        const unsigned long long t2 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        off = chain(blk, off);
        const unsigned long long t3 = __builtin_amdgcn_s_memtime();
        const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int r = 0; r < kLong; ++r) off = chain(blk, off);
        const unsigned long long t4 = __builtin_amdgcn_s_memtime();
        const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        acc += off;
        if (threadIdx.x == 0) {
            unsigned long long* o = out + tr * 8;
            o[0] = t1 - t0; o[1] = t2 - t1; o[2] = t3 - t2; o[3] = t4 - t3; o[4] = r1 - r0;
        }
    }
    if (threadIdx.x == 0) *sink = acc;
}

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main() {
    std::vector<uint32_t> h(kTrials * kLines * 16, 0u);
    for (int tr = 0; tr < kTrials; ++tr)
        for (int i = 0; i < kLines; ++i) h[(tr * kLines + i) * 16] = (uint32_t)(((i + 1) % kLines) * 64);   // next line, bytes
    uint32_t *d_blk = nullptr, *d_sink = nullptr;
    unsigned long long* d_out = nullptr;
    CHECK(hipMalloc(&d_blk, h.size() * 4));
    CHECK(hipMalloc(&d_out, kTrials * 8 * sizeof(unsigned long long)));
    CHECK(hipMalloc(&d_sink, 4));
    CHECK(hipMemcpy(d_blk, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    std::vector<unsigned long long> o(kTrials * 8);
    for (int pass = 0; pass < 2; ++pass) {   // (pass 0: code and clocks warm up; pass 1 is reported)
        hipLaunchKernelGGL(k_sload, dim3(1), dim3(64), 0, 0, d_blk, d_out, d_sink);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(o.data(), d_out, o.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    std::vector<double> e, l2, w, lg, mhz;
    for (int tr = 1; tr < kTrials; ++tr) {   // (trial 0 also fetches the loop's code)
        const unsigned long long* p = &o[tr * 8];
        e.push_back((double)p[0]);
        l2.push_back(((double)p[1] - (double)p[0]) / kLines);
        w.push_back(((double)p[2] - (double)p[0]) / kLines);
        lg.push_back((double)p[3] / (kLong * kLines));
        mhz.push_back((double)p[3] / (double)p[4] * 100.0);
    }
    // (pass 1 re-reads blocks pass 0 left in L2; the scalar cache is invalidated between kernels)
    std::printf("s_memtime pair %.0f cycles; dependent s_load_dword, cycles per load (median of %d trials):\n"
                "  after vector loads only (L2 hit) %.1f\n  second pass (scalar cache hit)   %.1f\n"
                "  %d more rounds                   %.1f\n  s_memtime ticks at %.0f MHz by s_memrealtime\n",
                median(e), kTrials - 1, median(l2), median(w), kLong, median(lg), median(mhz));
    CHECK(hipFree(d_blk));
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_sink));
    return 0;
}
