// mppi_stores.h -- the rollout kernels' global stores: trajectory planes through a buffer resource, the
// write-through record stores, and the end-of-wave drain.
#pragma once
#include "mppi_device.h"
#include "mppi_diag.h"

// Trajectory stores (every wave store instruction writes 256 contiguous bytes).  The
// planes of one vehicle are one buffer resource (C*K*H*4 < 4 GiB, checked at create):
// the lane's byte offset sits in one VGPR and the plane offset in an SGPR, so a store
// costs no 64-bit address arithmetic (a v_lshl_add_u64 per store with flat addresses).
// kTrajAux is the stores' cache-policy field: sc1 (device scope: written through
// the XCD's L2) | nt (streaming).  With plain stores (0) the L2s hold up to 8 x 4 MB of
// dirty trajectory lines when the waves finish, and the kernel-end release writes them
// back serially: same-box A/B (profiles/r02/ab_store_policy.txt) whole-body K=8192 H=64
// rollout 16.4 -> 12.8 us, arm C3 7.1 -> 6.0 us, V=8 fleet 93.7 -> 81.2 us.
constexpr int kTrajAux = 18;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t traj_rsrc(float* planes_v, uint32_t plane_b, int C) {
    return __builtin_amdgcn_make_buffer_rsrc(planes_v, 0, (int)(plane_b * (uint32_t)C), 0x00020000);
}
__device__ __forceinline__ void traj_store(__amdgpu_buffer_rsrc_t rs, uint32_t voff, uint32_t soff, float x) {
    if (MPPI_KO & 16) return;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(x), rs, (int)voff, (int)soff, kTrajAux);
}
// Write-through stores for the record bodies the finalize reads (full 256 B t-runs): a raw
// buffer over a wave-uniform base, byte offsets < 4 GiB.  NOT for S: its one-lane 4 B
// stores become partial-line writes through to memory (whole-body K=8192 rollout
// 13.7 -> 19.0 us, profiles/r02/ab_store_policy.txt); in L2 they merge into full lines.
// Record bodies: sc1 (written through) without nt, so the lines stay allocated on their way
// to memory and the finalize's loads (other XCDs) come back sooner.  Order-balanced A/B vs
// sc1|nt (profiles/r02/ab_record_store_policy.txt): step pair arm C3 10.40 -> 10.08 us,
// whole-body K=8192 19.66 -> 18.96 us, quadrotor 12.25 -> 11.99 us.
constexpr int kRecAux = 16;
__device__ __forceinline__ void wt_store(float* base_uniform, uint32_t byte_off, float x) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base_uniform, 0, (int)0xFFFFFFFFu, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(x), rs, (int)byte_off, 0, kRecAux);
}
// the record header (rho, eta, eta2, nan) of one block, written through like the bodies
__device__ __forceinline__ void wt_store4(float* base_uniform, uint32_t byte_off, float4 x) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base_uniform, 0, (int)0xFFFFFFFFu, 0x00020000);
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = {__float_as_uint(x.x), __float_as_uint(x.y), __float_as_uint(x.z), __float_as_uint(x.w)};
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)byte_off, 0, kRecAux);
}
// The rollout's outputs the finalize reads (record bodies and headers, and the vehicle
// constants block 0 hands over) are written through at device scope; every wave waits for its
// stores before it ends.  So they are visible device-wide when the kernel completes, and the
// native dispatch's rollout packet needs no release fence (the end-of-kernel L2 writeback,
// ~0.8 us per step at C3; mppi_aql.cpp).
__device__ __forceinline__ void drain_stores() {
    if (!(MPPI_KO & 512)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
