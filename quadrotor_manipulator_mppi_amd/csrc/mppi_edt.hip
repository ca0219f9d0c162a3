// mppi_edt.hip -- the occupancy grid's distance transform (mppi_set_occupancy): an exact, separable
// Euclidean transform in int32 squared index distances, from the occupancy bytes to the field buffer's
// x-pair cells.  Not part of the control step: HIP launches on the engine's stream, outside any batch.
//
// Both seed sets -- the occupied nodes and the free ones -- are carried together through one sweep per
// axis, in two grids (EdtParams::g_occ, g_free) that are transformed in place:
//   k_edt_x       one wave per x row, lane = x (nx > 64: node x = 64 c + lane of chunk c, up to 8 chunks).
//                 Per seed set a forward wave scan (max) of "index of the last seed at or before x" with
//                 the carry of the chunks before, and a backward one (min) of the first seed at or after;
//                 the squared distance to the nearer, kEdtInf where the row holds no seed of the set.
//   k_edt_axis    the y pass, then the z pass: out[i] = min_j (in[j] + (i - j)^2) along the axis.  Lines
//                 along y and z are strided in memory, so a block owns kEdtTile adjacent x columns of one
//                 z (one y) and stages their whole lines of both grids in LDS as [j][column]: every global
//                 access is a run of kEdtTile consecutive words, and the lanes of a wave read four
//                 consecutive LDS rows, 64 different banks.  Thread (column, slot) computes the outputs
//                 i = slot, slot + 16, ...: j walks outward from i and stops where (i - j)^2 reaches both
//                 running minima (no further j can lower either) or the cap's window (mppi_edt.h
//                 edt_window); the results are exact under both cuts.
//   k_edt_finish  one thread per node: the sign (occupied <=> D2_occ == 0), the root, the clamp
//                 (mppi_edt.h edt_value, the host's own inline) and the 8 B x-pair store
//                 (d[ix], d[min(ix + 1, nx - 1)]).
// The header of the field buffer is the host's small copy, queued behind these launches.
//
// Bounds.  Every index is formed from the block and thread ids and the dims of the parameters, which the
// launcher checks (2..512 per axis, at most 2^21 nodes); each is compared with its dim before use.  No
// value read from the occupancy or from a grid forms an address.
#include "mppi_device.h"
#include "mppi_edt.h"

namespace {

constexpr int kChunks = kEdtMaxLine / 64;    // 64-node chunks of the longest x row
constexpr int kSlots = kEdtThreads / kEdtTile;
constexpr int kNoneL = -(1 << 20), kNoneR = 1 << 20;   // "no seed on this side": any distance to it is >= 2^20 - 511

__device__ __forceinline__ int scan_max_up(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ int scan_min_down(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_down(v, d, 64);
        if (lane + d < 64) v = t < v ? t : v;
    }
    return v;
}
__device__ __forceinline__ int32_t sq_or_inf(int d) { return d < kEdtMaxLine ? d * d : kEdtInf; }

}  // namespace

__global__ __launch_bounds__(kEdtThreads) void k_edt_x(EdtParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)p.ny * p.nz;
    const int64_t row = (int64_t)blockIdx.x * (kEdtThreads / 64) + wave;
    if (row >= rows) return;   // (wave-uniform)
    const int nx = p.nx;
    const size_t base = (size_t)row * (size_t)nx;
    int left_o[kChunks], left_f[kChunks];
    bool occ[kChunks];
    int carry_o = kNoneL, carry_f = kNoneL;
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        left_o[c] = left_f[c] = kNoneL;
        occ[c] = false;
        if (c * 64 < nx) {   // (wave-uniform)
            const int x = c * 64 + lane;
            const bool in = x < nx;
            occ[c] = in && p.occ[base + (size_t)(in ? x : 0)] != 0;
            int vo = scan_max_up(in && occ[c] ? x : kNoneL, lane), vf = scan_max_up(in && !occ[c] ? x : kNoneL, lane);
            vo = vo > carry_o ? vo : carry_o;
            vf = vf > carry_f ? vf : carry_f;
            left_o[c] = vo; left_f[c] = vf;
            carry_o = __shfl(vo, 63, 64); carry_f = __shfl(vf, 63, 64);
        }
    }
    carry_o = carry_f = kNoneR;
#pragma unroll
    for (int c = kChunks - 1; c >= 0; --c) {
        if (c * 64 < nx) {
            const int x = c * 64 + lane;
            const bool in = x < nx;
            int vo = scan_min_down(in && occ[c] ? x : kNoneR, lane), vf = scan_min_down(in && !occ[c] ? x : kNoneR, lane);
            vo = vo < carry_o ? vo : carry_o;
            vf = vf < carry_f ? vf : carry_f;
            carry_o = __shfl(vo, 0, 64); carry_f = __shfl(vf, 0, 64);
            if (in) {
                const int dlo = x - left_o[c], dro = vo - x, dlf = x - left_f[c], drf = vf - x;
                p.g_occ[base + (size_t)x] = sq_or_inf(dlo < dro ? dlo : dro);
                p.g_free[base + (size_t)x] = sq_or_inf(dlf < drf ? dlf : drf);
            }
        }
    }
}

// n: the nodes of a line; line_stride: between its nodes; blockIdx.y picks the line's other coordinate,
// outer_stride apart (y pass: n = ny, nx, nx ny; z pass: n = nz, nx ny, nx).  LDS: 2 * n * kEdtTile words.
__global__ __launch_bounds__(kEdtThreads) void k_edt_axis(EdtParams p, int32_t n, int32_t line_stride, int32_t outer_stride) {
    extern __shared__ int32_t edt_lds[];
    int32_t* const A = edt_lds;
    int32_t* const B = edt_lds + n * kEdtTile;
    const int c = threadIdx.x % kEdtTile, slot = threadIdx.x / kEdtTile;
    const int x = blockIdx.x * kEdtTile + c;
    const bool in = x < p.nx;
    const size_t base = (size_t)blockIdx.y * (size_t)outer_stride + (size_t)(in ? x : 0);
    for (int i = slot; i < n; i += kSlots) {
        const size_t g = base + (size_t)i * (size_t)line_stride;
        A[i * kEdtTile + c] = in ? p.g_occ[g] : kEdtInf;
        B[i * kEdtTile + c] = in ? p.g_free[g] : kEdtInf;
    }
    __syncthreads();
    if (!in) return;
    const int reach = p.window < n - 1 ? p.window : n - 1;
    for (int i = slot; i < n; i += kSlots) {
        int32_t a = A[i * kEdtTile + c], b = B[i * kEdtTile + c];
        for (int d = 1; d <= reach; ++d) {
            const int32_t dd = d * d;
            if (dd >= a && dd >= b) break;
            if (i - d >= 0) {
                const int32_t ta = A[(i - d) * kEdtTile + c] + dd, tb = B[(i - d) * kEdtTile + c] + dd;
                a = ta < a ? ta : a;
                b = tb < b ? tb : b;
            }
            if (i + d < n) {
                const int32_t ta = A[(i + d) * kEdtTile + c] + dd, tb = B[(i + d) * kEdtTile + c] + dd;
                a = ta < a ? ta : a;
                b = tb < b ? tb : b;
            }
        }
        const size_t g = base + (size_t)i * (size_t)line_stride;
        p.g_occ[g] = a;
        p.g_free[g] = b;
    }
}

__global__ __launch_bounds__(kEdtThreads) void k_edt_finish(EdtParams p) {
    const int64_t nvox = (int64_t)p.nx * p.ny * p.nz;
    const int64_t e = (int64_t)blockIdx.x * kEdtThreads + threadIdx.x;
    if (e >= nvox) return;
    const int x = (int)(e % p.nx);
    const int64_t e1 = x + 1 < p.nx ? e + 1 : e;
    float2 pair;
    pair.x = edt_value(p.g_occ[e], p.g_free[e], p.voxel, p.cap);
    pair.y = edt_value(p.g_occ[e1], p.g_free[e1], p.voxel, p.cap);
    *(float2*)(p.cells + 2 * (size_t)e) = pair;
}

extern "C" int mppi_launch_edt_stage(const EdtParams* p, int stage, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    if (!p || !p->occ || !p->g_occ || !p->g_free || !p->cells) return -1;
    for (const int32_t n : {p->nx, p->ny, p->nz})
        if (n < 2 || n > kEdtMaxLine) return -1;
    const int64_t nvox = (int64_t)p->nx * p->ny * p->nz;
    if (nvox > (int64_t)(1 << 21) || p->window < 1 || !(p->voxel > 0.0f) || !(p->cap > 0.0f)) return -1;
    const dim3 block(kEdtThreads);
    const unsigned tiles = (unsigned)((p->nx + kEdtTile - 1) / kEdtTile);
    const auto lds = [](int n) { return (size_t)2 * (size_t)n * kEdtTile * sizeof(int32_t); };
    switch (stage) {
        case 0: {
            const int64_t rows = (int64_t)p->ny * p->nz;
            return go(k_edt_x, dim3((unsigned)((rows + kEdtThreads / 64 - 1) / (kEdtThreads / 64))), block, 0, s, *p);
        }
        case 1:
            return go(k_edt_axis, dim3(tiles, (unsigned)p->nz), block, lds(p->ny), s, *p, p->ny, p->nx, p->nx * p->ny);
        case 2:
            return go(k_edt_axis, dim3(tiles, (unsigned)p->ny), block, lds(p->nz), s, *p, p->nz, p->nx * p->ny, p->nx);
        case 3:
            return go(k_edt_finish, dim3((unsigned)((nvox + kEdtThreads - 1) / kEdtThreads)), block, 0, s, *p);
    }
    return -1;
}

extern "C" int mppi_launch_edt(const EdtParams* p, void* stream) {
    for (int stage = 0; stage < 4; ++stage) {
        const int rc = mppi_launch_edt_stage(p, stage, stream);
        if (rc != 0) return rc;
    }
    return 0;
}
