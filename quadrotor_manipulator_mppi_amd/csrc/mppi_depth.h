// mppi_depth.h -- depth images into the occupancy map (mppi_integrate_depth, mppi_shift_map,
// mppi_depth_integrate_host): what the kernels (mppi_depth.hip), their host entry points (mppi_engine.cpp)
// and the host twin (mppi_layout.cpp depth_integrate; tools/depth_host_check.cpp) share -- the ray of a
// pixel, the samples of a ray, the in-grid test, the launch parameters and the launchers.  Internal: not
// part of the public ABI.
//
// The definition (include/mppi_hip.h has it in full): a used pixel (i, j) with value z is skipped (NaN,
// -inf, z < z_min), a return (z_min <= z <= z_max) or a miss (z > z_max: the ray ends at z_max and marks
// nothing).  Its end point and the camera go to index coordinates ue, uo; the ray is sampled at
// u(m) = fmaf((float)m * inv_n, du, uo), 0 <= m < n, n = clamp(ceil(2 max|du|), 1, kDepthMaxSamples).  The
// in-grid samples' nodes are carved (a return's samples in its own end node excepted), then the in-grid end
// nodes of the returns are marked.  All of it is fp32, every product-sum an explicit fmaf, contraction off,
// one correctly rounded division per ray: the host and the device run these very inlines and agree bit for
// bit.
//
// Bounds.  A node index is formed only from a coordinate that passed depth_in_grid (-0.5 <= u < n - 0.5
// on all three axes, in float; NaN and +-inf fail every comparison), so it lies in [0, n) per axis: no
// value of the image or of the view can form an address outside the grid.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPPI_DEPTH_HD __host__ __device__
#else
#define MPPI_DEPTH_HD
#endif

namespace mppi {

constexpr int kDepthMaxSamples = 16384;     // MPPI_DEPTH_MAX_SAMPLES
constexpr int kDepthMaxPixels = 1 << 20;    // MPPI_DEPTH_MAX_PIXELS
constexpr float kDepthFltMax = 3.4028234663852886e38f;   // |x| <= this: x is finite
constexpr int kDepthThreads = 256;
constexpr int kDepthGroup = 16;             // lanes of one ray in k_depth_carve: 4 rays per wave, 16 per block

struct DepthParams {
    const float* depth;      // (height, width) metres along the optical axis
    uint8_t* occ;            // (nz, ny, nx) the map
    int32_t nx, ny, nz;
    int32_t width, height, stride;
    int32_t cols, rows;      // used columns and rows: ceil(width / stride), ceil(height / stride)
    int32_t carve;
    float inv_fx, inv_fy, cx, cy, z_min, z_max, inv_voxel;
    float R[9], pos[3], origin[3];
};

// rows or columns 0, stride, 2 stride, ... below n
inline int32_t depth_used(int32_t n, int32_t stride) { return (int32_t)(((int64_t)n + stride - 1) / stride); }

struct DepthRay {
    float uo[3], du[3];
    float inv_n;
    int32_t n;               // samples
    int32_t m_lo, m_hi;      // the samples that can lie in the grid: m_lo <= m <= m_hi (empty: m_lo > m_hi)
    int64_t end;             // a return's in-grid end node (flat index); -1: a miss, or an end point outside
};

// -0.5 <= u_d < n_d - 0.5 on all three axes, in float (false for NaN and +-inf)
MPPI_DEPTH_HD inline bool depth_in_grid(const DepthParams& p, float ux, float uy, float uz) {
    return ux >= -0.5f && ux < (float)p.nx - 0.5f && uy >= -0.5f && uy < (float)p.ny - 0.5f &&
           uz >= -0.5f && uz < (float)p.nz - 0.5f;
}
// the flat index of the node nearest to an in-grid point (call only after depth_in_grid)
MPPI_DEPTH_HD inline int64_t depth_node(const DepthParams& p, float ux, float uy, float uz) {
    const int ix = (int)floorf(ux + 0.5f), iy = (int)floorf(uy + 0.5f), iz = (int)floorf(uz + 0.5f);
    return ((int64_t)iz * p.ny + iy) * p.nx + ix;
}

// The samples that can lie in the grid, as a range of m (the slab clip the definition allows).  Sample m
// is fl(t_m du + uo) with t_m = fl(m fl(1/n)) = (m / n)(1 + 2 eps'), eps' <= 2^-24: it differs from the
// line's point at m / n by at most E_d = 2^-22 (|du_d| + |uo_d|) on axis d.  An in-grid sample therefore has
// its line point inside [-0.5 - E_d, n_d - 0.5 + E_d]; the clip uses the slab [-1 - 2 E_d, n_d + 2 E_d],
// half a voxel and E_d wider on either side, which covers the fp32 roundings of the clip itself (each
// quotient is off by a few ulp of (|bound| + |uo_d|) / |du_d| in t, that is by less than E_d in u), and
// takes one more sample at either end for the rounding of t n (less than 2^-10 of a sample).  An axis along
// which the ray does not move (|du_d| below 1e-30: the quotients would overflow) only tests uo_d.
MPPI_DEPTH_HD inline void depth_clip(const DepthParams& p, DepthRay& r) {
#pragma clang fp contract(off)
    float t0 = 0.0f, t1 = 1.0f;
    const float nd[3] = {(float)p.nx, (float)p.ny, (float)p.nz};
    bool empty = false;
    for (int d = 0; d < 3; ++d) {
        const float E = 4.76837158203125e-07f * (fabsf(r.du[d]) + fabsf(r.uo[d]));   // 2^-21 (...) = 2 E_d
        const float lo = -1.0f - E, hi = nd[d] + E;
        if (!(fabsf(r.du[d]) <= kDepthFltMax)) { empty = true; continue; }   // du_d = +-inf: every sample is non-finite
        if (fabsf(r.du[d]) < 1e-30f) {
            if (!(r.uo[d] >= lo && r.uo[d] <= hi)) empty = true;
            continue;
        }
        const float a = (lo - r.uo[d]) / r.du[d], b = (hi - r.uo[d]) / r.du[d];
        t0 = fmaxf(t0, fminf(a, b));
        t1 = fminf(t1, fmaxf(a, b));
    }
    if (empty || !(t0 <= t1)) { r.m_lo = 0; r.m_hi = -1; return; }
    const float fn = (float)r.n;
    const int lo = (int)floorf(t0 * fn) - 1, hi = (int)ceilf(t1 * fn) + 1;   // (t in [0, 1]: |t n| <= 16384)
    r.m_lo = lo < 0 ? 0 : lo;
    r.m_hi = hi > r.n - 1 ? r.n - 1 : hi;
}

// The ray of used pixel (i, j) with value z.  false: the pixel is skipped (z is NaN, -inf or < z_min, or
// the end point or the camera is not finite in index coordinates).
MPPI_DEPTH_HD inline bool depth_ray(const DepthParams& p, int i, int j, float z, DepthRay& r) {
#pragma clang fp contract(off)
    if (!(z >= p.z_min)) return false;
    const bool hit = z <= p.z_max;
    if (!hit) z = p.z_max;
    const float xn = ((float)i - p.cx) * p.inv_fx, yn = ((float)j - p.cy) * p.inv_fy;
    const float p0 = xn * z, p1 = yn * z, p2 = z;
    float ue[3];
    bool finite = true;
    for (int d = 0; d < 3; ++d) {
        const float w = fmaf(p.R[3 * d], p0, fmaf(p.R[3 * d + 1], p1, fmaf(p.R[3 * d + 2], p2, p.pos[d])));
        ue[d] = (w - p.origin[d]) * p.inv_voxel;
        r.uo[d] = (p.pos[d] - p.origin[d]) * p.inv_voxel;
        finite = finite && fabsf(ue[d]) <= kDepthFltMax && fabsf(r.uo[d]) <= kDepthFltMax;
    }
    if (!finite) return false;
    float L = 0.0f;
    for (int d = 0; d < 3; ++d) {
        r.du[d] = ue[d] - r.uo[d];
        L = fmaxf(L, fabsf(r.du[d]));
    }
    r.n = (int)fminf(fmaxf(ceilf(2.0f * L), 1.0f), (float)kDepthMaxSamples);
    r.inv_n = 1.0f / (float)r.n;
    r.end = hit && depth_in_grid(p, ue[0], ue[1], ue[2]) ? depth_node(p, ue[0], ue[1], ue[2]) : -1;
    depth_clip(p, r);
    return true;
}

// The node sample m of a ray carves; -1: none (the sample is outside the grid, or in the ray's own end node).
MPPI_DEPTH_HD inline int64_t depth_sample(const DepthParams& p, const DepthRay& r, int m) {
#pragma clang fp contract(off)
    const float t = (float)m * r.inv_n;
    const float ux = fmaf(t, r.du[0], r.uo[0]), uy = fmaf(t, r.du[1], r.uo[1]), uz = fmaf(t, r.du[2], r.uo[2]);
    if (!depth_in_grid(p, ux, uy, uz)) return -1;
    const int64_t node = depth_node(p, ux, uy, uz);
    return node == r.end ? -1 : node;
}

struct ShiftParams {
    const uint8_t* src;      // the map as it was (a copy in the transform's scratch)
    uint8_t* occ;            // the map
    int32_t nx, ny, nz;
    int32_t sx, sy, sz;      // each within [-n_d, n_d]
};
// the new value of node e: the old node (ix + sx, iy + sy, iz + sz), free where that falls outside
MPPI_DEPTH_HD inline uint8_t shift_value(const ShiftParams& p, int64_t e) {
    const int ix = (int)(e % p.nx), iy = (int)((e / p.nx) % p.ny), iz = (int)(e / ((int64_t)p.nx * p.ny));
    const int ox = ix + p.sx, oy = iy + p.sy, oz = iz + p.sz;
    if (ox < 0 || ox >= p.nx || oy < 0 || oy >= p.ny || oz < 0 || oz >= p.nz) return 0;
    return p.src[((int64_t)oz * p.ny + oy) * p.nx + ox] != 0 ? 1 : 0;
}

}  // namespace mppi

extern "C" {
// The two passes of one image on a stream: k_depth_carve (skipped with carve = 0), then k_depth_mark.
// 0 launched, -1 refused (null pointers, dims outside 2..512 or their product past 2^21, an image outside
// 1..kDepthMaxPixels, a stride < 1), > 0 a HIP error.
int mppi_launch_depth(const mppi::DepthParams* p, void* stream);
// k_map_shift: occ from src.  Same returns (-1 also for a shift outside [-n_d, n_d]).
int mppi_launch_map_shift(const mppi::ShiftParams* p, void* stream);
}
