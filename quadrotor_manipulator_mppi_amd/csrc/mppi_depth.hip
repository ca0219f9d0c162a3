// mppi_depth.hip -- depth images into the occupancy map (mppi_integrate_depth, mppi_shift_map): the rays
// of one image carve free space out of the map's bytes and mark their end points, and the window move
// shifts the bytes.  Not part of the control step: HIP launches on the engine's stream, outside any batch,
// followed by the transform (mppi_edt.hip) that rebuilds the field from the map.
//
//   k_depth_carve  a group of kDepthGroup = 16 lanes per used pixel, lanes over the samples of its ray: lane
//                  q takes m = m_lo + q, m_lo + q + 16, ...  The rays of one wave differ in length by
//                  an order of magnitude (10 to 400 in-grid samples in a VGA frame at voxel 0.05), so one
//                  thread per ray would idle most lanes for most of the longest ray's march; here a wave
//                  idles at most 15 samples per ray.  Each lane of a group reads the same pixel (one
//                  address per group: the load coalesces) and forms the ray's constants itself -- some 50
//                  flops and up to seven IEEE divisions (1 / n, and two per moving axis in the slab clip),
//                  repeated by the 16 lanes, against a march of tens of samples.  A broadcast of the
//                  constants from one lane, and one thread per ray, were not built or measured against
//                  this.  Only the samples of the slab clip's range (mppi_depth.h
//                  depth_clip) are visited.  Every in-grid sample outside the ray's own end node stores 0.
//   k_depth_mark   one thread per used pixel: a return whose end point is in the grid stores 1.
//   k_map_shift    one thread per node: the old map (a copy in the transform's scratch) read at the shifted
//                  node, 0 where that is outside.
// Carve runs before mark on the stream, so occupied wins within a frame; both store constants, so duplicate
// stores are equal stores and the result does not depend on the order of the threads.
//
// Bounds.  The pixel index is formed from the block and thread ids and compared with the used rows and
// columns; the launcher checks the image and the dims.  A node index is formed only after depth_in_grid
// (mppi_depth.h): no value read from the image forms an address outside the map.
#include "mppi_device.h"
#include "mppi_depth.h"

__global__ __launch_bounds__(kDepthThreads) void k_depth_carve(DepthParams p) {
    const int q = threadIdx.x % kDepthGroup;
    const int64_t ray = (int64_t)blockIdx.x * (kDepthThreads / kDepthGroup) + threadIdx.x / kDepthGroup;
    if (ray >= (int64_t)p.cols * p.rows) return;
    const int i = (int)(ray % p.cols) * p.stride, j = (int)(ray / p.cols) * p.stride;
    if (i >= p.width || j >= p.height) return;
    DepthRay r;
    if (!depth_ray(p, i, j, p.depth[(size_t)j * (size_t)p.width + (size_t)i], r)) return;
    for (int m = r.m_lo + q; m <= r.m_hi; m += kDepthGroup) {
        const int64_t node = depth_sample(p, r, m);
        if (node >= 0) p.occ[node] = 0;
    }
}

__global__ __launch_bounds__(kDepthThreads) void k_depth_mark(DepthParams p) {
    const int64_t ray = (int64_t)blockIdx.x * kDepthThreads + threadIdx.x;
    if (ray >= (int64_t)p.cols * p.rows) return;
    const int i = (int)(ray % p.cols) * p.stride, j = (int)(ray / p.cols) * p.stride;
    if (i >= p.width || j >= p.height) return;
    DepthRay r;
    if (!depth_ray(p, i, j, p.depth[(size_t)j * (size_t)p.width + (size_t)i], r)) return;
    if (r.end >= 0) p.occ[r.end] = 1;
}

__global__ __launch_bounds__(kDepthThreads) void k_map_shift(ShiftParams p) {
    const int64_t nvox = (int64_t)p.nx * p.ny * p.nz;
    const int64_t e = (int64_t)blockIdx.x * kDepthThreads + threadIdx.x;
    if (e >= nvox) return;
    p.occ[e] = shift_value(p, e);
}

namespace {
bool dims_ok(int32_t nx, int32_t ny, int32_t nz) {
    for (const int32_t n : {nx, ny, nz})
        if (n < 2 || n > 512) return false;
    return (int64_t)nx * ny * nz <= (int64_t)(1 << 21);
}
}  // namespace

extern "C" int mppi_launch_depth(const DepthParams* p, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    if (!p || !p->depth || !p->occ || !dims_ok(p->nx, p->ny, p->nz)) return -1;
    if (p->width < 1 || p->height < 1 || (int64_t)p->width * p->height > (int64_t)kDepthMaxPixels || p->stride < 1) return -1;
    if (p->cols != depth_used(p->width, p->stride) || p->rows != depth_used(p->height, p->stride)) return -1;
    const int64_t rays = (int64_t)p->cols * p->rows;
    const dim3 block(kDepthThreads);
    if (p->carve) {
        const int per = kDepthThreads / kDepthGroup;
        const int rc = go(k_depth_carve, dim3((unsigned)((rays + per - 1) / per)), block, 0, s, *p);
        if (rc != 0) return rc;
    }
    return go(k_depth_mark, dim3((unsigned)((rays + kDepthThreads - 1) / kDepthThreads)), block, 0, s, *p);
}

extern "C" int mppi_launch_map_shift(const ShiftParams* p, void* stream) {
    if (!p || !p->src || !p->occ || p->src == p->occ || !dims_ok(p->nx, p->ny, p->nz)) return -1;
    if (p->sx < -p->nx || p->sx > p->nx || p->sy < -p->ny || p->sy > p->ny || p->sz < -p->nz || p->sz > p->nz) return -1;
    const int64_t nvox = (int64_t)p->nx * p->ny * p->nz;
    return go(k_map_shift, dim3((unsigned)((nvox + kDepthThreads - 1) / kDepthThreads)), dim3(kDepthThreads), 0,
              (hipStream_t)stream, *p);
}
