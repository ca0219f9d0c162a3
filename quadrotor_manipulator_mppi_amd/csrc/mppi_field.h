// mppi_field.h -- the distance field of a field engine (mppi_create_scene_field): the layout of its
// device buffer and the sampling of one world point.  Shared by the field rollout (mppi_rollout.h
// rollout_body FLD), the plan kernel (mppi_plan.hip) and the host (mppi_layout.cpp validates and packs,
// mppi_debug_field_sample and tools/field_host_check.cpp replay it), so it compiles as HIP and as plain C++.
//
// The field buffer, in 4-byte words:
//   header (kFieldHdrW words, wave-uniform: the kernels stage it in LDS beside the scene)
//     [0..2] origin (m, world axes)   [3] 1 / voxel   [4..6] nx, ny, nz   [7] set flag (0: contributes nothing)
//     [8] row stride nx   [9] slab stride nx * ny (both in cells)   [10] nx * ny * nz   [11] voxel (m)   [12..15] spare
//   cells, from word kFieldHdrW on: one 8-byte x-pair per node, C order (nz, ny, nx),
//     cell (iz, iy, ix) = (d[iz][iy][ix], d[iz][iy][min(ix + 1, nx - 1)])
//   so the two x-neighbours of a sample come with one 8 B load: four loads per sample instead of eight
//   4 B ones, at twice the memory (at most 2^21 cells: 16 MiB).
// Dims and voxel are fixed at creation; the origin, the set flag and the cells are what an upload replaces.
//
// Sampling at c (field_sample): u = (c - origin) * (1 / voxel) per axis, clamped to [0, n - 1] with the
// constant as fmaxf / fminf's surviving operand, so a NaN coordinate lands on 0 and +-inf on a face; the
// integer conversion comes after the clamp, i = min((int)u, n - 2) >= 0, f = u - i in [0, 1]; the 8 nodes
// are interpolated x, then y, then z, each lerp fmaf(f, b - a, a).  No coordinate can form an index
// outside the grid: a point outside reads the value at its clamped position.
#pragma once
#include "mppi_obstacles.h"

namespace mppi {

constexpr int kFieldHdrW = 16;
constexpr int kFieldMaxVoxels = 1 << 21, kFieldMaxDim = 512;
constexpr inline int64_t field_words(int64_t nvox) { return kFieldHdrW + 2 * nvox; }

// the clamped cell index and fraction of one axis: u in grid units, n nodes (n >= 2)
MPPI_OBS_FN void field_axis(float u, int n, int& i, float& f) {
    u = fminf(fmaxf(u, 0.0f), (float)(n - 1));
    const int iu = (int)u;
    i = iu < n - 2 ? iu : n - 2;
    f = u - (float)i;
}

MPPI_OBS_FN void field_pair(const float* cells, int e, float& a, float& b) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float2 p = *(const float2*)(cells + 2 * (size_t)e);
    a = p.x; b = p.y;
#else
    a = cells[2 * (size_t)e]; b = cells[2 * (size_t)e + 1];
#endif
}

// d(c): hdr = the header (device: its LDS copy), cells = the buffer past the header.  idx (may be null):
// the eight nodes' linear indices into d[iz][iy][ix], x fastest, then y, then z.
MPPI_OBS_FN float field_sample(const float* hdr, const float* cells, float cx, float cy, float cz, int32_t* idx = nullptr) {
    const int nx = scene_int(hdr + 4), ny = scene_int(hdr + 5), nz = scene_int(hdr + 6);
    const int sy = scene_int(hdr + 8), sz = scene_int(hdr + 9);
    const float inv = hdr[3];
    int ix, iy, iz;
    float fx, fy, fz;
    field_axis((cx - hdr[0]) * inv, nx, ix, fx);
    field_axis((cy - hdr[1]) * inv, ny, iy, fy);
    field_axis((cz - hdr[2]) * inv, nz, iz, fz);
    const int e = iz * sz + iy * sy + ix;
    float a0, b0, a1, b1, a2, b2, a3, b3;
    field_pair(cells, e, a0, b0);
    field_pair(cells, e + sy, a1, b1);
    field_pair(cells, e + sz, a2, b2);
    field_pair(cells, e + sz + sy, a3, b3);
    const float x00 = fmaf(fx, b0 - a0, a0), x10 = fmaf(fx, b1 - a1, a1);
    const float x01 = fmaf(fx, b2 - a2, a2), x11 = fmaf(fx, b3 - a3, a3);
    const float y0 = fmaf(fy, x10 - x00, x00), y1 = fmaf(fy, x11 - x01, x01);
    if (idx) {
        for (int k = 0; k < 8; ++k) idx[k] = e + (k & 1) + ((k >> 1) & 1) * sy + (k >> 2) * sz;
    }
    return fmaf(fz, y1 - y0, y0);
}

// obs_frame with the field as one more obstacle: each sphere of the slot against the vehicle's
// obstacles, then -- where the field is set -- its centre sampled, g = d(c) - r_b into the same
// accumulators.  The centre and the pair loop are obs_frame's, restated, not shared: lifted into helpers
// that both call, they changed the register allocation of all 32 scene kernels (tried; the scene code
// objects must stay as they are), as mppi_plan.hip found for the chain loops.  Keep the two in step.
MPPI_OBS_FN void obs_frame_field(const float* T, const float* body, const float* veh, int slot, float tau,
                                 const float* fhdr, const float* cells, float& hinge, float& gmin) {
    const int b0 = scene_int(body + kSceneRng + slot), b1 = scene_int(body + kSceneRng + slot + 1);
    const int n = scene_int(veh);
    const bool set = scene_int(fhdr + 7) != 0;
    const float margin = body[2];
    for (int b = b0; b < b1; ++b) {
        const float* s = body + kSceneSph + 4 * b;
        const float cx = fmaf(T[0], s[0], fmaf(T[1], s[1], fmaf(T[2], s[2], T[3])));
        const float cy = fmaf(T[4], s[0], fmaf(T[5], s[1], fmaf(T[6], s[2], T[7])));
        const float cz = fmaf(T[8], s[0], fmaf(T[9], s[1], fmaf(T[10], s[2], T[11])));
        for (int o = 0; o < n; ++o) obs_pair(cx, cy, cz, s[3], veh + 4 + 8 * o, tau, margin, hinge, gmin);
        if (set) {
            const float g = field_sample(fhdr, cells, cx, cy, cz) - s[3];
            hinge += fmaxf(0.0f, margin - g);
            gmin = fminf(gmin, g);
        }
    }
}

}  // namespace mppi
