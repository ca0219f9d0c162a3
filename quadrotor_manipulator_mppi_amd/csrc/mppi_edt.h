// mppi_edt.h -- the occupancy grid's way into the distance field (mppi_set_occupancy, mppi_occupancy_field):
// what the transform's kernels (mppi_edt.hip), its host entry points (mppi_engine.cpp) and the host twin
// (mppi_layout.cpp occupancy_field; tools/occupancy_host_check.cpp) share -- the definition of the value,
// the sentinel, the launch parameters and the launchers.  Internal: not part of the public ABI.
//
// The definition (include/mppi_hip.h has it in full): D2_occ(n) / D2_free(n) = the smallest squared index
// distance from node n to an occupied / a free node of the grid (outside the grid: no seeds);
//   free node      d = +voxel (sqrt(D2_occ)  - 0.5)
//   occupied node  d = -voxel (sqrt(D2_free) - 0.5)
// clamped to [-cap, +cap]; a seed set that is empty reads the cap itself.  edt_value below is that, in
// fp32 with a correctly rounded square root: every operation is exactly rounded, so the host and the
// device agree bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPPI_EDT_HD __host__ __device__
#else
#define MPPI_EDT_HD
#endif

namespace mppi {

// "No seed": more than any in-grid squared distance (3 * 511^2 = 783363) and small enough to survive the
// two further (i - j)^2 <= 511^2 terms of the y and the z pass in int32.
constexpr int32_t kEdtInf = 1 << 29;
constexpr int kEdtTile = 16;        // adjacent x columns of one y / z pass block: 64 B rows, 2 grids * 512 * 16 * 4 B = 64 KiB of LDS at most
constexpr int kEdtThreads = 256;
constexpr int kEdtMaxLine = 512;    // kFieldMaxDim

// the cap of mppi_set_occupancy's max_dist (> 0: itself; else more than any in-grid distance)
inline float edt_cap(const int32_t dims[3], float voxel, float max_dist) {
    return max_dist > 0.0f ? max_dist : voxel * (float)(dims[0] + dims[1] + dims[2]);
}
// The y and z passes' window: a minimiser further than this along an axis gives a value the cap clamps
// anyway (its D2 >= (w + 1)^2 > (cap / voxel + 0.5)^2), and a result the clamp leaves alone has its
// minimiser inside the window on both axes, so the cut changes no output.
inline int32_t edt_window(float voxel, float cap) {
    const double w = ceil((double)cap / (double)voxel) + 1.0;
    return w < (double)kEdtMaxLine ? (int32_t)w : kEdtMaxLine;
}

MPPI_EDT_HD inline float edt_side(int32_t d2, float voxel, float cap) {
    if (d2 >= kEdtInf) return cap;
    const float t = sqrtf((float)d2);   // (d2 < 2^24: the conversion is exact)
    const float d = voxel * (t - 0.5f);
    return fminf(d, cap);
}
// the signed value of one node from its two squared distances (occupied <=> d2_occ == 0)
MPPI_EDT_HD inline float edt_value(int32_t d2_occ, int32_t d2_free, float voxel, float cap) {
    return d2_occ == 0 ? -edt_side(d2_free, voxel, cap) : edt_side(d2_occ, voxel, cap);
}

struct EdtParams {
    const uint8_t* occ;   // (nz, ny, nx) nonzero = occupied
    int32_t* g_occ;       // the two int32 grids (nz, ny, nx): squared distance to the nearest occupied /
    int32_t* g_free;      //   free node so far (the axes done), kEdtInf = none
    float* cells;         // the field buffer past its header: one x-pair per node
    int32_t nx, ny, nz;
    int32_t window;       // edt_window
    float voxel, cap;
};

// bytes of device scratch for a grid of nvox nodes: the two grids, then the occupancy
inline size_t edt_scratch_bytes(int64_t nvox) { return (size_t)nvox * (2 * sizeof(int32_t) + 1); }

}  // namespace mppi

extern "C" {
// One launch of the transform: stage 0 the x pass, 1 the y pass, 2 the z pass, 3 the finish (sign, root,
// clamp, x-pair stores).  0 launched (or described into the capture target), -1 refused (null pointers,
// dims outside 2..512 or their product past 2^21), > 0 a HIP error.
int mppi_launch_edt_stage(const mppi::EdtParams* p, int stage, void* stream);
// All four, in order.
int mppi_launch_edt(const mppi::EdtParams* p, void* stream);
}
