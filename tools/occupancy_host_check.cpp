// occupancy_host_check.cpp -- the host code of occupancy grids (mppi_occupancy_field; mppi_set_occupancy's
// argument check) as a stand-alone program for the sanitizers (tools/, not shipped).  No GPU, no Python:
//
//   cd quadrotor_manipulator_mppi_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I . -I ../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Xarch_host -fno-omit-frame-pointer \
//       ../../tools/occupancy_host_check.cpp mppi_layout.cpp mppi_host_math.cpp -o ../../tools/_bin/occupancy_host_check
//   ../../tools/_bin/occupancy_host_check
//
// The helper on a few grids, the occupancy and the output in exactly-sized heap blocks, so
// AddressSanitizer sees any index past either end: the 2 x 2 x 2 and 512 x 2 x 2 corners (and the latter
// turned onto y and z), odd sizes, the largest legal grid (128^3); patterns: empty, full, one corner node,
// a box, random.  On the small grids every node is compared with a brute-force search over all seeds
// through the same inline (mppi_edt.h edt_value), bit for bit; on all of them the sign is the occupancy and
// |d| stays within the cap.  Then the error returns.  Exit status 0 and a count line when all hold.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mppi_layout.h"

using namespace mppi;
using namespace mppi_host;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s (line %d)\n", #x, __LINE__); ++fails; } } while (0)

static mppi_field_desc desc(int nx, int ny, int nz, float voxel) {
    mppi_field_desc f;
    std::memset(&f, 0, sizeof(f));
    f.dims[0] = nx; f.dims[1] = ny; f.dims[2] = nz;
    f.voxel = voxel;
    return f;
}

static uint32_t lcg = 2463534242u;
static uint32_t rnd() { lcg = lcg * 1664525u + 1013904223u; return lcg >> 8; }

// 0 empty, 1 full, 2 the far corner of x, 3 a box, 4 random 2 %, 5 random 50 %
static std::vector<uint8_t> pattern(const mppi_field_desc& f, int kind) {
    const int nx = f.dims[0], ny = f.dims[1], nz = f.dims[2];
    std::vector<uint8_t> o((size_t)field_voxels(f), kind == 1 ? 1 : 0);
    if (kind == 2) o[(size_t)nx - 1] = 200;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                uint8_t& v = o[((size_t)z * ny + y) * nx + x];
                if (kind == 3) v = x >= nx / 4 && x <= nx / 2 && y >= ny / 4 && y <= ny / 2 && z >= nz / 4 && z <= nz / 2;
                if (kind == 4) v = rnd() % 50 == 0;
                if (kind == 5) v = rnd() % 2 == 0 ? 255 : 0;
            }
    return o;
}

static int run(const mppi_field_desc& f, int kind, float max_dist, bool brute) {
    const int nx = f.dims[0], ny = f.dims[1], nz = f.dims[2];
    const std::vector<uint8_t> o = pattern(f, kind);
    std::vector<float> d((size_t)field_voxels(f), std::numeric_limits<float>::quiet_NaN());
    CHECK(mppi_occupancy_field(&f, o.data(), max_dist, d.data()) == MPPI_OK);
    const float cap = edt_cap(f.dims, f.voxel, max_dist);
    int n = 0;
    for (size_t e = 0; e < d.size(); ++e) {
        CHECK(std::isfinite(d[e]) && std::fabs(d[e]) <= cap && (d[e] < 0.0f) == (o[e] != 0));
        ++n;
    }
    if (kind == 0) for (const float v : d) CHECK(v == cap);
    if (kind == 1) for (const float v : d) CHECK(v == -cap);
    if (!brute) return n;
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                int32_t best[2] = {kEdtInf, kEdtInf};   // to the nearest occupied, free node
                for (int c = 0; c < nz; ++c)
                    for (int b = 0; b < ny; ++b)
                        for (int a = 0; a < nx; ++a) {
                            const int32_t q = (a - x) * (a - x) + (b - y) * (b - y) + (c - z) * (c - z);
                            int32_t& m = best[o[((size_t)c * ny + b) * nx + a] ? 0 : 1];
                            if (q < m) m = q;
                        }
                const float want = edt_value(best[0], best[1], f.voxel, cap);
                const float got = d[((size_t)z * ny + y) * nx + x];
                CHECK(std::memcmp(&want, &got, sizeof(float)) == 0);
                ++n;
            }
    return n;
}

int main() {
    int n_checked = 0;
    const float voxel = 0.05f;
    // ---- small grids against brute force: the corners of the dims, odd sizes
    const int small[][3] = {{2, 2, 2}, {512, 2, 2}, {2, 512, 2}, {2, 2, 512}, {7, 5, 3}, {33, 6, 9}, {3, 70, 4}};
    for (const auto& s : small) {
        const mppi_field_desc f = desc(s[0], s[1], s[2], voxel);
        CHECK(field_validate(&f) == MPPI_OK);
        for (int kind = 0; kind < 6; ++kind)
            for (const float md : {0.0f, 3.5f * voxel, 1e6f}) n_checked += run(f, kind, md, true);
    }
    // ---- the largest legal grids: indices only (sign, cap, finite), under the sanitizers
    const int large[][3] = {{128, 128, 128}, {512, 512, 8}, {8, 512, 512}};
    for (const auto& s : large) {
        const mppi_field_desc f = desc(s[0], s[1], s[2], voxel);
        for (const int kind : {2, 3, 4}) n_checked += run(f, kind, kind == 2 ? 0.0f : 1.0f, false);
    }
    // ---- one free node in a full grid, one occupied node in an empty one: half a voxel either side of the face
    {
        const mppi_field_desc f = desc(5, 4, 3, voxel);
        std::vector<uint8_t> o((size_t)field_voxels(f), 1);
        std::vector<float> d(o.size());
        o[7] = 0;
        CHECK(mppi_occupancy_field(&f, o.data(), 0.0f, d.data()) == MPPI_OK);
        CHECK(d[7] == 0.5f * voxel && d[6] == -0.5f * voxel && d[8] == -0.5f * voxel);
        std::memset(o.data(), 0, o.size());
        o[7] = 1;
        CHECK(mppi_occupancy_field(&f, o.data(), 0.0f, d.data()) == MPPI_OK);
        CHECK(d[7] == -0.5f * voxel && d[6] == 0.5f * voxel && d[9] == voxel * (std::sqrt(4.0f) - 0.5f));
        n_checked += 6;
    }
    // ---- error returns
    {
        const mppi_field_desc f = desc(5, 4, 3, voxel);
        std::vector<uint8_t> o((size_t)field_voxels(f), 0);
        std::vector<float> d(o.size());
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
        CHECK(mppi_occupancy_field(nullptr, o.data(), 0.0f, d.data()) == MPPI_ERR_INVALID_ARG);
        CHECK(mppi_occupancy_field(&f, nullptr, 0.0f, d.data()) == MPPI_ERR_INVALID_ARG);
        CHECK(mppi_occupancy_field(&f, o.data(), 0.0f, nullptr) == MPPI_ERR_INVALID_ARG);
        CHECK(mppi_occupancy_field(&f, o.data(), nan, d.data()) == MPPI_ERR_INVALID_ARG);
        CHECK(mppi_occupancy_field(&f, o.data(), inf, d.data()) == MPPI_ERR_INVALID_ARG);
        CHECK(mppi_occupancy_field(&f, o.data(), -inf, d.data()) == MPPI_OK);
        const mppi_field_desc bad = desc(513, 4, 3, voxel), big = desc(512, 512, 16, voxel), one = desc(1, 4, 3, voxel);
        for (const mppi_field_desc* b : {&bad, &big, &one}) CHECK(mppi_occupancy_field(b, o.data(), 0.0f, d.data()) == MPPI_ERR_INVALID_ARG);
        const float o3[3] = {0.0f, nan, 0.0f}, ok3[3] = {1.0f, 2.0f, 3.0f};
        CHECK(occupancy_validate(o3, o.data(), 0.0f) == MPPI_ERR_INVALID_ARG);
        CHECK(occupancy_validate(ok3, o.data(), 1.0f) == MPPI_OK && occupancy_validate(nullptr, o.data(), 0.0f) == MPPI_OK);
        CHECK(occupancy_validate(ok3, nullptr, 0.0f) == MPPI_ERR_INVALID_ARG);
        CHECK(edt_window(voxel, 3.5f * voxel) == 5 && edt_window(voxel, 1e6f) == kEdtMaxLine);
        n_checked += 15;
    }
    std::printf("%s: %d checks, %d failed\n", fails ? "FAILED" : "ok", n_checked, fails);
    return fails ? 1 : 0;
}
