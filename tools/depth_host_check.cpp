// depth_host_check.cpp -- the host code of depth-image integration (mppi_depth_integrate_host; the window move's
// host twin; their argument checks) as a stand-alone program for the sanitizers (tools/, not shipped).  No
// GPU, no Python:
//
//   cd quadrotor_manipulator_mppi_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I . -I ../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Xarch_host -fno-omit-frame-pointer \
//       ../../tools/depth_host_check.cpp mppi_layout.cpp mppi_host_math.cpp -o ../../tools/_bin/depth_host_check
//   ../../tools/_bin/depth_host_check
//
// The twin on a few grids and images, the image and the map in exactly-sized heap blocks, so AddressSanitizer
// sees any index past either end: the 2 x 2 x 2 and 512 x 2 x 2 corners, 1 x 1 and odd images, strides that
// do and do not divide the image, the camera inside the grid, outside it and on its faces; then hostile
// values -- NaN, +-inf, negatives and 3e38 in the image, poses at 1e30 and 3e38, a z range up to the limit --
// which by the definition form no address; on every run the map holds 0 or 1 only, a frame integrated twice
// gives the same map, carve = 0 clears nothing, and on the small cases every in-grid sample of a brute-force
// march over all m (no slab clip) through the same inlines lands on the same map.  Then the window move
// against a direct loop, and the error returns.  Exit status 0 and a count line when all hold.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "mppi_layout.h"

using namespace mppi;
using namespace mppi_host;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s (line %d)\n", #x, __LINE__); ++fails; } } while (0)

static const float kInf = std::numeric_limits<float>::infinity(), kNan = std::numeric_limits<float>::quiet_NaN();

static mppi_field_desc desc(int nx, int ny, int nz, float voxel) {
    mppi_field_desc f;
    std::memset(&f, 0, sizeof(f));
    f.dims[0] = nx; f.dims[1] = ny; f.dims[2] = nz;
    f.voxel = voxel;
    f.origin[0] = 0.25f; f.origin[1] = -0.5f; f.origin[2] = 1.0f;
    return f;
}

static mppi_depth_view view(int w, int h, int stride, const mppi_field_desc& f, float ux, float uy, float uz) {
    mppi_depth_view v;
    std::memset(&v, 0, sizeof(v));
    v.width = w; v.height = h; v.stride = stride; v.carve = 1;
    v.fx = 0.8f * (float)w + 0.5f; v.fy = v.fx; v.cx = 0.5f * (float)w - 0.3f; v.cy = 0.5f * (float)h - 0.1f;
    v.z_min = 0.05f; v.z_max = 3.0f;
    v.pos[0] = f.origin[0] + f.voxel * ux; v.pos[1] = f.origin[1] + f.voxel * uy; v.pos[2] = f.origin[2] + f.voxel * uz;
    // looking along +x, slightly off: the optical z axis on world x, x (right) on -y, y (down) on -z
    v.quat_xyzw[0] = 0.52f; v.quat_xyzw[1] = -0.49f; v.quat_xyzw[2] = 0.5f; v.quat_xyzw[3] = -0.51f;
    return v;
}

static uint32_t lcg = 2463534242u;
static uint32_t rnd() { lcg = lcg * 1664525u + 1013904223u; return lcg >> 8; }

// kind 0: a wall with holes; 1: hostile values
static std::unique_ptr<float[]> image(int w, int h, int kind) {
    std::unique_ptr<float[]> d(new float[(size_t)w * h]);
    const float hostile[] = {kNan, kInf, -kInf, -1.0f, 3e38f, 0.0f, 1.0f, 1.7f, 1e-30f, -0.0f};
    for (int i = 0; i < w * h; ++i)
        d[i] = kind == 1 ? hostile[rnd() % 10] : (rnd() % 7 == 0 ? kInf : 0.3f + 0.001f * (float)(rnd() % 2000));
    return d;
}

// the map after one frame by a march over every m of every ray, through the same inlines but without the clip
static void brute(const mppi_field_desc& f, const mppi_depth_view& v, const float* depth, uint8_t* occ) {
    DepthParams p;
    depth_params(f, v, p);
    const int64_t nvox = field_voxels(f);
    for (int64_t e = 0; e < nvox; ++e) occ[e] = occ[e] != 0;
    for (int pass = v.carve ? 0 : 1; pass < 2; ++pass)
        for (int j = 0; j < v.height; j += v.stride)
            for (int i = 0; i < v.width; i += v.stride) {
                DepthRay r;
                if (!depth_ray(p, i, j, depth[(size_t)j * v.width + i], r)) continue;
                if (pass == 1) { if (r.end >= 0) { CHECK(r.end < nvox); occ[r.end] = 1; } continue; }
                for (int m = 0; m < r.n; ++m) {
                    const int64_t node = depth_sample(p, r, m);
                    CHECK(node < nvox);
                    if (node >= 0) {
                        CHECK(m >= r.m_lo && m <= r.m_hi);   // the clip is conservative
                        occ[node] = 0;
                    }
                }
            }
}

static int run(const mppi_field_desc& f, mppi_depth_view v, int kind, bool with_brute) {
    const size_t nvox = (size_t)field_voxels(f);
    const std::unique_ptr<float[]> d = image(v.width, v.height, kind);
    std::unique_ptr<uint8_t[]> a(new uint8_t[nvox]), b(new uint8_t[nvox]), c(new uint8_t[nvox]);
    for (size_t e = 0; e < nvox; ++e) a[e] = rnd() % 5 == 0 ? (uint8_t)(1 + rnd() % 255) : 0;
    std::memcpy(b.get(), a.get(), nvox);
    std::memcpy(c.get(), a.get(), nvox);
    CHECK(mppi_depth_integrate_host(&f, &v, d.get(), b.get()) == MPPI_OK);
    int n = 0;
    for (size_t e = 0; e < nvox; ++e) { CHECK(b[e] <= 1); ++n; }
    if (with_brute) {
        brute(f, v, d.get(), c.get());
        CHECK(std::memcmp(b.get(), c.get(), nvox) == 0);
        ++n;
    }
    std::memcpy(c.get(), b.get(), nvox);
    CHECK(mppi_depth_integrate_host(&f, &v, d.get(), c.get()) == MPPI_OK);
    CHECK(std::memcmp(b.get(), c.get(), nvox) == 0);   // the same frame twice
    v.carve = 0;
    std::memcpy(c.get(), a.get(), nvox);
    CHECK(mppi_depth_integrate_host(&f, &v, d.get(), c.get()) == MPPI_OK);
    for (size_t e = 0; e < nvox; ++e) CHECK(!(a[e] != 0 && c[e] == 0));   // mark only: nothing is cleared
    return n + 2;
}

int main() {
    int n_checked = 0;
    const float voxel = 0.05f;
    static_assert(sizeof(mppi_depth_view) == 80, "mppi_depth_view");
    // ---- grids x images x strides x camera positions (index coordinates), against the unclipped march
    const int grids[][3] = {{2, 2, 2}, {512, 2, 2}, {2, 512, 2}, {2, 2, 512}, {7, 5, 3}, {33, 17, 9}};
    const int images[][3] = {{1, 1, 1}, {7, 5, 1}, {7, 5, 3}, {7, 5, 9}, {33, 21, 2}};
    for (const auto& g : grids) {
        const mppi_field_desc f = desc(g[0], g[1], g[2], voxel);
        CHECK(field_validate(&f) == MPPI_OK);
        const float cams[][3] = {{0.37f, 0.41f, 0.43f}, {-0.5f, 0.0f, 0.0f}, {-7.3f, 0.6f, 0.2f}, {(float)g[0] - 0.5f, 0.5f, 0.5f},
                                 {(float)g[0] + 3.2f, 0.5f, 0.5f}, {0.5f * (float)g[0], -40.0f, 0.3f}};
        for (const auto& im : images)
            for (const auto& cam : cams)
                for (int kind = 0; kind < 2; ++kind)
                    n_checked += run(f, view(im[0], im[1], im[2], f, cam[0], cam[1], cam[2]), kind, true);
    }
    // ---- a larger frame into a larger grid, and the longest rays the z limit allows (16384 samples each)
    {
        const mppi_field_desc f = desc(64, 48, 40, voxel);
        n_checked += run(f, view(160, 120, 1, f, 3.3f, 20.2f, 17.7f), 0, false);
        mppi_depth_view v = view(7, 5, 1, f, -3000.0f, 20.2f, 17.7f);
        v.z_max = 4095.0f * voxel;
        n_checked += run(f, v, 1, true);
    }
    // ---- hostile poses: far away, at the edge of the float range, and mixed
    {
        const mppi_field_desc f = desc(33, 17, 9, voxel);
        const float far[][3] = {{1e30f, -1e30f, 1e30f}, {3e38f, 3e38f, -3e38f}, {0.4f, 1e30f, 1.2f}, {-3.4e38f, 0.0f, 1.0f}};
        for (const auto& p : far)
            for (int kind = 0; kind < 2; ++kind) {
                mppi_depth_view v = view(7, 5, 1, f, 0.0f, 0.0f, 0.0f);
                for (int d = 0; d < 3; ++d) v.pos[d] = p[d];
                v.z_max = 200.0f;
                n_checked += run(f, v, kind, true);
            }
    }
    // ---- the window move against a direct loop
    {
        const int g[][3] = {{2, 2, 2}, {512, 2, 2}, {7, 5, 3}};
        const int shifts[][3] = {{0, 0, 0}, {1, 0, 0}, {-1, 1, -1}, {0, -2, 1}, {511, 0, 0}, {512, 0, 0}, {2147483647, 0, 0},
                                 {0, 0, -2147483647 - 1}};
        for (const auto& d3 : g)
            for (const auto& s : shifts) {
                const mppi_field_desc f = desc(d3[0], d3[1], d3[2], voxel);
                const size_t nvox = (size_t)field_voxels(f);
                std::unique_ptr<uint8_t[]> a(new uint8_t[nvox]), b(new uint8_t[nvox]);
                for (size_t e = 0; e < nvox; ++e) a[e] = rnd() % 3 == 0 ? (uint8_t)(1 + rnd() % 255) : 0;
                ShiftParams p;
                float origin[3];
                CHECK(shift_validate(f, s, 0.0f, p, origin) == MPPI_OK);
                p.src = a.get(); p.occ = b.get();
                map_shift(p);
                for (int z = 0; z < d3[2]; ++z)
                    for (int y = 0; y < d3[1]; ++y)
                        for (int x = 0; x < d3[0]; ++x) {
                            const int64_t ox = (int64_t)x + s[0], oy = (int64_t)y + s[1], oz = (int64_t)z + s[2];
                            const bool in = ox >= 0 && ox < d3[0] && oy >= 0 && oy < d3[1] && oz >= 0 && oz < d3[2];
                            const uint8_t want = in ? a[(size_t)((oz * d3[1] + oy) * d3[0] + ox)] != 0 : 0;
                            CHECK(b[((size_t)z * d3[1] + y) * d3[0] + x] == want);
                            ++n_checked;
                        }
                for (int d = 0; d < 3; ++d) CHECK(origin[d] == fmaf((float)s[d], voxel, f.origin[d]));
            }
    }
    // ---- error returns
    {
        const mppi_field_desc f = desc(7, 5, 3, voxel);
        const mppi_depth_view ok = view(7, 5, 1, f, 0.4f, 0.4f, 0.4f);
        const std::unique_ptr<float[]> d = image(7, 5, 0);
        std::unique_ptr<uint8_t[]> o(new uint8_t[(size_t)field_voxels(f)]());
        const auto st = [&](const mppi_depth_view& v) { return mppi_depth_integrate_host(&f, &v, d.get(), o.get()); };
        CHECK(st(ok) == MPPI_OK);
        CHECK(mppi_depth_integrate_host(nullptr, &ok, d.get(), o.get()) == MPPI_ERR_INVALID_ARG);
        CHECK(mppi_depth_integrate_host(&f, nullptr, d.get(), o.get()) == MPPI_ERR_INVALID_ARG);
        CHECK(mppi_depth_integrate_host(&f, &ok, nullptr, o.get()) == MPPI_ERR_INVALID_ARG);
        CHECK(mppi_depth_integrate_host(&f, &ok, d.get(), nullptr) == MPPI_ERR_INVALID_ARG);
        mppi_depth_view v;
        v = ok; v.width = 0; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        v = ok; v.height = -3; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        v = ok; v.width = 1 << 11; v.height = 1 << 10; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        v = ok; v.width = 2147483647; v.height = 2147483647; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        v = ok; v.stride = 0; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        v = ok; v.stride = 2147483647; CHECK(st(v) == MPPI_OK);
        v = ok; v.carve = 2; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        for (const float x : {kNan, kInf, -kInf}) {
            float mppi_depth_view::* const m[] = {&mppi_depth_view::fx, &mppi_depth_view::fy, &mppi_depth_view::cx,
                                                  &mppi_depth_view::cy, &mppi_depth_view::z_min, &mppi_depth_view::z_max};
            for (const auto pm : m) { v = ok; v.*pm = x; CHECK(st(v) == MPPI_ERR_INVALID_ARG); ++n_checked; }
            for (int k = 0; k < 3; ++k) { v = ok; v.pos[k] = x; CHECK(st(v) == MPPI_ERR_INVALID_ARG); }
            for (int k = 0; k < 4; ++k) { v = ok; v.quat_xyzw[k] = x; CHECK(st(v) == MPPI_ERR_INVALID_ARG); }
        }
        v = ok; v.fx = 0.0f; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        v = ok; v.fy = -2.0f; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        v = ok; v.fx = 1e-45f; CHECK(st(v) == MPPI_ERR_INVALID_ARG);   // (its reciprocal is not finite)
        v = ok; v.z_min = -0.1f; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        v = ok; v.z_min = v.z_max; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        v = ok; v.z_max = 4097.0f * voxel; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        v = ok; for (float& q : v.quat_xyzw) q *= 0.5f; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        v = ok; for (float& q : v.quat_xyzw) q *= 2.0f; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        v = ok; for (float& q : v.quat_xyzw) q = 0.0f; CHECK(st(v) == MPPI_ERR_INVALID_ARG);
        for (int k = 0; k < 3; ++k) { v = ok; v.reserved[k] = 1; CHECK(st(v) == MPPI_ERR_INVALID_ARG); }
        ShiftParams p;
        float origin[3];
        const int32_t s[3] = {1, 2, 3};
        CHECK(shift_validate(f, nullptr, 0.0f, p, origin) == MPPI_ERR_INVALID_ARG);
        CHECK(shift_validate(f, s, kNan, p, origin) == MPPI_ERR_INVALID_ARG);
        CHECK(shift_validate(f, s, kInf, p, origin) == MPPI_ERR_INVALID_ARG);
        CHECK(shift_validate(f, s, -kInf, p, origin) == MPPI_OK);
        mppi_field_desc big = f;
        big.voxel = 3e37f;
        const int32_t far[3] = {2147483647, 0, 0};
        CHECK(shift_validate(big, far, 0.0f, p, origin) == MPPI_ERR_INVALID_ARG);
        n_checked += 40;
    }
    std::printf("%s: %d checks, %d failed\n", fails ? "FAILED" : "ok", n_checked, fails);
    return fails ? 1 : 0;
}
