// obstacle_host_check.cpp -- the host code of the sphere scene (mppi_create_scene, mppi_set_obstacles) as
// a stand-alone program for the sanitizers (tools/, not shipped).  No GPU, no Python:
//
//   cd quadrotor_manipulator_mppi_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I . -I ../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Xarch_host -fno-omit-frame-pointer \
//       ../../tools/obstacle_host_check.cpp mppi_layout.cpp mppi_host_math.cpp -o ../../tools/_bin/obstacle_host_check
//   ../../tools/_bin/obstacle_host_check
//
// Scene validation: every error of mppi_create_scene (model, n_body, frames, non-finite values, radii,
// weights) and the default scenes.  Frame folding and sorting: a chain with three leading fixed joints
// (rotated and translated), spheres on every frame from -1 up; the body table's slot ranges must be
// ascending and cover the spheres in stable order, and the world centre of every folded sphere --
// folded base times the table's offset -- must equal the unfolded chain product times the caller's
// offset, in double, to 1e-6 m.  The staging fill: obstacle blocks for n = 0, 1, 16 with and without
// velocities, the errors of mppi_set_obstacles, and the pair arithmetic of mppi_obstacles.h on the
// host against a direct formula.  Exit status 0 and a count line when all hold.
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

static int word(const float* p) {
    int32_t i;
    std::memcpy(&i, p, sizeof(i));
    return i;
}

// three leading fixed joints, then seven revolute-z joints and a trailing fixed one
static void chain(mppi_config& c) {
    c.n_joints = 11;
    std::memset(c.joints, 0, sizeof(c.joints));
    const float xyz[3][3] = {{0.0f, 0.0f, 0.1f}, {0.05f, -0.02f, 0.2f}, {-0.1f, 0.3f, 0.0f}};
    const float rpy[3][3] = {{0.3f, -0.2f, 1.1f}, {-1.57079633f, 0.0f, 0.4f}, {0.0f, 0.7f, -0.9f}};
    for (int j = 0; j < 11; ++j) {
        mppi_joint& J = c.joints[j];
        J.q_index = -1;
        if (j < 3) {
            J.type = MPPI_JOINT_FIXED;
            std::memcpy(J.xyz, xyz[j], sizeof(J.xyz));
            std::memcpy(J.rpy, rpy[j], sizeof(J.rpy));
        } else if (j < 10) {
            J.type = MPPI_JOINT_REVOLUTE; J.q_index = j - 3; J.has_axis = 1; J.axis[2] = 1.0f;
            J.xyz[2] = -0.05f * (float)(j - 2); J.rpy[0] = 0.5f * (float)(j - 6);
        } else {
            J.type = MPPI_JOINT_FIXED; J.xyz[1] = 0.07f;
        }
    }
}

// p <- O p for a 3x4 row-major transform, in double
static void apply(const float* O, double* p) {
    double r[3];
    for (int i = 0; i < 3; ++i) r[i] = (double)O[4 * i] * p[0] + (double)O[4 * i + 1] * p[1] + (double)O[4 * i + 2] * p[2] + (double)O[4 * i + 3];
    std::memcpy(p, r, sizeof(r));
}

int main() {
    int n_checked = 0;
    // ---- validation
    for (int m : {MPPI_MODEL_DRONE, MPPI_MODEL_ARM, MPPI_MODEL_WHOLEBODY, MPPI_MODEL_QUADROTOR}) {
        mppi_config c;
        mppi_config_default(&c, m);
        c.n_samples = 64;
        if (m == MPPI_MODEL_ARM || m == MPPI_MODEL_WHOLEBODY) chain(c);
        mppi_scene s;
        mppi_scene_default(&s, &c);
        CHECK(s.w_obs == 100.0f && s.margin == 0.05f && s.penalty == 1e4f);
        if (m == MPPI_MODEL_QUADROTOR) {
            CHECK(scene_validate(c, s) == MPPI_ERR_INVALID_ARG);
            continue;
        }
        CHECK(scene_validate(c, s) == MPPI_OK);
        CHECK(s.n_body == (m == MPPI_MODEL_DRONE ? 1 : m == MPPI_MODEL_ARM ? 7 : 8));
        const int nj = m == MPPI_MODEL_DRONE ? 0 : c.n_joints;
        mppi_scene b = s;
        b.n_body = 17; CHECK(scene_validate(c, b) == MPPI_ERR_INVALID_ARG);
        b.n_body = -1; CHECK(scene_validate(c, b) == MPPI_ERR_INVALID_ARG);
        b = s; b.body[0].frame = nj; CHECK(scene_validate(c, b) == MPPI_ERR_INVALID_ARG);
        b = s; b.body[0].frame = -2; CHECK(scene_validate(c, b) == MPPI_ERR_INVALID_ARG);
        if (nj) { b = s; b.body[0].frame = nj - 1; CHECK(scene_validate(c, b) == MPPI_OK); }
        b = s; b.body[0].radius = 0.0f; CHECK(scene_validate(c, b) == MPPI_ERR_INVALID_ARG);
        b = s; b.body[0].radius = -0.1f; CHECK(scene_validate(c, b) == MPPI_ERR_INVALID_ARG);
        b = s; b.body[0].radius = std::numeric_limits<float>::quiet_NaN(); CHECK(scene_validate(c, b) == MPPI_ERR_INVALID_ARG);
        b = s; b.body[0].offset[1] = std::numeric_limits<float>::infinity(); CHECK(scene_validate(c, b) == MPPI_ERR_INVALID_ARG);
        b = s; b.w_obs = -1.0f; CHECK(scene_validate(c, b) == MPPI_ERR_INVALID_ARG);
        b = s; b.margin = -0.01f; CHECK(scene_validate(c, b) == MPPI_ERR_INVALID_ARG);
        b = s; b.penalty = std::numeric_limits<float>::quiet_NaN(); CHECK(scene_validate(c, b) == MPPI_ERR_INVALID_ARG);
        b = s; b.n_body = 0; CHECK(scene_validate(c, b) == MPPI_OK);
        n_checked += 14;
    }
    // ---- folding and sorting
    {
        mppi_config c;
        mppi_config_default(&c, MPPI_MODEL_ARM);
        c.n_samples = 64;
        chain(c);
        CHECK(validate(c) == MPPI_OK);
        EngineLayout l;
        CHECK(layout_of(c, l) == MPPI_OK);
        CHECK(l.dp.j0 == 3);
        mppi_scene s;
        mppi_scene_default(&s, &c);
        // out of frame order on purpose, two spheres on one frame, all 16 used
        const int frames[16] = {7, -1, 2, 0, 5, 1, 3, 3, 6, -1, 4, 2, 0, 7, 1, 5};
        s.n_body = 16;
        for (int b = 0; b < 16; ++b) {
            s.body[b].frame = frames[b];
            s.body[b].offset[0] = 0.01f * (float)(b + 1); s.body[b].offset[1] = -0.02f * (float)(b % 5); s.body[b].offset[2] = 0.03f * (float)(b % 3) - 0.01f;
            s.body[b].radius = 0.02f + 0.005f * (float)b;
        }
        CHECK(scene_validate(c, s) == MPPI_OK);
        std::vector<float> table(kSceneBodyW + 8, -777.0f);   // (a guard past the table)
        int order[16];
        scene_body_table(l, s, table.data(), order);
        for (int i = kSceneBodyW; i < kSceneBodyW + 8; ++i) CHECK(table[i] == -777.0f);
        CHECK(word(&table[0]) == 16 && table[1] == s.w_obs && table[2] == s.margin && table[3] == s.penalty);
        CHECK(word(&table[4]) == (int)scene_clr_off(l.V) && word(&table[5]) == (int)scene_plan_off(l.V, l.K) && word(&table[6]) == l.K);
        CHECK(word(&table[kSceneRng]) == 0 && word(&table[kSceneRng + kSceneSlots]) == 16);
        int seen = 0;
        for (int sl = 0; sl < kSceneSlots; ++sl) {
            const int b0 = word(&table[kSceneRng + sl]), b1 = word(&table[kSceneRng + sl + 1]);
            CHECK(b0 <= b1 && b0 == seen);
            for (int i = b0; i < b1; ++i) {
                const int b = order[i], want = frames[b] < 3 ? 0 : frames[b] - 3 + 1;
                CHECK(want == sl);
                if (i > b0) CHECK(order[i - 1] < b);   // stable
                CHECK(table[kSceneSph + 4 * i + 3] == s.body[b].radius);
                // unfolded: O_0 .. O_f (o, 1); folded: O_0 O_1 O_2 (o', 1)
                double pu[3] = {s.body[b].offset[0], s.body[b].offset[1], s.body[b].offset[2]};
                for (int j = frames[b] < 3 ? frames[b] : -1; j >= 0; --j) apply(l.joints[j].O, pu);
                double pf[3] = {table[kSceneSph + 4 * i], table[kSceneSph + 4 * i + 1], table[kSceneSph + 4 * i + 2]};
                if (sl == 0) {
                    for (int j = 2; j >= 0; --j) apply(l.joints[j].O, pf);
                    for (int d = 0; d < 3; ++d) CHECK(std::fabs(pf[d] - pu[d]) < 1e-6);
                } else {
                    for (int d = 0; d < 3; ++d) CHECK(table[kSceneSph + 4 * i + d] == s.body[b].offset[d]);
                }
                ++n_checked;
            }
            seen = b1;
        }
        CHECK(seen == 16);
        // the same product through the folded base the engine uses (fixedM), in float: 1e-6 m as well
        for (int i = word(&table[kSceneRng]); i < word(&table[kSceneRng + 1]); ++i) {
            const int b = order[i];
            double pu[3] = {s.body[b].offset[0], s.body[b].offset[1], s.body[b].offset[2]};
            for (int j = frames[b]; j >= 0; --j) apply(l.joints[j].O, pu);
            double pf[3] = {table[kSceneSph + 4 * i], table[kSceneSph + 4 * i + 1], table[kSceneSph + 4 * i + 2]};
            apply(l.fixedM, pf);
            for (int d = 0; d < 3; ++d) CHECK(std::fabs(pf[d] - pu[d]) < 1e-6);
        }
    }
    // ---- the obstacle blocks and the pair arithmetic
    {
        const float nan = std::numeric_limits<float>::quiet_NaN();
        std::vector<float> c(48), r(16), v(48);
        for (int o = 0; o < 16; ++o) {
            r[o] = 0.05f + 0.01f * (float)o;
            for (int d = 0; d < 3; ++d) { c[3 * o + d] = 0.1f * (float)(o - 8) + 0.3f * (float)d; v[3 * o + d] = 0.2f * (float)(d - 1) * (float)(o % 3); }
        }
        CHECK(obstacles_validate(2, 0, 16, c.data(), r.data(), v.data()) == MPPI_OK);
        CHECK(obstacles_validate(2, 1, 0, nullptr, nullptr, nullptr) == MPPI_OK);
        CHECK(obstacles_validate(2, 2, 1, c.data(), r.data(), nullptr) == MPPI_ERR_INVALID_ARG);
        CHECK(obstacles_validate(2, -1, 1, c.data(), r.data(), nullptr) == MPPI_ERR_INVALID_ARG);
        CHECK(obstacles_validate(2, 0, 17, c.data(), r.data(), nullptr) == MPPI_ERR_INVALID_ARG);
        CHECK(obstacles_validate(2, 0, -1, c.data(), r.data(), nullptr) == MPPI_ERR_INVALID_ARG);
        CHECK(obstacles_validate(2, 0, 1, nullptr, r.data(), nullptr) == MPPI_ERR_INVALID_ARG);
        { auto r2 = r; r2[3] = 0.0f; CHECK(obstacles_validate(2, 0, 16, c.data(), r2.data(), nullptr) == MPPI_ERR_INVALID_ARG);
          CHECK(obstacles_validate(2, 0, 3, c.data(), r2.data(), nullptr) == MPPI_OK); }
        { auto c2 = c; c2[10] = nan; CHECK(obstacles_validate(2, 0, 16, c2.data(), r.data(), nullptr) == MPPI_ERR_INVALID_ARG); }
        { auto v2 = v; v2[47] = nan; CHECK(obstacles_validate(2, 0, 16, c.data(), r.data(), v2.data()) == MPPI_ERR_INVALID_ARG); }
        for (int n : {0, 1, 16})
            for (int with_v = 0; with_v < 2; ++with_v) {
                std::vector<float> block(kSceneObsW + 4, -777.0f);
                obstacles_fill(block.data(), n, c.data(), r.data(), with_v ? v.data() : nullptr);
                for (int i = kSceneObsW; i < kSceneObsW + 4; ++i) CHECK(block[i] == -777.0f);
                CHECK(word(block.data()) == n);
                for (int o = 0; o < 16; ++o) {
                    const float* row = block.data() + 4 + 8 * o;
                    for (int d = 0; d < 3; ++d) {
                        CHECK(row[d] == (o < n ? c[3 * o + d] : 0.0f));
                        CHECK(row[4 + d] == (o < n && with_v ? v[3 * o + d] : 0.0f));
                    }
                    CHECK(row[3] == (o < n ? r[o] : 0.0f));
                }
                // one frame's spheres against the block: obs_frame on the host against the formula
                float body[kSceneBodyW] = {0};
                const int32_t rng[2] = {0, 2};
                std::memcpy(body + kSceneRng, &rng[0], 4); std::memcpy(body + kSceneRng + 1, &rng[1], 4);
                body[1] = 100.0f; body[2] = 0.05f; body[3] = 1e4f;
                const float sph[8] = {0.1f, -0.2f, 0.3f, 0.05f, 0.0f, 0.0f, 0.0f, 0.07f};
                std::memcpy(body + kSceneSph, sph, sizeof(sph));
                const float T[12] = {0.0f, -1.0f, 0.0f, 0.2f, 1.0f, 0.0f, 0.0f, -0.1f, 0.0f, 0.0f, 1.0f, 0.4f};
                float hinge = 0.0f, gmin = INFINITY;
                const float tau = 0.07f;
                obs_frame(T, body, block.data(), 0, tau, hinge, gmin);
                double hs = 0.0, gm = INFINITY;
                for (int b = 0; b < 2; ++b) {
                    const double ctr[3] = {0.2 - sph[4 * b + 1], -0.1 + sph[4 * b], 0.4 + sph[4 * b + 2]};
                    for (int o = 0; o < n; ++o) {
                        double d2 = 0.0;
                        for (int d = 0; d < 3; ++d) {
                            const double x = ctr[d] - ((double)c[3 * o + d] + (with_v ? (double)v[3 * o + d] : 0.0) * tau);
                            d2 += x * x;
                        }
                        const double g = std::sqrt(d2) - sph[4 * b + 3] - r[o];
                        hs += std::fmax(0.0, 0.05 - g);
                        gm = std::fmin(gm, g);
                    }
                }
                CHECK(std::fabs(hinge - hs) < 1e-5);
                CHECK(n == 0 ? std::isinf(gmin) : std::fabs(gmin - gm) < 1e-6);
                CHECK(std::fabs(obs_step_cost(body, hinge, gmin) - (100.0 * hs + (gm < 0.0 ? 1e4 : 0.0))) < 1e-2);
                ++n_checked;
            }
    }
    std::printf("%d checks made, %d failures\n", n_checked, fails);
    return fails ? 1 : 0;
}
