// target_track_host_check.cpp -- the host code of target tracking (MPPI_COST_TARGET_TRACK) as a
// stand-alone program for the sanitizers (tools/, not shipped).  No GPU, no Python:
//
//   cd quadrotor_manipulator_mppi_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I . -I ../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Xarch_host -fno-omit-frame-pointer \
//       ../../tools/target_track_host_check.cpp mppi_layout.cpp mppi_host_math.cpp -o ../../tools/_bin/target_track_host_check
//   ../../tools/_bin/target_track_host_check
//
// Config validation: bit 32 of cost_terms on all four models, bits 1..16 refused on DRONE and
// QUADROTOR with and without it, bits above 32 refused, and layout_of under the bit alone (no
// CostManager tables).  Row conversion: a (V, H, 12) table filled as the engine fills it -- p*(3) then
// R* = quat_xyzw_to_R(q*_t) -- from unit and scaled quaternions; R* must not depend on the scale
// (rotation_conversions.py:45-75 divides by |q|^2) and must be orthonormal.  Exit status 0 and a
// count line when all hold (and the sanitizers stayed silent).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mppi_layout.h"

using namespace mppi_host;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s (line %d)\n", #x, __LINE__); ++fails; } } while (0)

// the Kinova j2s7s300 chain behind one fixed mount (tools/layout_host_check.cpp)
static void kinova(mppi_config& c) {
    const float pi = 3.14159265358979f, h = pi / 2;
    const float rpy[7][3] = {{0, pi, 0}, {-h, 0, pi}, {-h, 0, 0}, {h, 0, pi}, {-h, 0, pi}, {h, 0, pi}, {-h, 0, pi}};
    const float xyz[7][3] = {{0, 0, .15675f}, {0, .0016f, -.11875f}, {0, -.205f, 0}, {0, 0, -.205f},
                             {0, .2073f, -.0114f}, {0, 0, -.10375f}, {0, .10375f, 0}};
    c.n_joints = 8;
    std::memset(c.joints, 0, sizeof(c.joints));
    c.joints[0].type = MPPI_JOINT_FIXED; c.joints[0].q_index = -1; c.joints[0].xyz[2] = 0.1f;
    for (int j = 0; j < 7; ++j) {
        mppi_joint& J = c.joints[1 + j];
        J.type = MPPI_JOINT_REVOLUTE; J.q_index = j; J.has_axis = 1; J.axis[2] = 1.0f;
        std::memcpy(J.rpy, rpy[j], sizeof(J.rpy));
        std::memcpy(J.xyz, xyz[j], sizeof(J.xyz));
    }
}

int main() {
    const int models[4] = {MPPI_MODEL_DRONE, MPPI_MODEL_ARM, MPPI_MODEL_WHOLEBODY, MPPI_MODEL_QUADROTOR};
    int n = 0;
    for (int m : models) {
        const bool vehicle = m == MPPI_MODEL_DRONE || m == MPPI_MODEL_QUADROTOR;
        for (int bits = 0; bits < 256; ++bits) {
            mppi_config c;
            mppi_config_default(&c, m);
            c.n_samples = 64;
            if (!vehicle) kinova(c);
            c.cost_terms = bits;
            const bool want = !(bits & ~0x3F) && !(vehicle && (bits & 0x1F));
            const mppi_status st = validate(c);
            CHECK((st == MPPI_OK) == want);
            if (st != MPPI_OK) continue;
            EngineLayout l;
            CHECK(layout_of(c, l) == MPPI_OK);
            CHECK(l.dp.cost_terms == bits);
            // the CostManager tables exist with the CostManager bits only
            CHECK(l.sinv.empty() == !(bits & 0x1F) && l.gamma_t.empty() == !(bits & 0x1F));
            ++n;
        }
    }
    // the table's rows, as mppi_set_target_trajectory fills them
    const int V = 3, H = 200;
    std::vector<float> tab((size_t)V * H * 12), pos((size_t)H * 3), quat((size_t)H * 4);
    for (int v = 0; v < V; ++v) {
        for (int t = 0; t < H; ++t) {
            const float a = 0.01f * (float)(t + 1) * (float)(v + 1), s = (t % 5 == 3) ? 0.5f : (t % 7 == 6) ? 2.0f : 1.0f;
            pos[3 * t] = a; pos[3 * t + 1] = -a; pos[3 * t + 2] = 1.0f + a;
            const float q[4] = {std::sin(a) * 0.6f, std::sin(a) * 0.0f, std::sin(a) * 0.8f, std::cos(a)};
            for (int i = 0; i < 4; ++i) quat[4 * t + i] = s * q[i];
            float* row = &tab[((size_t)v * H + t) * 12];
            std::memcpy(row, &pos[3 * t], 3 * sizeof(float));
            quat_xyzw_to_R(&quat[4 * t], row + 3);
            float Ru[9];
            quat_xyzw_to_R(q, Ru);
            for (int i = 0; i < 9; ++i) CHECK(std::fabs(Ru[i] - row[3 + i]) < 1e-6f);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    float d = 0.0f;
                    for (int k = 0; k < 3; ++k) d += row[3 + 3 * i + k] * row[3 + 3 * j + k];
                    CHECK(std::fabs(d - (i == j ? 1.0f : 0.0f)) < 1e-5f);
                }
        }
    }
    std::printf("%d accepted configurations, %d rows converted, %d failures\n", n, V * H, fails);
    return fails ? 1 : 0;
}
