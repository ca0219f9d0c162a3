// self_collision_host_check.cpp -- the host code of the self-collision pairs (mppi_create_scene_self) as a
// stand-alone program for the sanitizers (tools/, not shipped).  No GPU, no Python:
//
//   cd quadrotor_manipulator_mppi_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I . -I ../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Xarch_host -fno-omit-frame-pointer \
//       ../../tools/self_collision_host_check.cpp mppi_layout.cpp mppi_host_math.cpp -o ../../tools/_bin/self_collision_host_check
//   ../../tools/_bin/self_collision_host_check
//
// Validation: every error of mppi_create_scene_self's pair list (model, n_pairs, indices, a = b, a repeated
// pair, rigid pairs across leading and trailing fixed joints, weights) and the default pairs.  The table: a
// body out of frame order with all 16 spheres, 32 pairs; the member indices must follow the body table's
// sort order, every row must name its two spheres' members and the sum of their radii, and nothing may
// be written past the region.  The block rule: self_layout's choice for 2 and 16 members and its
// refusals.  The pair arithmetic: a host replay of the kernels' own inlines (obs_frame_self into a
// column, self_pairs, self_step_cost) over a small grid of joint vectors against a direct formula in
// double.  The restated frame loops: obs_frame, obs_frame_field and obs_frame_self with 16 moving obstacles and a
// set field must give the same hinge sums and clearances bit for bit.  Exit status 0 and a count line when all hold.
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
    for (int j = 0; j < 11; ++j) {
        mppi_joint& J = c.joints[j];
        J.q_index = -1;
        if (j < 3) {
            J.type = MPPI_JOINT_FIXED;
            J.xyz[2] = 0.1f * (float)(j + 1); J.rpy[0] = 0.3f * (float)j;
        } else if (j < 10) {
            J.type = MPPI_JOINT_REVOLUTE; J.q_index = j - 3; J.has_axis = 1; J.axis[2] = 1.0f;
            J.xyz[2] = -0.05f * (float)(j - 2); J.rpy[0] = 0.5f * (float)(j - 6);
        } else {
            J.type = MPPI_JOINT_FIXED; J.xyz[1] = 0.07f;
        }
    }
}

// T <- T * (O * Rz(q)) for 3x4 row-major transforms, in float as the kernels hold them
static void joint_step(float* T, const float* O, float q, bool revolute) {
    float M[12], R[12];
    const float c = std::cos(q), s = std::sin(q);
    for (int i = 0; i < 3; ++i) {   // M = O * Rz
        M[4 * i] = revolute ? O[4 * i] * c + O[4 * i + 1] * s : O[4 * i];
        M[4 * i + 1] = revolute ? O[4 * i + 1] * c - O[4 * i] * s : O[4 * i + 1];
        M[4 * i + 2] = O[4 * i + 2];
        M[4 * i + 3] = O[4 * i + 3];
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j)
            R[4 * i + j] = T[4 * i] * M[j] + T[4 * i + 1] * M[4 + j] + T[4 * i + 2] * M[8 + j] + (j == 3 ? T[4 * i + 3] : 0.0f);
    std::memcpy(T, R, sizeof(R));
}

int main() {
    int n_checked = 0;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    mppi_config c;
    mppi_config_default(&c, MPPI_MODEL_ARM);
    c.n_samples = 64;
    chain(c);
    CHECK(validate(c) == MPPI_OK);
    mppi_scene s;
    mppi_scene_default(&s, &c);
    CHECK(s.n_body == 7);   // frames 3..9
    // ---- validation
    {
        mppi_self_collision d;
        mppi_self_collision_default(&d, &c, &s);
        CHECK(d.n_pairs == 10 && d.w_self == 100.0f && d.margin == 0.02f && d.penalty == 1e4f);
        CHECK(d.pair[0][0] == 0 && d.pair[0][1] == 3 && d.pair[9][0] == 3 && d.pair[9][1] == 6);
        CHECK(self_validate(c, s, &d) == MPPI_OK);
        CHECK(self_validate(c, s, nullptr) == MPPI_ERR_INVALID_ARG);
        mppi_self_collision b = d;
        b.n_pairs = 33; CHECK(self_validate(c, s, &b) == MPPI_ERR_INVALID_ARG);
        b.n_pairs = -1; CHECK(self_validate(c, s, &b) == MPPI_ERR_INVALID_ARG);
        b = d; b.n_pairs = 0; CHECK(self_validate(c, s, &b) == MPPI_OK);
        b = d; b.pair[2][1] = 7; CHECK(self_validate(c, s, &b) == MPPI_ERR_INVALID_ARG);
        b = d; b.pair[2][0] = -1; CHECK(self_validate(c, s, &b) == MPPI_ERR_INVALID_ARG);
        b = d; b.pair[4][0] = b.pair[4][1]; CHECK(self_validate(c, s, &b) == MPPI_ERR_INVALID_ARG);
        b = d; b.pair[5][0] = d.pair[1][1]; b.pair[5][1] = d.pair[1][0]; CHECK(self_validate(c, s, &b) == MPPI_ERR_INVALID_ARG);
        b = d; b.w_self = -1.0f; CHECK(self_validate(c, s, &b) == MPPI_ERR_INVALID_ARG);
        b = d; b.margin = nan; CHECK(self_validate(c, s, &b) == MPPI_ERR_INVALID_ARG);
        b = d; b.penalty = std::numeric_limits<float>::infinity(); CHECK(self_validate(c, s, &b) == MPPI_ERR_INVALID_ARG);
        // rigid pairs: the base and the leading fixed joints' frames; the last moving joint's frame and the trailing fixed one's
        mppi_scene r = s;
        r.n_body = 6;
        const int fr[6] = {-1, 0, 2, 3, 9, 10};
        for (int i = 0; i < 6; ++i) r.body[i].frame = fr[i];
        CHECK(scene_validate(c, r) == MPPI_OK);
        CHECK(self_sep(c, -1, 2) == 0 && self_sep(c, 2, -1) == 0 && self_sep(c, 9, 10) == 0 && self_sep(c, 2, 3) == 1 && self_sep(c, -1, 10) == 7);
        b = d; b.n_pairs = 1;
        const int rigid[3][2] = {{0, 1}, {1, 2}, {4, 5}}, moving[3][2] = {{2, 3}, {0, 5}, {3, 4}};
        for (const auto& p : rigid) { b.pair[0][0] = p[0]; b.pair[0][1] = p[1]; CHECK(self_validate(c, r, &b) == MPPI_ERR_INVALID_ARG); }
        for (const auto& p : moving) { b.pair[0][0] = p[0]; b.pair[0][1] = p[1]; CHECK(self_validate(c, r, &b) == MPPI_OK); }
        mppi_config dr;
        mppi_config_default(&dr, MPPI_MODEL_DRONE);
        mppi_scene ds;
        mppi_scene_default(&ds, &dr);
        b = d; b.n_pairs = 0; CHECK(self_validate(dr, ds, &b) == MPPI_ERR_INVALID_ARG);
        mppi_self_collision_default(&b, &dr, nullptr); CHECK(b.n_pairs == 0);
        n_checked += 28;
    }
    // ---- the table
    mppi_scene s16 = s;
    const int frames[16] = {9, -1, 4, 3, 7, 5, 6, 6, 8, 1, 4, 10, 3, 9, 5, 7};
    s16.n_body = 16;
    for (int b = 0; b < 16; ++b) {
        s16.body[b].frame = frames[b];
        s16.body[b].offset[0] = 0.01f * (float)(b + 1); s16.body[b].offset[1] = -0.02f * (float)(b % 5); s16.body[b].offset[2] = 0.03f * (float)(b % 3) - 0.01f;
        s16.body[b].radius = 0.02f + 0.005f * (float)b;
    }
    CHECK(scene_validate(c, s16) == MPPI_OK);
    mppi_self_collision p32;
    std::memset(&p32, 0, sizeof(p32));
    p32.w_self = 50.0f; p32.margin = 0.03f; p32.penalty = 123.0f;
    for (int a = 0; a < 16 && p32.n_pairs < 32; ++a)
        for (int b = a + 1; b < 16 && p32.n_pairs < 32; ++b)
            if (self_sep(c, frames[a], frames[b]) >= 2 && (a + b) % 3 != 1) { p32.pair[p32.n_pairs][0] = b; p32.pair[p32.n_pairs][1] = a; ++p32.n_pairs; }
    CHECK(p32.n_pairs == 32 && self_validate(c, s16, &p32) == MPPI_OK);
    EngineLayout l;
    const int members = self_member_count(p32);
    CHECK(self_layout(c, members, l) == MPPI_OK);
    std::vector<float> table(kSceneBodyW), region(kSelfHdrW + 8, -777.0f);
    int order[16];
    scene_body_table(l, s16, table.data(), order);
    CHECK(self_table(l, s16, p32, order, region.data()) == members);
    for (int i = kSelfHdrW; i < kSelfHdrW + 8; ++i) CHECK(region[i] == -777.0f);
    CHECK(word(&region[0]) == 32 && region[1] == 50.0f && region[2] == 0.03f && region[3] == 123.0f && word(&region[4]) == members);
    CHECK(word(&region[5]) == (int)self_clr_off(l.V, l.K, l.H) && word(&region[6]) == (int)self_plan_off(l.V, l.K, l.H));
    CHECK(self_off(l.V, l.K, l.H) == scene_words(l.V, l.K, l.H) && self_words(l.V, l.K, l.H) > self_plan_off(l.V, l.K, l.H));
    {
        int next = 0, pos[16];
        for (int n = 0; n < 16; ++n) pos[order[n]] = n;
        for (int n = 0; n < 16; ++n) {
            bool used = false;
            for (int i = 0; i < 32; ++i) used = used || p32.pair[i][0] == order[n] || p32.pair[i][1] == order[n];
            CHECK(word(&region[kSelfMem + n]) == (used ? next : -1));
            next += used;
        }
        CHECK(next == members && members <= kSelfMaxMembers);
        for (int i = 0; i < 32; ++i) {
            const float* r = &region[kSelfPair + 3 * i];
            CHECK(word(r) == word(&region[kSelfMem + pos[p32.pair[i][0]]]) && word(r + 1) == word(&region[kSelfMem + pos[p32.pair[i][1]]]));
            CHECK(word(r) >= 0 && word(r + 1) >= 0 && word(r) != word(r + 1));
            CHECK(r[2] == s16.body[p32.pair[i][0]].radius + s16.body[p32.pair[i][1]].radius);
            ++n_checked;
        }
    }
    // ---- the block rule
    {
        EngineLayout a;
        mppi_config k = c;
        CHECK(self_layout(k, 2, a) == MPPI_OK && a.threads == 256);
        CHECK(self_dyn_lds(a.A, a.H, a.threads, a.dp.iters, 2) + kSelfStaticLds <= kSelfLdsTarget);
        CHECK(self_layout(k, 16, a) == MPPI_OK && a.threads == 128);
        k.block_threads = 512; CHECK(self_layout(k, 2, a) == MPPI_ERR_INVALID_ARG);
        k.block_threads = 256; CHECK(self_layout(k, 16, a) == MPPI_ERR_INVALID_ARG);
        k.block_threads = 256; CHECK(self_layout(k, 9, a) == MPPI_OK && a.threads == 256);
        k.block_threads = 64; CHECK(self_layout(k, 16, a) == MPPI_OK && a.threads == 64);
        k = c; k.n_horizon = 200; CHECK(self_layout(k, 16, a) == MPPI_OK && a.threads == 64);
        CHECK(self_dyn_lds(a.A, a.H, 64, a.dp.iters, 16) + kSelfStaticLds <= kSelfLdsMax);
        n_checked += 9;
    }
    // ---- the pair arithmetic: the kernels' inlines on the host over a grid of joint vectors
    {
        float body[kSceneBodyW], veh[kSceneObsW] = {0};
        std::memcpy(body, table.data(), sizeof(body));
        std::vector<float> col(3 * kSelfMaxMembers + 4, -777.0f);
        for (int g = 0; g < 27; ++g) {
            const float q[7] = {0.4f * (float)(g % 3 - 1), 0.7f * (float)(g / 3 % 3 - 1), 1.1f * (float)(g / 9 - 1), 0.9f, -0.6f + 0.1f * (float)g,
                                0.3f, -1.2f};
            float T[12] = {1.0f, 0.0f, 0.0f, 0.1f, 0.0f, 1.0f, 0.0f, -0.2f, 0.0f, 0.0f, 1.0f, 0.9f};
            float Tb[12];
            for (int i = 0; i < 3; ++i)   // the folded base: T * fixedM
                for (int j = 0; j < 4; ++j)
                    Tb[4 * i + j] = T[4 * i] * l.fixedM[j] + T[4 * i + 1] * l.fixedM[4 + j] + T[4 * i + 2] * l.fixedM[8 + j] + (j == 3 ? T[4 * i + 3] : 0.0f);
            std::memcpy(T, Tb, sizeof(T));
            double ctr[16][3];   // by sorted position, in double from the same transforms
            float hinge = 0.0f, gmin = INFINITY, oh = 0.0f, og = INFINITY;
            for (int slot = 0; slot <= c.n_joints - l.dp.j0; ++slot) {
                if (slot > 0) {
                    const int j = l.dp.j0 + slot - 1;
                    joint_step(T, l.joints[j].O, c.joints[j].q_index >= 0 ? q[c.joints[j].q_index] : 0.0f, c.joints[j].type == MPPI_JOINT_REVOLUTE);
                }
                for (int b = word(&body[kSceneRng + slot]); b < word(&body[kSceneRng + slot + 1]); ++b)
                    for (int d = 0; d < 3; ++d) {
                        const float* sp = body + kSceneSph + 4 * b;
                        ctr[b][d] = (double)T[4 * d] * sp[0] + (double)T[4 * d + 1] * sp[1] + (double)T[4 * d + 2] * sp[2] + (double)T[4 * d + 3];
                    }
                obs_frame_self<false>(T, body, veh, slot, 0.01f, nullptr, nullptr, region.data(), col.data(), 1, oh, og);
            }
            CHECK(oh == 0.0f && std::isinf(og));   // no obstacles
            for (int i = 3 * members; i < 3 * kSelfMaxMembers + 4; ++i) CHECK(col[i] == -777.0f);
            self_pairs(region.data(), col.data(), 1, hinge, gmin);
            double hs = 0.0, gm = INFINITY;
            int pos[16];
            for (int n = 0; n < 16; ++n) pos[order[n]] = n;
            for (int i = 0; i < 32; ++i) {
                const int a = pos[p32.pair[i][0]], b = pos[p32.pair[i][1]];
                double d2 = 0.0;
                for (int d = 0; d < 3; ++d) d2 += (ctr[a][d] - ctr[b][d]) * (ctr[a][d] - ctr[b][d]);
                const double gab = std::sqrt(d2) - (double)s16.body[p32.pair[i][0]].radius - (double)s16.body[p32.pair[i][1]].radius;
                hs += std::fmax(0.0, 0.03 - gab);
                gm = std::fmin(gm, gab);
            }
            CHECK(std::fabs(hinge - hs) < 1e-4);
            CHECK(std::fabs(gmin - gm) < 1e-5);
            CHECK(std::fabs(self_step_cost(region.data(), hinge, gmin) - (50.0 * hs + (gm < 0.0 ? 123.0 : 0.0))) < 1e-2);
            ++n_checked;
        }
    }
    // ---- the three restated frame loops stay in step: obs_frame, obs_frame_field and obs_frame_self over the same
    // slots with 16 moving obstacles and a set field give the same hinge sums and clearances bit for bit
    {
        float body[kSceneBodyW];
        std::memcpy(body, table.data(), sizeof(body));
        body[1] = 100.0f; body[2] = 0.05f; body[3] = 1e4f;
        std::vector<float> oc(48), orad(16), ov(48), veh(kSceneObsW);
        for (int o = 0; o < 16; ++o) {
            orad[o] = 0.04f + 0.01f * (float)o;
            for (int d = 0; d < 3; ++d) { oc[3 * o + d] = 0.15f * (float)(o % 5 - 2) + 0.2f * (float)d; ov[3 * o + d] = 0.3f * (float)(d - 1) * (float)(o % 3); }
        }
        obstacles_fill(veh.data(), 16, oc.data(), orad.data(), ov.data());
        mppi_field_desc fd;
        std::memset(&fd, 0, sizeof(fd));
        fd.dims[0] = 9; fd.dims[1] = 7; fd.dims[2] = 8; fd.voxel = 0.25f;
        fd.origin[0] = -1.0f; fd.origin[1] = -1.0f; fd.origin[2] = -0.5f;
        CHECK(field_validate(&fd) == MPPI_OK);
        std::vector<float> dz((size_t)field_voxels(fd)), words((size_t)field_words(field_voxels(fd)));
        for (size_t i = 0; i < dz.size(); ++i) dz[i] = 0.02f * (float)((int)(i * 7 % 23) - 6);   // some nodes inside
        field_header(fd, fd.origin, true, words.data());
        field_pack(fd, dz.data(), words.data() + kFieldHdrW);
        std::vector<float> col(3 * kSelfMaxMembers, 0.0f);
        int n_hinge = 0, n_field = 0;   // (the comparison must not be of zeros: some slots meet an obstacle, some the field)
        for (int g = 0; g < 8; ++g) {
            const float a = 0.35f * (float)g, ca = std::cos(a), sa = std::sin(a);
            const float T[12] = {ca, -sa, 0.0f, 0.1f * (float)g - 0.3f, sa, ca, 0.0f, 0.2f, 0.0f, 0.0f, 1.0f, 0.4f + 0.05f * (float)g};
            for (int slot = 0; slot < kSceneSlots; ++slot) {
                const float tau = 0.01f * (float)(g + 1);
                float h0 = 0.0f, g0 = INFINITY, h1 = 0.0f, g1 = INFINITY, h2 = 0.0f, g2 = INFINITY, h3 = 0.0f, g3 = INFINITY;
                obs_frame(T, body, veh.data(), slot, tau, h0, g0);
                obs_frame_self<false>(T, body, veh.data(), slot, tau, nullptr, nullptr, region.data(), col.data(), 1, h1, g1);
                obs_frame_field(T, body, veh.data(), slot, tau, words.data(), words.data() + kFieldHdrW, h2, g2);
                obs_frame_self<true>(T, body, veh.data(), slot, tau, words.data(), words.data() + kFieldHdrW, region.data(), col.data(), 1, h3, g3);
                CHECK(std::memcmp(&h0, &h1, 4) == 0 && std::memcmp(&g0, &g1, 4) == 0);
                CHECK(std::memcmp(&h2, &h3, 4) == 0 && std::memcmp(&g2, &g3, 4) == 0);
                if (word(&body[kSceneRng + slot]) < word(&body[kSceneRng + slot + 1])) {
                    CHECK(std::isfinite(g0) && std::isfinite(g2));
                    n_hinge += h0 > 0.0f;
                    n_field += (h2 != h0 || g2 != g0);
                }
                ++n_checked;
            }
        }
        CHECK(n_hinge > 0 && n_field > 0);
    }
    std::printf("%d checks made, %d failures\n", n_checked, fails);
    return fails ? 1 : 0;
}
