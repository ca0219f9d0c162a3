// layout_host_check.cpp -- layout_of (csrc/mppi_layout.cpp) over a sweep of configurations, as a
// stand-alone host program for the sanitizers (tools/, not shipped).  No GPU, no Python:
//
//   cd quadrotor_manipulator_mppi_amd/csrc && hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -I . -I ../../include \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Xarch_host -fno-omit-frame-pointer \
//       ../../tools/layout_host_check.cpp mppi_layout.cpp mppi_host_math.cpp -o ../../tools/_bin/layout_host_check
//   ../../tools/_bin/layout_host_check
//
// Every accepted layout is checked for what the kernels rely on: the blocks cover the samples, the
// cost run fits its LDS stage, the output buffer's parts are ordered and 16 B aligned.  Exit
// status 0 and a count line when all hold (and the sanitizers stayed silent).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mppi_layout.h"

using namespace mppi_host;

// the Kinova j2s7s300 chain behind one fixed mount (mppi_dev.h kKinova lists the origins)
static void kinova(mppi_config& c, bool tilt) {
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
    if (tilt) c.joints[3].axis[0] = 0.5f;
}

int main() {
    const int Ks[] = {1, 16, 77, 100, 4096, 8192, 65536, 1000000}, Hs[] = {2, 20, 32, 33, 64, 65, 100, 128, 129, 193, 256};
    const int Vs[] = {1, 3, 64, 256}, bts[] = {0, 64, 128, 256, 512}, bpvs[] = {0, 3, 8192};
    const char* envs[][2] = {{nullptr, nullptr}, {"MPPI_FIN_TSZ", "4"}, {"MPPI_NO_KINOVA_PATH", "1"},
                             {"MPPI_GENERIC_KERNELS", "1"}, {"MPPI_GENERIC_KERNELS", "quiet_rollout"}};
    long accepted = 0, refused = 0, kin = 0;
    for (const auto& env : envs) {
        if (env[0]) setenv(env[0], env[1], 1);
        for (int model = 0; model < 4; ++model)
            for (int K : Ks) for (int H : Hs) for (int V : Vs) for (int bt : bts) for (int bpv : bpvs)
                for (int variant = 0; variant < 4; ++variant) {   // plain; cost terms + full Sigma; singular Sigma; odd chain
                    mppi_config c;
                    mppi_config_default(&c, model);
                    c.n_samples = K; c.n_horizon = H; c.n_vehicles = V; c.block_threads = bt; c.blocks_per_vehicle = bpv;
                    if (H == 2) c.savgol_window = 3;
                    if (model == MPPI_MODEL_ARM || model == MPPI_MODEL_WHOLEBODY) kinova(c, variant == 3);
                    if (variant == 1 || variant == 2) {
                        c.cost_terms = (model == MPPI_MODEL_ARM || model == MPPI_MODEL_WHOLEBODY) ? 0x1F : 0;
                        for (int i = 0; i < c.n_action * c.n_action; ++i)
                            if (i % (c.n_action + 1)) c.sigma[i] = 0.01f;
                        if (variant == 2) std::memset(c.sigma, 0, sizeof(c.sigma));
                        c.shard_rank = 2; c.shard_count = 4; c.store_noise = 1;
                    }
                    EngineLayout l{};
                    if (validate(c) != MPPI_OK || layout_of(c, l) != MPPI_OK) { ++refused; continue; }
                    ++accepted;
                    kin += l.dp.chain_fast == 2;
                    const int per = model == MPPI_MODEL_QUADROTOR ? 16 : l.threads / 64 * l.dp.R;
                    const size_t o[5] = {off_u0(&l), off_stats(&l), off_flags(&l), off_xerr(&l), (size_t)l.out_bytes};
                    bool ok = l.dp.nb >= 1 && l.dp.nb <= 4096 && l.dp.iters >= 1 && (long)l.dp.nb * l.dp.iters * per >= K;
                    if (model != MPPI_MODEL_QUADROTOR) ok = ok && l.dp.iters * mppi::cost_run_stride(per) <= mppi::kMaxCostRun;
                    for (int i = 0; i < 4; ++i) ok = ok && o[i] % 16 == 0 && o[i] < o[i + 1];
                    ok = ok && o[3] + 16 == o[4] && l.fin_ts * l.fin_tsz >= H && l.dp.hp % 16 == 0;
                    ok = ok && (c.cost_terms ? (int)l.sinv.size() == l.A * l.A && (int)l.gamma_t.size() == H : l.sinv.empty());
                    if (!ok) {
                        fprintf(stderr, "bad layout: model %d K %d H %d V %d bt %d bpv %d variant %d\n", model, K, H, V, bt, bpv, variant);
                        return 1;
                    }
                }
        if (env[0]) unsetenv(env[0]);
    }
    printf("layout_host_check: %ld layouts accepted (%ld on the Kinova path), %ld refused\n", accepted, kin, refused);
    return accepted && refused && kin ? 0 : 1;
}
