// rollout_force_test.cpp — UavSwarm::rolloutForceDevice and applyForceDevice with plain hipMalloc'd rows: 1 000 UAVs take B = 6
// ATTITUDE_RATE_CMD row blocks, each held for 10 steps, a force row block every 5 steps (12 blocks) and report position, velocity and
// orientation every 20 steps (3 row blocks).  With every force block holding the same rows, the call must equal, bit for bit,
// applyForceDevice of those rows followed by rolloutRateDevice on a twin; with the gust sequence the rows must differ from the unforced
// twin's and the swarm must be left carrying the last force block.  The gust rows are written to argv[1] for
// tests/test_rollout_force_gpu.py to compare with mrs_multirotor_simulator_amd.tensors.rollout(forces=) of the same swarm.  Exit code 0
// and "ok ..." lines on success.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <mrs_multirotor_simulator/uav_system/uav_system.hpp>

using namespace mrs_multirotor_simulator;

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                  \
    }                                                            \
  } while (0)
#define HIP(c) CHECK((c) == hipSuccess)

int main(int argc, char** argv) {
  const int                    n = 1000, B = 6, HOLD = 10, EVERY = 20, FEVERY = 5, W = 10, FS = 4;  // W: POS | VEL | QUAT; FS: padded force rows
  const int                    steps = B * HOLD, rows = steps / EVERY, FB = steps / FEVERY;
  MultirotorModel::ModelParams mp;
  std::vector<Eigen::Vector3d> pos;
  std::vector<double>          hdg;
  std::vector<double>          cmd((size_t)B * n * 4), gust((size_t)FB * n * FS, -7.0), steady((size_t)FB * n * FS, -7.0);
  for (int i = 0; i < n; i++) {  // (the same expressions as test_rollout_force_gpu.test_cpp_facade_equals_python)
    pos.push_back(Eigen::Vector3d(4.0 * (i % 32), 4.0 * (i / 32), 5.0));
    hdg.push_back(0.003 * i);
    for (int j = 0; j < B; j++) {
      double* c = &cmd[((size_t)j * n + i) * 4];
      c[0] = 0.02 * std::sin(0.1 * j + 0.001 * i);
      c[1] = -0.01 + 0.0 * j + 0.0 * i;
      c[2] = 0.3 + 0.0001 * i + 0.0 * j;
      c[3] = 0.55 + 0.005 * j + 0.0 * i;
    }
    for (int j = 0; j < FB; j++) {
      double* f = &gust[((size_t)j * n + i) * FS];
      f[0] = 0.5 * (j % 5) - 1.0 + 0.004 * i;
      f[1] = -1.5 + 0.25 * j + 0.0 * i;
      f[2] = (j % 3 == 0) ? 0.0 : 0.002 * i - 1.0;
      double* g = &steady[((size_t)j * n + i) * FS];
      g[0] = 2.0 + 0.001 * i + 0.0 * j;
      g[1] = -1.0 + 0.0 * i + 0.0 * j;
      g[2] = 0.5 + 0.0 * i + 0.0 * j;
    }
  }
  UavSwarm sw(n), twin(n), calm(n), gusty(n);  // (sw and twin stay bit-identical twins throughout)
  for (UavSwarm* s : {&sw, &twin, &calm, &gusty}) s->construct(0, n, mp, pos, hdg);
  double *d_cmd = nullptr, *d_gust = nullptr, *d_steady = nullptr, *d_obs = nullptr, *d_twin = nullptr;
  HIP(hipMalloc((void**)&d_cmd, sizeof(double) * cmd.size()));
  HIP(hipMalloc((void**)&d_gust, sizeof(double) * ((size_t)(FB * n - 1) * FS + 3)));  // exactly sized: the last row has no padding
  HIP(hipMalloc((void**)&d_steady, sizeof(double) * steady.size()));
  HIP(hipMalloc((void**)&d_obs, sizeof(double) * (size_t)rows * n * W));
  HIP(hipMalloc((void**)&d_twin, sizeof(double) * (size_t)rows * n * W));
  HIP(hipMemcpy(d_cmd, cmd.data(), sizeof(double) * cmd.size(), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_gust, gust.data(), sizeof(double) * ((size_t)(FB * n - 1) * FS + 3), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_steady, steady.data(), sizeof(double) * steady.size(), hipMemcpyHostToDevice));
  const uint32_t      groups = MRS_OBS_POS | MRS_OBS_VEL | MRS_OBS_QUAT;
  std::vector<double> obs((size_t)rows * n * W), ref((size_t)rows * n * W), f_a((size_t)n * 3), f_b((size_t)n * 3);
  // 1. one force for the whole run: the force rollout == applyForceDevice + the rate rollout
  sw.rolloutForceDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, FEVERY, d_cmd, MRS_DTYPE_F64, 4, d_steady, FS, groups, d_obs, W);
  calm.rolloutRateDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, 4, groups, d_twin, W);  // (unforced)
  twin.applyForceDevice(0, n, d_steady, MRS_DTYPE_F64, FS);
  twin.rolloutRateDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, 4, groups, d_twin, W);
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(obs.data(), d_obs, sizeof(double) * obs.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(ref.data(), d_twin, sizeof(double) * ref.size(), hipMemcpyDeviceToHost));
  CHECK(std::memcmp(obs.data(), ref.data(), sizeof(double) * obs.size()) == 0);
  std::printf("ok steady_force_equals_apply_force_and_the_rate_rollout\n");
  std::vector<mrs_uav_pose_t> p_sw = sw.getPoseArray(0, n), p_calm = calm.getPoseArray(0, n);
  int                         moved = 0;
  for (int i = 0; i < n; i++) moved += std::memcmp(p_sw[(size_t)i].position, p_calm[(size_t)i].position, sizeof(double) * 3) != 0;
  CHECK(moved == n);
  std::printf("ok the_force_moves_every_uav\n");
  // 2. the gust sequence: finite rows, the last row block is the pose array, the swarm is left carrying the last force block
  gusty.rolloutForceDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, FEVERY, d_cmd, MRS_DTYPE_F64, 4, d_gust, FS, groups, d_obs, W);
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(obs.data(), d_obs, sizeof(double) * obs.size(), hipMemcpyDeviceToHost));
  for (size_t e = 0; e < obs.size(); e++) CHECK(std::isfinite(obs[e]));
  std::vector<mrs_uav_pose_t> poses = gusty.getPoseArray(0, n);
  for (int i = 0; i < n; i++) {
    const double* r = &obs[((size_t)(rows - 1) * n + i) * W];
    CHECK(std::memcmp(r, poses[(size_t)i].position, sizeof(double) * 3) == 0);
    CHECK(std::memcmp(r + 6, poses[(size_t)i].orientation, sizeof(double) * 4) == 0);
  }
  std::printf("ok last_row_equals_pose_array\n");
  mrs_throw_on_error(mrs_swarm_get_external_force(gusty.handle(), 0, n, f_a.data()));
  for (int i = 0; i < n; i++) CHECK(std::memcmp(&f_a[(size_t)i * 3], &gust[((size_t)(FB - 1) * n + i) * FS], sizeof(double) * 3) == 0);
  std::printf("ok last_force_block_is_left_behind\n");
  // 3. applyForceDevice == applyForce
  for (int i = 0; i < n; i++) std::memcpy(&f_b[(size_t)i * 3], &gust[((size_t)2 * n + i) * FS], sizeof(double) * 3);
  sw.applyForceDevice(0, n, d_gust + (size_t)2 * n * FS, MRS_DTYPE_F64, FS);
  mrs_throw_on_error(mrs_swarm_apply_force(twin.handle(), 0, n, f_b.data()));
  sw.makeSteps(0.001, 5);
  twin.makeSteps(0.001, 5);
  std::vector<mrs_uav_pose_t> pa = sw.getPoseArray(0, n), pb = twin.getPoseArray(0, n);
  for (int i = 0; i < n; i++) CHECK(std::memcmp(pa[(size_t)i].position, pb[(size_t)i].position, sizeof(double) * 3) == 0);
  std::printf("ok apply_force_device_equals_apply_force\n");
  // a refused call throws and changes nothing: a force rate that does not divide the steps
  bool threw = false;
  try {
    gusty.rolloutForceDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, 7, d_cmd, MRS_DTYPE_F64, 4, d_gust, FS, groups, d_obs, W);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  std::vector<mrs_uav_pose_t> after = gusty.getPoseArray(0, n);
  for (int i = 0; i < n; i++) CHECK(std::memcmp(after[(size_t)i].position, poses[(size_t)i].position, sizeof(double) * 3) == 0);
  std::printf("ok refused_call_changes_nothing\n");
  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f && std::fwrite(obs.data(), sizeof(double), obs.size(), f) == obs.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  HIP(hipFree(d_cmd));
  HIP(hipFree(d_gust));
  HIP(hipFree(d_steady));
  HIP(hipFree(d_obs));
  HIP(hipFree(d_twin));
  return 0;
}
