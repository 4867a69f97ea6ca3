// rollout_rate_test.cpp — UavSwarm::rolloutRateDevice with plain hipMalloc'd rows: 1 000 UAVs take B = 6 ATTITUDE_RATE_CMD row blocks, each
// held for 10 steps, and report position, velocity and orientation every 20 steps (3 row blocks).  The rows must equal, bit for bit,
// rows 19, 39 and 59 of UavSwarm::rolloutDevice on a twin swarm with every command row repeated ten times; the last row block must equal
// the pose array of the final state.  The rows are written to argv[1] for tests/test_rollout_rate_gpu.py to compare with
// mrs_multirotor_simulator_amd.tensors.rollout(hold=10, obs_every=20) of the same swarm.  Exit code 0 and "ok ..." lines on success.
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
  const int                    n = 1000, B = 6, HOLD = 10, EVERY = 20, W = 10;  // W: POS | VEL | QUAT
  const int                    steps = B * HOLD, rows = steps / EVERY;
  MultirotorModel::ModelParams mp;
  std::vector<Eigen::Vector3d> pos;
  std::vector<double>          hdg;
  std::vector<double>          cmd((size_t)B * n * 4), rep((size_t)steps * n * 4);
  for (int i = 0; i < n; i++) {  // (the same expressions as test_rollout_rate_gpu.test_cpp_facade_equals_python)
    pos.push_back(Eigen::Vector3d(4.0 * (i % 32), 4.0 * (i / 32), 5.0));
    hdg.push_back(0.003 * i);
    for (int j = 0; j < B; j++) {
      double* c = &cmd[((size_t)j * n + i) * 4];
      c[0] = 0.02 * std::sin(0.1 * j + 0.001 * i);
      c[1] = -0.01 + 0.0 * j + 0.0 * i;
      c[2] = 0.3 + 0.0001 * i + 0.0 * j;
      c[3] = 0.55 + 0.005 * j + 0.0 * i;
      for (int h = 0; h < HOLD; h++) std::memcpy(&rep[((size_t)(j * HOLD + h) * n + i) * 4], c, sizeof(double) * 4);
    }
  }
  UavSwarm sw(n), twin(n);
  sw.construct(0, n, mp, pos, hdg);
  twin.construct(0, n, mp, pos, hdg);
  double *d_cmd = nullptr, *d_rep = nullptr, *d_obs = nullptr, *d_all = nullptr;
  HIP(hipMalloc((void**)&d_cmd, sizeof(double) * cmd.size()));
  HIP(hipMalloc((void**)&d_rep, sizeof(double) * rep.size()));
  HIP(hipMalloc((void**)&d_obs, sizeof(double) * (size_t)rows * n * W));  // exactly the decimated size
  HIP(hipMalloc((void**)&d_all, sizeof(double) * (size_t)steps * n * W));
  HIP(hipMemcpy(d_cmd, cmd.data(), sizeof(double) * cmd.size(), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_rep, rep.data(), sizeof(double) * rep.size(), hipMemcpyHostToDevice));
  const uint32_t groups = MRS_OBS_POS | MRS_OBS_VEL | MRS_OBS_QUAT;
  sw.rolloutRateDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, 4, groups, d_obs, W);
  twin.rolloutDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, d_rep, MRS_DTYPE_F64, 4, groups, d_all, W);
  HIP(hipDeviceSynchronize());
  std::vector<double> obs((size_t)rows * n * W), all((size_t)steps * n * W);
  HIP(hipMemcpy(obs.data(), d_obs, sizeof(double) * obs.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(all.data(), d_all, sizeof(double) * all.size(), hipMemcpyDeviceToHost));
  for (int b = 0; b < rows; b++)
    CHECK(std::memcmp(&obs[(size_t)b * n * W], &all[(size_t)((b + 1) * EVERY - 1) * n * W], sizeof(double) * (size_t)n * W) == 0);
  std::printf("ok rows_equal_the_plain_rollout\n");
  std::vector<mrs_uav_pose_t> poses = sw.getPoseArray(0, n), twin_poses = twin.getPoseArray(0, n);
  for (int i = 0; i < n; i++) {
    const double* r = &obs[((size_t)(rows - 1) * n + i) * W];
    CHECK(std::memcmp(r, poses[(size_t)i].position, sizeof(double) * 3) == 0);
    CHECK(std::memcmp(r + 6, poses[(size_t)i].orientation, sizeof(double) * 4) == 0);
    CHECK(std::memcmp(poses[(size_t)i].position, twin_poses[(size_t)i].position, sizeof(double) * 3) == 0);
  }
  std::printf("ok last_row_equals_pose_array\n");
  for (size_t e = 0; e < obs.size(); e++) CHECK(std::isfinite(obs[e]));
  for (int i = 0; i < n; i++) CHECK(obs[(size_t)i * W + 5] != obs[((size_t)(rows - 1) * n + i) * W + 5]);  // v_z: every UAV moved
  std::printf("ok rows_finite_and_moving\n");
  // a refused call throws and changes nothing: a rate that does not divide the steps
  bool threw = false;
  try {
    sw.rolloutRateDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, 7, EVERY, d_cmd, MRS_DTYPE_F64, 4, groups, d_obs, W);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  std::vector<mrs_uav_pose_t> after = sw.getPoseArray(0, n);
  for (int i = 0; i < n; i++) CHECK(std::memcmp(after[(size_t)i].position, poses[(size_t)i].position, sizeof(double) * 3) == 0);
  std::printf("ok refused_call_changes_nothing\n");
  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f && std::fwrite(obs.data(), sizeof(double), obs.size(), f) == obs.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  HIP(hipFree(d_cmd));
  HIP(hipFree(d_rep));
  HIP(hipFree(d_obs));
  HIP(hipFree(d_all));
  return 0;
}
