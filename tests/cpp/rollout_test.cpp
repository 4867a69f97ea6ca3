// rollout_test.cpp — UavSwarm::rolloutDevice with plain hipMalloc'd rows: 1 000 UAVs take 20 steps of ATTITUDE_RATE_CMD rows and report
// position, velocity and orientation after each.  The last row block must equal the pose array of the final state, and every row is
// finite.  The rows are written to argv[1] for tests/test_rollout_gpu.py to compare with
// mrs_multirotor_simulator_amd.tensors.rollout of the same swarm.  Exit code 0 and "ok ..." lines on success.
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
  const int                    n = 1000, H = 20, W = 10;  // W: POS | VEL | QUAT
  MultirotorModel::ModelParams mp;
  std::vector<Eigen::Vector3d> pos;
  std::vector<double>          hdg;
  std::vector<double>          cmd((size_t)H * n * 4);
  for (int i = 0; i < n; i++) {  // (the same expressions as test_rollout_gpu.test_cpp_facade_equals_python)
    pos.push_back(Eigen::Vector3d(4.0 * (i % 32), 4.0 * (i / 32), 5.0));
    hdg.push_back(0.003 * i);
    for (int t = 0; t < H; t++) {
      double* c = &cmd[((size_t)t * n + i) * 4];
      c[0] = 0.02 * std::sin(0.1 * t + 0.001 * i);
      c[1] = -0.01 + 0.0 * t + 0.0 * i;
      c[2] = 0.3 + 0.0001 * i + 0.0 * t;
      c[3] = 0.55 + 0.005 * t + 0.0 * i;
    }
  }
  UavSwarm sw(n);
  sw.construct(0, n, mp, pos, hdg);
  double *d_cmd = nullptr, *d_obs = nullptr;
  HIP(hipMalloc((void**)&d_cmd, sizeof(double) * cmd.size()));
  HIP(hipMalloc((void**)&d_obs, sizeof(double) * (size_t)H * n * W));
  HIP(hipMemcpy(d_cmd, cmd.data(), sizeof(double) * cmd.size(), hipMemcpyHostToDevice));
  sw.rolloutDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, H, d_cmd, MRS_DTYPE_F64, 4, MRS_OBS_POS | MRS_OBS_VEL | MRS_OBS_QUAT, d_obs, W);
  HIP(hipDeviceSynchronize());
  std::vector<double> obs((size_t)H * n * W);
  HIP(hipMemcpy(obs.data(), d_obs, sizeof(double) * obs.size(), hipMemcpyDeviceToHost));
  std::vector<mrs_uav_pose_t> poses = sw.getPoseArray(0, n);
  for (int i = 0; i < n; i++) {
    const double* r = &obs[((size_t)(H - 1) * n + i) * W];
    CHECK(std::memcmp(r, poses[(size_t)i].position, sizeof(double) * 3) == 0);
    CHECK(std::memcmp(r + 6, poses[(size_t)i].orientation, sizeof(double) * 4) == 0);
  }
  std::printf("ok last_row_equals_pose_array\n");
  for (size_t e = 0; e < obs.size(); e++) CHECK(std::isfinite(obs[e]));
  for (int i = 0; i < n; i++) CHECK(obs[(size_t)i * W + 5] != obs[((size_t)(H - 1) * n + i) * W + 5]);  // v_z: every UAV moved
  std::printf("ok rows_finite_and_moving\n");
  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f && std::fwrite(obs.data(), sizeof(double), obs.size(), f) == obs.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  HIP(hipFree(d_cmd));
  HIP(hipFree(d_obs));
  return 0;
}
