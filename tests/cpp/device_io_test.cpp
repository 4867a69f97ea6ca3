// device_io_test.cpp — the device-resident calls of the UavSwarm facade with plain hipMalloc'd rows: position commands go in through
// setInputDevice, 1 000 UAVs fly 300 steps, and gatherDevice(POS | QUAT) must equal getPoseArray bit for bit (mrs_uav_pose_t is the same
// 7 doubles).  A twin swarm fed the same commands through the host setInput must end in the same state.  crashedDevice reports the UAVs
// crashed on the host.  Exit code 0 and "ok ..." lines on success.
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

int main() {
  const int                    n = 1000;
  MultirotorModel::ModelParams mp;
  mp.ground_enabled = true;
  mp.ground_z       = 0.0;
  std::vector<Eigen::Vector3d> pos;
  std::vector<double>          hdg;
  std::vector<double>          cmd((size_t)n * 4);
  for (int i = 0; i < n; i++) {
    pos.push_back(Eigen::Vector3d(4.0 * (i % 32), 4.0 * (i / 32), 0.0));
    hdg.push_back(0.003 * i);
    cmd[(size_t)i * 4 + 0] = 4.0 * (i % 32) + 1.0;
    cmd[(size_t)i * 4 + 1] = 4.0 * (i / 32) - 0.5;
    cmd[(size_t)i * 4 + 2] = 2.0 + 0.002 * i;
    cmd[(size_t)i * 4 + 3] = 0.001 * i - 0.5;
  }
  UavSwarm dev(n), host(n);
  dev.construct(0, n, mp, pos, hdg);
  host.construct(0, n, mp, pos, hdg);

  double* d_cmd = nullptr;
  double* d_obs = nullptr;
  uint8_t* d_crashed = nullptr;
  const int stride = 7;  // POS (3) + QUAT (4)
  HIP(hipMalloc((void**)&d_cmd, sizeof(double) * (size_t)n * 4));
  HIP(hipMalloc((void**)&d_obs, sizeof(double) * (size_t)n * stride));
  HIP(hipMalloc((void**)&d_crashed, (size_t)n));
  HIP(hipMemcpy(d_cmd, cmd.data(), sizeof(double) * cmd.size(), hipMemcpyHostToDevice));

  dev.setInputDevice(0, n, MRS_POSITION_CMD, d_cmd, MRS_DTYPE_F64, 4);  // (null stream: fenced against the copy above)
  mrs_throw_on_error(mrs_swarm_set_input(host.handle(), 0, n, MRS_POSITION_CMD, cmd.data(), 4));
  dev.makeSteps(0.001, 300);
  host.makeSteps(0.001, 300);

  int32_t width = 0;
  mrs_throw_on_error(mrs_swarm_gather_width(MRS_OBS_POS | MRS_OBS_QUAT, &width));
  CHECK(width == stride);
  dev.gatherDevice(0, n, MRS_OBS_POS | MRS_OBS_QUAT, d_obs, MRS_DTYPE_F64, stride);
  std::vector<double> obs((size_t)n * stride);
  HIP(hipMemcpy(obs.data(), d_obs, sizeof(double) * obs.size(), hipMemcpyDeviceToHost));
  std::vector<mrs_uav_pose_t> poses = dev.getPoseArray(0, n);
  static_assert(sizeof(mrs_uav_pose_t) == 7 * sizeof(double), "pose record = 7 doubles");
  CHECK(std::memcmp(obs.data(), poses.data(), sizeof(double) * obs.size()) == 0);
  bool moved = false;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < 3; j++) moved = moved || std::fabs(obs[(size_t)i * stride + j] - pos[(size_t)i](j)) > 1e-6;
  CHECK(moved);
  std::printf("ok gather_equals_pose_array %d\n", n);

  std::vector<mrs_uav_pose_t> twin = host.getPoseArray(0, n);
  CHECK(std::memcmp(twin.data(), poses.data(), sizeof(mrs_uav_pose_t) * (size_t)n) == 0);
  std::printf("ok device_commands_equal_host_commands\n");

  mrs_throw_on_error(mrs_swarm_crash(dev.handle(), 100, 7));
  dev.crashedDevice(0, n, d_crashed);
  std::vector<uint8_t> crashed((size_t)n);
  HIP(hipMemcpy(crashed.data(), d_crashed, (size_t)n, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) CHECK(crashed[(size_t)i] == ((i >= 100 && i < 107) ? 1 : 0));
  std::printf("ok crashed_device\n");

  HIP(hipFree(d_cmd));
  HIP(hipFree(d_obs));
  HIP(hipFree(d_crashed));
  return 0;
}
