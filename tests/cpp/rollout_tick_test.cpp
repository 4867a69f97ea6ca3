// rollout_tick_test.cpp — UavSwarm::rolloutTickDevice with plain hipMalloc'd rows: 1 000 UAVs on a 4 m grid, of which the first 16 odd
// ones stand 0.4 m beside their even neighbour, take B = 6 ATTITUDE_RATE_CMD row blocks held for 4 ticks each in crash mode and report
// position, velocity, orientation and the crash flags every 2 ticks (12 row blocks).  The rows must equal, bit for bit, those of the
// loop the call stands for on a twin swarm (setInputDevice / makeStep / gatherDevice + crashedDevice / handleCollisions); the crash bytes
// are 1 for the 32 UAVs in contact (the collision pass of tick 0 crashed them; block 0 is taken after tick 1) and 0 for all others.  Rows and crash bytes are
// written to argv[1] for tests/test_rollout_tick_gpu.py to compare with mrs_multirotor_simulator_amd.tensors.rollout_ticks of the same
// swarm.  Exit code 0 and "ok ..." lines on success.
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
  const int                    n = 1000, B = 6, HOLD = 4, EVERY = 2, W = 10, PAIRS = 16;  // W: POS | VEL | QUAT
  const int                    ticks = B * HOLD, rows = ticks / EVERY;
  const double                 dt = 0.001, rebounce = 100.0;
  MultirotorModel::ModelParams mp;
  std::vector<Eigen::Vector3d> pos;
  std::vector<double>          hdg;
  std::vector<double>          cmd((size_t)B * n * 4);
  for (int i = 0; i < n; i++) {  // (the same expressions as test_rollout_tick_gpu.test_cpp_facade_equals_python)
    pos.push_back(Eigen::Vector3d(4.0 * (i % 32), 4.0 * (i / 32), 5.0));
    if (i < 2 * PAIRS && i % 2 == 1) pos.back() = Eigen::Vector3d(4.0 * (i - 1) + 0.4, 0.0, 5.0);
    hdg.push_back(0.003 * i);
    for (int j = 0; j < B; j++) {
      double* c = &cmd[((size_t)j * n + i) * 4];
      c[0] = 0.02 * std::sin(0.1 * j + 0.001 * i);
      c[1] = -0.01 + 0.0 * j + 0.0 * i;
      c[2] = 0.3 + 0.0001 * i + 0.0 * j;
      c[3] = 0.55 + 0.005 * j + 0.0 * i;
    }
  }
  UavSwarm sw(n, -1, false), twin(n, -1, false);  // LITERAL arithmetic: the call equals the loop bit for bit
  sw.construct(0, n, mp, pos, hdg);
  twin.construct(0, n, mp, pos, hdg);
  double * d_cmd = nullptr, *d_obs = nullptr, *d_want = nullptr;
  uint8_t *d_cr = nullptr, *d_cr_want = nullptr;
  HIP(hipMalloc((void**)&d_cmd, sizeof(double) * cmd.size()));
  HIP(hipMalloc((void**)&d_obs, sizeof(double) * (size_t)rows * n * W));  // exactly the decimated sizes
  HIP(hipMalloc((void**)&d_want, sizeof(double) * (size_t)rows * n * W));
  HIP(hipMalloc((void**)&d_cr, (size_t)rows * n));
  HIP(hipMalloc((void**)&d_cr_want, (size_t)rows * n));
  HIP(hipMemset(d_cr, 7, (size_t)rows * n));
  HIP(hipMemcpy(d_cmd, cmd.data(), sizeof(double) * cmd.size(), hipMemcpyHostToDevice));
  const uint32_t groups = MRS_OBS_POS | MRS_OBS_VEL | MRS_OBS_QUAT;
  sw.rolloutTickDevice(0, n, MRS_ATTITUDE_RATE_CMD, dt, ticks, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, 4, groups, d_obs, W, d_cr, true, rebounce);
  for (int t = 0; t < ticks; t++) {  // the loop the call stands for
    if (t % HOLD == 0) twin.setInputDevice(0, n, MRS_ATTITUDE_RATE_CMD, d_cmd + (size_t)(t / HOLD) * n * 4, MRS_DTYPE_F64, 4);
    twin.makeStep(dt);
    if ((t + 1) % EVERY == 0) {
      const size_t j = (size_t)((t + 1) / EVERY - 1);
      twin.gatherDevice(0, n, groups, d_want + j * n * W, MRS_DTYPE_F64, W);
      twin.crashedDevice(0, n, d_cr_want + j * n);
    }
    twin.handleCollisions(true, true, rebounce);
  }
  HIP(hipDeviceSynchronize());
  std::vector<double>  obs((size_t)rows * n * W), want((size_t)rows * n * W);
  std::vector<uint8_t> cr((size_t)rows * n), cr_want((size_t)rows * n);
  HIP(hipMemcpy(obs.data(), d_obs, sizeof(double) * obs.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(want.data(), d_want, sizeof(double) * want.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(cr.data(), d_cr, cr.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(cr_want.data(), d_cr_want, cr_want.size(), hipMemcpyDeviceToHost));
  CHECK(std::memcmp(obs.data(), want.data(), sizeof(double) * obs.size()) == 0);
  CHECK(std::memcmp(cr.data(), cr_want.data(), cr.size()) == 0);
  std::printf("ok rows_equal_the_loop\n");
  for (int b = 0; b < rows; b++)
    for (int i = 0; i < n; i++) CHECK(cr[(size_t)b * n + i] == (i < 2 * PAIRS ? 1 : 0));
  std::printf("ok crash_bytes\n");
  std::vector<mrs_uav_pose_t> poses = sw.getPoseArray(0, n), twin_poses = twin.getPoseArray(0, n);
  for (int i = 0; i < n; i++) {
    const double* r = &obs[((size_t)(rows - 1) * n + i) * W];
    CHECK(std::memcmp(r, poses[(size_t)i].position, sizeof(double) * 3) == 0);
    CHECK(std::memcmp(r + 6, poses[(size_t)i].orientation, sizeof(double) * 4) == 0);
    CHECK(std::memcmp(poses[(size_t)i].position, twin_poses[(size_t)i].position, sizeof(double) * 3) == 0);
  }
  std::printf("ok last_row_equals_pose_array\n");
  // a refused call throws and changes nothing: a rebounce that is not finite
  bool threw = false;
  try {
    sw.rolloutTickDevice(0, n, MRS_ATTITUDE_RATE_CMD, dt, ticks, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, 4, groups, d_obs, W, d_cr, true, NAN);
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
    CHECK(std::fwrite(cr.data(), 1, cr.size(), f) == cr.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  HIP(hipFree(d_cmd));
  HIP(hipFree(d_obs));
  HIP(hipFree(d_want));
  HIP(hipFree(d_cr));
  HIP(hipFree(d_cr_want));
  return 0;
}
