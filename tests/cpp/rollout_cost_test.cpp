// rollout_cost_test.cpp — UavSwarm::rolloutCostDevice with plain hipMalloc'd rows: 1 000 UAVs take B = 6 ATTITUDE_RATE_CMD row blocks, each
// held for 10 steps, and are evaluated every 20 steps (3 evaluations) against per-UAV targets under per-evaluation weights.  The cost
// vector must equal, bit for bit, the restatement of include/mrs_swarm.h applied on the host to the rows UavSwarm::rolloutRateDevice
// writes on a twin swarm; the final states must agree; a second call with accumulate adds to the vector; a refused call changes nothing.
// The costs are written to argv[1] for tests/test_rollout_cost_gpu.py to compare with mrs_multirotor_simulator_amd.tensors.rollout_cost
// of the same swarm.  Exit code 0 and "ok ..." lines on success.
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
  const int                    steps = B * HOLD, E = steps / EVERY;
  MultirotorModel::ModelParams mp;
  std::vector<Eigen::Vector3d> pos;
  std::vector<double>          hdg;
  std::vector<double>          cmd((size_t)B * n * 4), tgt((size_t)E * n * W), wt((size_t)E * W);
  for (int i = 0; i < n; i++) {  // (the same expressions as test_rollout_cost_gpu.test_cpp_facade_equals_python)
    pos.push_back(Eigen::Vector3d(4.0 * (i % 32), 4.0 * (i / 32), 5.0));
    hdg.push_back(0.003 * i);
    for (int j = 0; j < B; j++) {
      double* c = &cmd[((size_t)j * n + i) * 4];
      c[0] = 0.02 * std::sin(0.1 * j + 0.001 * i);
      c[1] = -0.01 + 0.0 * j + 0.0 * i;
      c[2] = 0.3 + 0.0001 * i + 0.0 * j;
      c[3] = 0.55 + 0.005 * j + 0.0 * i;
    }
    for (int e = 0; e < E; e++)
      for (int c = 0; c < W; c++) tgt[((size_t)e * n + i) * W + c] = 0.25 * c - 0.5 * e + 0.002 * i;
  }
  for (int e = 0; e < E; e++)
    for (int c = 0; c < W; c++) wt[(size_t)e * W + c] = (e == E - 1 ? 10.0 : 1.0) + 0.125 * c;
  UavSwarm sw(n), twin(n);
  sw.construct(0, n, mp, pos, hdg);
  twin.construct(0, n, mp, pos, hdg);
  double *d_cmd = nullptr, *d_tgt = nullptr, *d_wt = nullptr, *d_cost = nullptr, *d_obs = nullptr;
  HIP(hipMalloc((void**)&d_cmd, sizeof(double) * cmd.size()));
  HIP(hipMalloc((void**)&d_tgt, sizeof(double) * tgt.size()));
  HIP(hipMalloc((void**)&d_wt, sizeof(double) * wt.size()));
  HIP(hipMalloc((void**)&d_cost, sizeof(double) * (size_t)n));
  HIP(hipMalloc((void**)&d_obs, sizeof(double) * (size_t)E * n * W));
  HIP(hipMemcpy(d_cmd, cmd.data(), sizeof(double) * cmd.size(), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_tgt, tgt.data(), sizeof(double) * tgt.size(), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_wt, wt.data(), sizeof(double) * wt.size(), hipMemcpyHostToDevice));
  HIP(hipMemset(d_cost, 0xFF, sizeof(double) * (size_t)n));  // (a NaN pattern: accumulate = false must overwrite it)
  const uint32_t groups = MRS_OBS_POS | MRS_OBS_VEL | MRS_OBS_QUAT;
  sw.rolloutCostDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, 4, groups, d_tgt, W, d_wt, W, d_cost);
  twin.rolloutRateDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, 4, groups, d_obs, W);
  HIP(hipDeviceSynchronize());
  std::vector<double> cost((size_t)n), obs((size_t)E * n * W), want((size_t)n);
  HIP(hipMemcpy(cost.data(), d_cost, sizeof(double) * cost.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(obs.data(), d_obs, sizeof(double) * obs.size(), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) {
    volatile double c = 0.0;  // (volatile: every operation rounds to FP64 on its own)
    for (int e = 0; e < E; e++) {
      volatile double term = 0.0;
      for (int col = 0; col < W; col++) {
        volatile double d  = obs[((size_t)e * n + i) * W + col] - tgt[((size_t)e * n + i) * W + col];
        volatile double wd = wt[(size_t)e * W + col] * d;
        volatile double p  = wd * d;
        term               = term + p;
      }
      c = c + term;
    }
    want[(size_t)i] = c;
  }
  CHECK(std::memcmp(cost.data(), want.data(), sizeof(double) * (size_t)n) == 0);
  std::printf("ok cost_equals_the_restatement\n");
  for (int i = 0; i < n; i++) CHECK(std::isfinite(cost[(size_t)i]) && cost[(size_t)i] > 0.0);
  std::vector<mrs_uav_pose_t> poses = sw.getPoseArray(0, n), twin_poses = twin.getPoseArray(0, n);
  for (int i = 0; i < n; i++) {
    CHECK(std::memcmp(poses[(size_t)i].position, twin_poses[(size_t)i].position, sizeof(double) * 3) == 0);
    CHECK(std::memcmp(poses[(size_t)i].orientation, twin_poses[(size_t)i].orientation, sizeof(double) * 4) == 0);
  }
  std::printf("ok final_state_equals_the_rate_rollout\n");
  // a refused call throws and changes nothing: a rate that does not divide the steps, and no observation group
  for (int which = 0; which < 2; which++) {
    bool threw = false;
    try {
      sw.rolloutCostDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, which == 0 ? 7 : EVERY, d_cmd, MRS_DTYPE_F64, 4, which == 0 ? groups : 0u,
                           d_tgt, W, d_wt, W, d_cost);
    } catch (const std::exception&) {
      threw = true;
    }
    CHECK(threw);
  }
  std::vector<mrs_uav_pose_t> after = sw.getPoseArray(0, n);
  for (int i = 0; i < n; i++) CHECK(std::memcmp(after[(size_t)i].position, poses[(size_t)i].position, sizeof(double) * 3) == 0);
  std::vector<double> again((size_t)n);
  HIP(hipMemcpy(again.data(), d_cost, sizeof(double) * again.size(), hipMemcpyDeviceToHost));
  CHECK(std::memcmp(again.data(), cost.data(), sizeof(double) * (size_t)n) == 0);
  std::printf("ok refused_call_changes_nothing\n");
  // accumulate: a second horizon adds to the vector
  sw.rolloutCostDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, 4, groups, d_tgt, W, d_wt, W, d_cost, true);
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(again.data(), d_cost, sizeof(double) * again.size(), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) CHECK(again[(size_t)i] > cost[(size_t)i]);
  std::printf("ok accumulate_adds\n");
  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f && std::fwrite(cost.data(), sizeof(double), cost.size(), f) == cost.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  HIP(hipFree(d_cmd));
  HIP(hipFree(d_tgt));
  HIP(hipFree(d_wt));
  HIP(hipFree(d_cost));
  HIP(hipFree(d_obs));
  return 0;
}
