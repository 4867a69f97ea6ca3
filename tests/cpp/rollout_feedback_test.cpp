// rollout_feedback_test.cpp — UavSwarm::rolloutFeedbackDevice with plain hipMalloc'd rows: 1 000 UAVs take B = 6 nominal
// ATTITUDE_RATE_CMD row blocks, each held for 10 steps, with a per-UAV gain (UAV-minor, one block for the call) on OBS_VEL | OBS_OMEGA and
// one shared setpoint row per block, and are evaluated every 20 steps as in rollout_cost_test.cpp.  With zero gains cost and final state
// must equal, bit for bit, UavSwarm::rolloutCostDevice on a twin swarm; with the gains the run differs; the call without cost groups
// steps the same state; a refused call changes nothing.  The costs of the run with gains are written to argv[1] for
// tests/test_rollout_feedback_gpu.py to compare with mrs_multirotor_simulator_amd.tensors.rollout_feedback of the same swarm.  Exit code
// 0 and "ok ..." lines on success.
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

static bool same_poses(const std::vector<mrs_uav_pose_t>& a, const std::vector<mrs_uav_pose_t>& b) {
  for (size_t i = 0; i < a.size(); i++)
    if (std::memcmp(a[i].position, b[i].position, sizeof(double) * 3) != 0 || std::memcmp(a[i].orientation, b[i].orientation, sizeof(double) * 4) != 0)
      return false;
  return a.size() == b.size();
}

int main(int argc, char** argv) {
  const int                    n = 1000, B = 6, HOLD = 10, EVERY = 20, W = 10, WC = 4, WO = 6;  // W: POS | VEL | QUAT; WO: VEL | OMEGA
  const int                    steps = B * HOLD, E = steps / EVERY;
  MultirotorModel::ModelParams mp;
  std::vector<Eigen::Vector3d> pos;
  std::vector<double>          hdg;
  std::vector<double>          cmd((size_t)B * n * 4), tgt((size_t)E * n * W), wt((size_t)E * W), gain((size_t)WC * WO * n), ref((size_t)B * WO);
  for (int i = 0; i < n; i++) {  // (the same expressions as test_rollout_feedback_gpu.test_cpp_facade_equals_python)
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
    for (int c = 0; c < WC; c++)
      for (int j = 0; j < WO; j++) gain[((size_t)c * WO + j) * n + i] = 0.01 * (c + 1) - 0.004 * j + 0.00001 * i;  // UAV-minor
  }
  for (int e = 0; e < E; e++)
    for (int c = 0; c < W; c++) wt[(size_t)e * W + c] = (e == E - 1 ? 10.0 : 1.0) + 0.125 * c;
  for (int b = 0; b < B; b++)
    for (int j = 0; j < WO; j++) ref[(size_t)b * WO + j] = 0.1 * j - 0.05 * b;
  UavSwarm sw(n), zero(n), twin(n), bare(n);
  for (UavSwarm* s : {&sw, &zero, &twin, &bare}) s->construct(0, n, mp, pos, hdg);
  double *d_cmd = nullptr, *d_tgt = nullptr, *d_wt = nullptr, *d_cost = nullptr, *d_cost2 = nullptr, *d_gain = nullptr, *d_zero = nullptr, *d_ref = nullptr;
  HIP(hipMalloc((void**)&d_cmd, sizeof(double) * cmd.size()));
  HIP(hipMalloc((void**)&d_tgt, sizeof(double) * tgt.size()));
  HIP(hipMalloc((void**)&d_wt, sizeof(double) * wt.size()));
  HIP(hipMalloc((void**)&d_cost, sizeof(double) * (size_t)n));
  HIP(hipMalloc((void**)&d_cost2, sizeof(double) * (size_t)n));
  HIP(hipMalloc((void**)&d_gain, sizeof(double) * gain.size()));
  HIP(hipMalloc((void**)&d_zero, sizeof(double) * gain.size()));
  HIP(hipMalloc((void**)&d_ref, sizeof(double) * ref.size()));
  HIP(hipMemcpy(d_cmd, cmd.data(), sizeof(double) * cmd.size(), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_tgt, tgt.data(), sizeof(double) * tgt.size(), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_wt, wt.data(), sizeof(double) * wt.size(), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_gain, gain.data(), sizeof(double) * gain.size(), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_ref, ref.data(), sizeof(double) * ref.size(), hipMemcpyHostToDevice));
  HIP(hipMemset(d_zero, 0, sizeof(double) * gain.size()));
  HIP(hipMemset(d_cost, 0xFF, sizeof(double) * (size_t)n));  // (a NaN pattern: accumulate = false must overwrite it)
  HIP(hipMemset(d_cost2, 0xFF, sizeof(double) * (size_t)n));
  const uint32_t fb = MRS_OBS_VEL | MRS_OBS_OMEGA, groups = MRS_OBS_POS | MRS_OBS_VEL | MRS_OBS_QUAT;
  // zero gains: the cost rollout, bit for bit
  zero.rolloutFeedbackDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, 4, fb, d_zero, true, 1, d_ref, 0, B, groups, d_tgt, W,
                             d_wt, W, d_cost);
  twin.rolloutCostDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, 4, groups, d_tgt, W, d_wt, W, d_cost2);
  HIP(hipDeviceSynchronize());
  std::vector<double> open_loop((size_t)n), want((size_t)n), cost((size_t)n);
  HIP(hipMemcpy(open_loop.data(), d_cost, sizeof(double) * open_loop.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(want.data(), d_cost2, sizeof(double) * want.size(), hipMemcpyDeviceToHost));
  CHECK(std::memcmp(open_loop.data(), want.data(), sizeof(double) * (size_t)n) == 0);
  for (int i = 0; i < n; i++) CHECK(std::isfinite(open_loop[(size_t)i]) && open_loop[(size_t)i] > 0.0);
  CHECK(same_poses(zero.getPoseArray(0, n), twin.getPoseArray(0, n)));
  std::printf("ok zero_gains_are_the_cost_rollout\n");
  // the gains close the loop: another run, another cost
  HIP(hipMemset(d_cost, 0xFF, sizeof(double) * (size_t)n));
  sw.rolloutFeedbackDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, 4, fb, d_gain, true, 1, d_ref, 0, B, groups, d_tgt, W,
                           d_wt, W, d_cost);
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(cost.data(), d_cost, sizeof(double) * cost.size(), hipMemcpyDeviceToHost));
  int differ = 0;
  for (int i = 0; i < n; i++) {
    CHECK(std::isfinite(cost[(size_t)i]) && cost[(size_t)i] > 0.0);
    differ += cost[(size_t)i] != open_loop[(size_t)i];
  }
  CHECK(differ == n);
  const std::vector<mrs_uav_pose_t> poses = sw.getPoseArray(0, n);
  CHECK(!same_poses(poses, twin.getPoseArray(0, n)));
  std::printf("ok feedback_changes_the_run\n");
  // without cost groups: the same closed loop, nothing but the state
  bare.rolloutFeedbackDevice(0, n, MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, HOLD, d_cmd, MRS_DTYPE_F64, 4, fb, d_gain, true, 1, d_ref, 0, B);
  HIP(hipDeviceSynchronize());
  CHECK(same_poses(poses, bare.getPoseArray(0, n)));
  std::printf("ok no_cost_steps_the_same_state\n");
  // a refused call throws and changes nothing: a wrong number of gain blocks, no feedback group, a mode without a payload
  for (int which = 0; which < 3; which++) {
    bool threw = false;
    try {
      sw.rolloutFeedbackDevice(0, n, which == 2 ? MRS_INPUT_UNKNOWN : MRS_ATTITUDE_RATE_CMD, 0.001, steps, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, 4,
                               which == 1 ? 0u : fb, d_gain, true, which == 0 ? 2 : 1, d_ref, 0, B, groups, d_tgt, W, d_wt, W, d_cost);
    } catch (const std::exception&) {
      threw = true;
    }
    CHECK(threw);
  }
  CHECK(same_poses(poses, sw.getPoseArray(0, n)));
  std::vector<double> again((size_t)n);
  HIP(hipMemcpy(again.data(), d_cost, sizeof(double) * again.size(), hipMemcpyDeviceToHost));
  CHECK(std::memcmp(again.data(), cost.data(), sizeof(double) * (size_t)n) == 0);
  std::printf("ok refused_call_changes_nothing\n");
  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f && std::fwrite(cost.data(), sizeof(double), cost.size(), f) == cost.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  for (double* p : {d_cmd, d_tgt, d_wt, d_cost, d_cost2, d_gain, d_zero, d_ref}) HIP(hipFree(p));
  return 0;
}
