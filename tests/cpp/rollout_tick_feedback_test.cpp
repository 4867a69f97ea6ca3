// rollout_tick_feedback_test.cpp — UavSwarm::rolloutTickFeedbackDevice with plain hipMalloc'd rows: the 1 000 UAVs of
// rollout_tick_cost_test.cpp (a 4 m grid, the first 16 odd ones 0.4 m beside their even neighbour) take B = 6 NOMINAL ATTITUDE_RATE_CMD
// row blocks held for 4 ticks each in crash mode; at the start of every block the command is the nominal row plus one shared 4 x 6 gain
// matrix times (the block's shared setpoint row - the UAV's position and velocity before the step).  The swarm is evaluated every 2
// ticks as in rollout_tick_cost_test.cpp.  Cost and positions must equal, bit for bit, the loop the call stands for on a twin swarm
// (gatherDevice -> the law on the host -> setInputDevice / makeStep / gatherDevice + crashedDevice / handleCollisions) and the
// contract's sum over its rows and crash bytes.  A pure closed-loop run (no cost at all) over the next horizon equals the loop too.  The
// cost vector is written to argv[1] for tests/test_rollout_tick_feedback_gpu.py to compare with
// mrs_multirotor_simulator_amd.tensors.rollout_tick_feedback of the same swarm.  Exit code 0 and "ok ..." lines on success.
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

namespace {
const int      n = 1000, B = 6, HOLD = 4, EVERY = 2, W = 10, WO = 6, WC = 4, PAIRS = 16;  // W: POS | VEL | QUAT; WO: POS | VEL
const double   dt = 0.001, rebounce = 100.0, crash_cost = 1000.0;
const uint32_t fb_groups = MRS_OBS_POS | MRS_OBS_VEL;

// the loop's feedback step for command block b on `g`: gather, the law line by line on the host (volatile: every operation is rounded
// to FP64 on its own), set_input
int feedback_block(UavSwarm& g, int b, const std::vector<double>& cmd, const std::vector<double>& gain, const std::vector<double>& ref, double* d_o,
                   double* d_u) {
  std::vector<double> o((size_t)n * WO), u((size_t)n * WC);
  g.gatherDevice(0, n, fb_groups, d_o, MRS_DTYPE_F64, WO);
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(o.data(), d_o, sizeof(double) * o.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < n; k++)
    for (int c = 0; c < WC; c++) {
      volatile double acc = cmd[((size_t)b * n + k) * WC + c];
      for (int j = 0; j < WO; j++) {
        volatile double e = ref[(size_t)b * WO + j] - o[(size_t)k * WO + j];
        volatile double p = gain[(size_t)c * WO + j] * e;
        acc               = acc + p;
      }
      u[(size_t)k * WC + c] = acc;
    }
  HIP(hipMemcpy(d_u, u.data(), sizeof(double) * u.size(), hipMemcpyHostToDevice));
  g.setInputDevice(0, n, MRS_ATTITUDE_RATE_CMD, d_u, MRS_DTYPE_F64, WC);
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  const int                    ticks = B * HOLD, evals = ticks / EVERY;
  MultirotorModel::ModelParams mp;
  std::vector<Eigen::Vector3d> pos;
  std::vector<double>          hdg;
  std::vector<double>          cmd((size_t)B * n * WC), gain((size_t)WC * WO), ref((size_t)B * WO), target((size_t)evals * W), weight(W);
  for (int i = 0; i < n; i++) {  // (the same expressions as test_rollout_tick_feedback_gpu.test_cpp_facade_equals_python)
    pos.push_back(Eigen::Vector3d(4.0 * (i % 32), 4.0 * (i / 32), 5.0));
    if (i < 2 * PAIRS && i % 2 == 1) pos.back() = Eigen::Vector3d(4.0 * (i - 1) + 0.4, 0.0, 5.0);
    hdg.push_back(0.003 * i);
    for (int j = 0; j < B; j++) {
      double* c = &cmd[((size_t)j * n + i) * WC];
      c[0] = 0.02 * std::sin(0.1 * j + 0.001 * i);
      c[1] = -0.01 + 0.0 * j + 0.0 * i;
      c[2] = 0.3 + 0.0001 * i + 0.0 * j;
      c[3] = 0.55 + 0.005 * j + 0.0 * i;
    }
  }
  for (int c = 0; c < WC; c++)
    for (int j = 0; j < WO; j++) gain[(size_t)c * WO + j] = (c + 1) * (j + 1) / 65536.0;  // (exact)
  for (int b = 0; b < B; b++)
    for (int j = 0; j < WO; j++) ref[(size_t)b * WO + j] = 0.5 * j + 0.25 * b;
  for (int j = 0; j < evals; j++)
    for (int c = 0; c < W; c++) target[(size_t)j * W + c] = 0.25 * c + 0.125 * j;
  for (int c = 0; c < W; c++) weight[(size_t)c] = 0.5 + 0.0625 * c;
  UavSwarm sw(n, -1, false), twin(n, -1, false);  // LITERAL arithmetic: the call equals the loop bit for bit
  sw.construct(0, n, mp, pos, hdg);
  twin.construct(0, n, mp, pos, hdg);
  double * d_cmd = nullptr, *d_gain = nullptr, *d_ref = nullptr, *d_tgt = nullptr, *d_wt = nullptr, *d_cost = nullptr, *d_want = nullptr;
  double * d_o = nullptr, *d_u = nullptr;
  uint8_t* d_cr_want = nullptr;
  HIP(hipMalloc((void**)&d_cmd, sizeof(double) * cmd.size()));  // exactly the sizes the call needs
  HIP(hipMalloc((void**)&d_gain, sizeof(double) * gain.size()));
  HIP(hipMalloc((void**)&d_ref, sizeof(double) * ref.size()));
  HIP(hipMalloc((void**)&d_tgt, sizeof(double) * target.size()));
  HIP(hipMalloc((void**)&d_wt, sizeof(double) * weight.size()));
  HIP(hipMalloc((void**)&d_cost, sizeof(double) * n));
  HIP(hipMalloc((void**)&d_want, sizeof(double) * (size_t)evals * n * W));
  HIP(hipMalloc((void**)&d_cr_want, (size_t)evals * n));
  HIP(hipMalloc((void**)&d_o, sizeof(double) * (size_t)n * WO));
  HIP(hipMalloc((void**)&d_u, sizeof(double) * (size_t)n * WC));
  HIP(hipMemset(d_cost, 0x7f, sizeof(double) * n));  // (overwritten: the call does not accumulate)
  HIP(hipMemcpy(d_cmd, cmd.data(), sizeof(double) * cmd.size(), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_gain, gain.data(), sizeof(double) * gain.size(), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_ref, ref.data(), sizeof(double) * ref.size(), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_tgt, target.data(), sizeof(double) * target.size(), hipMemcpyHostToDevice));
  HIP(hipMemcpy(d_wt, weight.data(), sizeof(double) * weight.size(), hipMemcpyHostToDevice));
  const uint32_t groups = MRS_OBS_POS | MRS_OBS_VEL | MRS_OBS_QUAT;
  sw.rolloutTickFeedbackDevice(0, n, MRS_ATTITUDE_RATE_CMD, dt, ticks, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, WC, fb_groups, d_gain, false, 1, d_ref, 0, B,
                               groups, d_tgt, 0, d_wt, 0, crash_cost, d_cost, false, true, rebounce);
  for (int t = 0; t < ticks; t++) {  // the loop the call stands for
    if (t % HOLD == 0) CHECK(feedback_block(twin, t / HOLD, cmd, gain, ref, d_o, d_u) == 0);
    twin.makeStep(dt);
    if ((t + 1) % EVERY == 0) {
      const size_t j = (size_t)((t + 1) / EVERY - 1);
      twin.gatherDevice(0, n, groups, d_want + j * n * W, MRS_DTYPE_F64, W);
      twin.crashedDevice(0, n, d_cr_want + j * n);
    }
    twin.handleCollisions(true, true, rebounce);
  }
  HIP(hipDeviceSynchronize());
  std::vector<double>  cost((size_t)n), rows((size_t)evals * n * W);
  std::vector<uint8_t> cr((size_t)evals * n);
  HIP(hipMemcpy(cost.data(), d_cost, sizeof(double) * cost.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(rows.data(), d_want, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(cr.data(), d_cr_want, cr.size(), hipMemcpyDeviceToHost));
  std::vector<double> want((size_t)n);
  for (int k = 0; k < n; k++) {  // the contract's evaluation, line by line
    volatile double c = 0.0;
    for (int j = 0; j < evals; j++) {
      volatile double term = 0.0;
      for (int col = 0; col < W; col++) {
        volatile double d = rows[((size_t)j * n + k) * W + col] - target[(size_t)j * W + col];
        volatile double p = weight[(size_t)col] * d;
        volatile double q = p * d;
        term              = term + q;
      }
      c = c + term;
      if (cr[(size_t)j * n + k]) c = c + crash_cost;
    }
    want[(size_t)k] = c;
  }
  CHECK(std::memcmp(cost.data(), want.data(), sizeof(double) * cost.size()) == 0);
  std::printf("ok cost_equals_the_loop\n");
  for (int j = 0; j < evals; j++)
    for (int i = 0; i < n; i++) CHECK(cr[(size_t)j * n + i] == (i < 2 * PAIRS ? 1 : 0));
  for (int i = 0; i < 2 * PAIRS; i++) CHECK(cost[(size_t)i] >= crash_cost * evals);  // (the weights are positive: no term is negative)
  std::printf("ok crashed_uavs_pay\n");
  std::vector<mrs_uav_pose_t> poses = sw.getPoseArray(0, n), twin_poses = twin.getPoseArray(0, n);
  for (int i = 0; i < n; i++) CHECK(std::memcmp(poses[(size_t)i].position, twin_poses[(size_t)i].position, sizeof(double) * 3) == 0);
  std::printf("ok state_equals_the_loop\n");
  // a refused call throws and changes nothing: a missing gain, cost groups without a cost vector
  int threw = 0;
  try {
    sw.rolloutTickFeedbackDevice(0, n, MRS_ATTITUDE_RATE_CMD, dt, ticks, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, WC, fb_groups, nullptr, false, 1, d_ref, 0, B,
                                 groups, d_tgt, 0, d_wt, 0, crash_cost, d_cost, false, true, rebounce);
  } catch (const std::exception&) {
    threw++;
  }
  try {
    sw.rolloutTickFeedbackDevice(0, n, MRS_ATTITUDE_RATE_CMD, dt, ticks, HOLD, EVERY, d_cmd, MRS_DTYPE_F64, WC, fb_groups, d_gain, false, 1, d_ref, 0, B,
                                 groups, d_tgt, 0, d_wt, 0, crash_cost, nullptr, false, true, rebounce);
  } catch (const std::exception&) {
    threw++;
  }
  CHECK(threw == 2);
  std::vector<mrs_uav_pose_t> after = sw.getPoseArray(0, n);
  std::vector<double>         cost_after((size_t)n);
  HIP(hipMemcpy(cost_after.data(), d_cost, sizeof(double) * cost_after.size(), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) CHECK(std::memcmp(after[(size_t)i].position, poses[(size_t)i].position, sizeof(double) * 3) == 0);
  CHECK(std::memcmp(cost_after.data(), cost.data(), sizeof(double) * cost.size()) == 0);
  std::printf("ok refused_call_changes_nothing\n");
  // a pure closed-loop run over two more command blocks: no evaluation, the state is the loop's and the vector stays as it is
  sw.rolloutTickFeedbackDevice(0, n, MRS_ATTITUDE_RATE_CMD, dt, 2 * HOLD, HOLD, HOLD, d_cmd, MRS_DTYPE_F64, WC, fb_groups, d_gain, false, 1, d_ref, 0, 2, 0u,
                               nullptr, 0, nullptr, 0, 0.0, nullptr, false, true, rebounce);
  for (int t = 0; t < 2 * HOLD; t++) {
    if (t % HOLD == 0) CHECK(feedback_block(twin, t / HOLD, cmd, gain, ref, d_o, d_u) == 0);
    twin.makeStep(dt);
    twin.handleCollisions(true, true, rebounce);
  }
  HIP(hipDeviceSynchronize());
  poses = sw.getPoseArray(0, n), twin_poses = twin.getPoseArray(0, n);
  for (int i = 0; i < n; i++) CHECK(std::memcmp(poses[(size_t)i].position, twin_poses[(size_t)i].position, sizeof(double) * 3) == 0);
  HIP(hipMemcpy(cost_after.data(), d_cost, sizeof(double) * cost_after.size(), hipMemcpyDeviceToHost));
  CHECK(std::memcmp(cost_after.data(), cost.data(), sizeof(double) * cost.size()) == 0);
  std::printf("ok closed_loop_without_cost\n");
  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f && std::fwrite(cost.data(), sizeof(double), cost.size(), f) == cost.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  HIP(hipFree(d_cmd));
  HIP(hipFree(d_gain));
  HIP(hipFree(d_ref));
  HIP(hipFree(d_tgt));
  HIP(hipFree(d_wt));
  HIP(hipFree(d_cost));
  HIP(hipFree(d_want));
  HIP(hipFree(d_cr_want));
  HIP(hipFree(d_o));
  HIP(hipFree(d_u));
  return 0;
}
