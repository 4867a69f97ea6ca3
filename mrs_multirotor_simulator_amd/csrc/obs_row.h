// obs_row.h — one observation row of a UAV: the MRS_OBS_* groups of include/mrs_swarm.h concatenated in bit order.  Shared by
// mrs_swarm_gather_device (device_io.hip, values from the state columns) and mrs_swarm_rollout_device (rollout_device.inc, values
// from the step kernel's registers), so both write the same bits.  The FAST step unit compiles with -ffp-contract=fast: the pragma
// here and pose_math.h (the pragmas, and opaque products where the backend would fuse anyway) keep every expression of a row
// uncontracted in either unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mrs_swarm.h"
#include "pose_math.h"

// widths of the observation groups, in bit order (MRS_OBS_POS first)
constexpr int kObsWidth[8] = {3, 3, 3, 9, 4, 3, 3, MRS_MAX_MOTORS};

// The row of `groups` into o[0 .. width).  FP32 rows hold the round-to-nearest cast of the FP64 value.  Src supplies the values:
// x(c), v(c), omega(c), imu(c) for c < 3, R(c) for c < 9 (row-major), n_motors() and rpm(m); a group's values are asked for only
// when the group is selected.
template <typename T, class Src>
__device__ __forceinline__ void mrs_obs_row(const Src& src, const uint32_t groups, T* o) {
#pragma clang fp contract(off)
  double v[3], R[9];
  if (groups & (MRS_OBS_VEL | MRS_OBS_VEL_BODY)) {
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = src.v(c);
  }
  if (groups & (MRS_OBS_VEL_BODY | MRS_OBS_ROT | MRS_OBS_QUAT)) {
#pragma unroll
    for (int c = 0; c < 9; c++) R[c] = src.R(c);
  }
  if (groups & MRS_OBS_POS) {
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = (T)src.x(c);
    o += 3;
  }
  if (groups & MRS_OBS_VEL) {
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = (T)v[c];
    o += 3;
  }
  if (groups & MRS_OBS_VEL_BODY) {
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = (T)body_velocity(R, v, c);
    o += 3;
  }
  if (groups & MRS_OBS_ROT) {
#pragma unroll
    for (int c = 0; c < 9; c++) o[c] = (T)R[c];
    o += 9;
  }
  if (groups & MRS_OBS_QUAT) {
    double q[4];
    quat_from_matrix(R, q);
#pragma unroll
    for (int c = 0; c < 4; c++) o[c] = (T)q[c];
    o += 4;
  }
  if (groups & MRS_OBS_OMEGA) {
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = (T)src.omega(c);
    o += 3;
  }
  if (groups & MRS_OBS_IMU) {
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = (T)src.imu(c);
    o += 3;
  }
  if (groups & MRS_OBS_RPM) {  // 0 past n_motors, as k_pack_states
    const int nm = src.n_motors();
#pragma unroll
    for (int m = 0; m < MRS_MAX_MOTORS; m++) o[m] = (T)(m < nm ? src.rpm(m) : 0.0);
  }
}

// The weighted squared distance of the FP64 row of `groups` (the values mrs_obs_row<double> would write, in its column order) from the
// target row tg[0 .. width) under the weights wt[0 .. width):
//   term = +0.0;  for col ascending: d = row[col] - tg[col];  term = term + (wt[col] * d) * d
// all of it FP64 and uncontracted; T = float targets and weights are widened exactly.  No column is skipped and nothing is
// special-cased (a zero weight times a non-finite residual is what IEEE makes of it; the rpm group's zeros past n_motors take part).
// Every value and every product goes through mrs_unfused: in the FAST unit the backend would otherwise fuse the multiply that produced
// a value into the subtraction, or the last product into the sum.
template <typename T, class Src>
__device__ __forceinline__ double mrs_obs_row_cost(const Src& src, const uint32_t groups, const T* tg, const T* wt) {
#pragma clang fp contract(off)
  double term = 0.0;
  double v[3], R[9];
  const auto col = [&](double value, int c) {
    const double d = mrs_unfused(value) - (double)tg[c];
    term           = term + mrs_unfused(mrs_unfused((double)wt[c] * d) * d);
  };
  if (groups & (MRS_OBS_VEL | MRS_OBS_VEL_BODY)) {
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = src.v(c);
  }
  if (groups & (MRS_OBS_VEL_BODY | MRS_OBS_ROT | MRS_OBS_QUAT)) {
#pragma unroll
    for (int c = 0; c < 9; c++) R[c] = src.R(c);
  }
  if (groups & MRS_OBS_POS) {
#pragma unroll
    for (int c = 0; c < 3; c++) col(src.x(c), c);
    tg += 3, wt += 3;
  }
  if (groups & MRS_OBS_VEL) {
#pragma unroll
    for (int c = 0; c < 3; c++) col(v[c], c);
    tg += 3, wt += 3;
  }
  if (groups & MRS_OBS_VEL_BODY) {
#pragma unroll
    for (int c = 0; c < 3; c++) col(body_velocity(R, v, c), c);
    tg += 3, wt += 3;
  }
  if (groups & MRS_OBS_ROT) {
#pragma unroll
    for (int c = 0; c < 9; c++) col(R[c], c);
    tg += 9, wt += 9;
  }
  if (groups & MRS_OBS_QUAT) {
    double q[4];
    quat_from_matrix(R, q);
#pragma unroll
    for (int c = 0; c < 4; c++) col(q[c], c);
    tg += 4, wt += 4;
  }
  if (groups & MRS_OBS_OMEGA) {
#pragma unroll
    for (int c = 0; c < 3; c++) col(src.omega(c), c);
    tg += 3, wt += 3;
  }
  if (groups & MRS_OBS_IMU) {
#pragma unroll
    for (int c = 0; c < 3; c++) col(src.imu(c), c);
    tg += 3, wt += 3;
  }
  if (groups & MRS_OBS_RPM) {
    const int nm = src.n_motors();
#pragma unroll
    for (int m = 0; m < MRS_MAX_MOTORS; m++) col(m < nm ? src.rpm(m) : 0.0, m);
  }
  return term;
}

// Linear state feedback on the FP64 row of `groups` (the values mrs_obs_row<double> would write, in its column order): on entry u[c]
// holds the nominal command of payload element c < wc, on return
//   for col ascending: e = ref[col] - row[col];  for each c < wc: u[c] = u[c] + (G[c][col] * e)
// which is, accumulator by accumulator, the sum over ascending columns of the contract (mrs_swarm_rollout_feedback_device): the column
// is the outer loop here so that one residual and the wc accumulators are live, never the row.  G[c][col] is read at
// gain[c * g_row + col * g_col] (shared gains: g_col 1, g_row the row width, a wave-uniform address; per-UAV gains: g_col the UAV
// count, the lane's own element behind a coalesced 512-B request per (c, col)).  All of it FP64 and uncontracted; T = float inputs are
// widened exactly.  No column is skipped and nothing is special-cased, as in mrs_obs_row_cost, and the values and products go through
// mrs_unfused for the reason given there.
template <int NC, typename T, class Src>
__device__ __forceinline__ void mrs_obs_row_feedback(const Src& src, const uint32_t groups, const T* ref, const T* gain, const size_t g_col,
                                                     const size_t g_row, const int wc, double (&u)[NC]) {
#pragma clang fp contract(off)
  double v[3], R[9];
  const auto col = [&](double value) {
    // A NaN operand is the residual, bits as they are (the setpoint's if both are NaN), which is what a host subtraction makes of it:
    // gfx950 forms r - o as r + (-o), and the negation would flip the sign bit of a NaN observation on its way into the command.
    const double r = (double)*ref, o = mrs_unfused(value);
    const double d = r - o;
    const double e = r != r ? r : (o != o ? o : d);
#pragma unroll
    for (int c = 0; c < NC; c++)
      if (c < wc) u[c] = u[c] + mrs_unfused((double)gain[(size_t)c * g_row] * e);
    ref++;
    gain += g_col;
  };
  if (groups & (MRS_OBS_VEL | MRS_OBS_VEL_BODY)) {
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = src.v(c);
  }
  if (groups & (MRS_OBS_VEL_BODY | MRS_OBS_ROT | MRS_OBS_QUAT)) {
#pragma unroll
    for (int c = 0; c < 9; c++) R[c] = src.R(c);
  }
  if (groups & MRS_OBS_POS) {
#pragma unroll
    for (int c = 0; c < 3; c++) col(src.x(c));
  }
  if (groups & MRS_OBS_VEL) {
#pragma unroll
    for (int c = 0; c < 3; c++) col(v[c]);
  }
  if (groups & MRS_OBS_VEL_BODY) {
#pragma unroll
    for (int c = 0; c < 3; c++) col(body_velocity(R, v, c));
  }
  if (groups & MRS_OBS_ROT) {
#pragma unroll
    for (int c = 0; c < 9; c++) col(R[c]);
  }
  if (groups & MRS_OBS_QUAT) {
    double q[4];
    quat_from_matrix(R, q);
#pragma unroll
    for (int c = 0; c < 4; c++) col(q[c]);
  }
  if (groups & MRS_OBS_OMEGA) {
#pragma unroll
    for (int c = 0; c < 3; c++) col(src.omega(c));
  }
  if (groups & MRS_OBS_IMU) {
#pragma unroll
    for (int c = 0; c < 3; c++) col(src.imu(c));
  }
  if (groups & MRS_OBS_RPM) {
    const int nm = src.n_motors();
#pragma unroll
    for (int m = 0; m < MRS_MAX_MOTORS; m++) col(m < nm ? src.rpm(m) : 0.0);
  }
}
