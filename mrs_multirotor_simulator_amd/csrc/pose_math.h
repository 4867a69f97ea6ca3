// pose_math.h — per-UAV pose expressions shared by the kernel units that derive published quantities from the state columns
// (outputs.hip: publisher payloads; device_io.hip and rollout_device.inc: observation rows for device-resident callers, obs_row.h).
// Each function turns FP contraction off for itself (and body_velocity keeps its products unfused in a -ffp-contract=fast unit), so
// one expression gives the same bits in every unit that includes it.
#pragma once
#include <hip/hip_runtime.h>

// Eigen::Quaterniond(Matrix3d) (what mrs_lib::AttitudeConverter(R) stores): Eigen/src/Geometry/Quaternion.h,
// quaternionbase_assign_impl<Other,3,3>.  R row-major; q = {x, y, z, w}.
__device__ __forceinline__ void quat_from_matrix(const double m[9], double q[4]) {
#pragma clang fp contract(off)  // (no product here feeds an add: nothing a -ffp-contract=fast unit could fuse either)
  double t = (m[0] + m[4]) + m[8];
  if (t > 0) {
    t    = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t    = 0.5 / t;
    q[0] = (m[7] - m[5]) * t;
    q[1] = (m[2] - m[6]) * t;
    q[2] = (m[3] - m[1]) * t;
  } else {
    // i = argmax of the diagonal with Eigen's tie rules; written without dynamic register indexing
    const bool i1 = m[4] > m[0];
    const double mi1 = i1 ? m[4] : m[0];
    const bool i2 = m[8] > mi1;
    if (i2) {  // i=2, j=0, k=1
      t    = sqrt(m[8] - m[0] - m[4] + 1.0);
      q[2] = 0.5 * t;
      t    = 0.5 / t;
      q[3] = (m[3] - m[1]) * t;  // (m(k,j) - m(j,k)) = m(1,0) - m(0,1)
      q[0] = (m[2] + m[6]) * t;  // (m(j,i) + m(i,j)) = m(0,2) + m(2,0)
      q[1] = (m[5] + m[7]) * t;  // (m(k,i) + m(i,k)) = m(1,2) + m(2,1)
    } else if (i1) {  // i=1, j=2, k=0
      t    = sqrt(m[4] - m[8] - m[0] + 1.0);
      q[1] = 0.5 * t;
      t    = 0.5 / t;
      q[3] = (m[2] - m[6]) * t;  // m(0,2) - m(2,0)
      q[2] = (m[7] + m[5]) * t;  // m(2,1) + m(1,2)
      q[0] = (m[1] + m[3]) * t;  // m(0,1) + m(1,0)
    } else {  // i=0, j=1, k=2
      t    = sqrt(m[0] - m[4] - m[8] + 1.0);
      q[0] = 0.5 * t;
      t    = 0.5 / t;
      q[3] = (m[7] - m[5]) * t;  // m(2,1) - m(1,2)
      q[1] = (m[3] + m[1]) * t;  // m(1,0) + m(0,1)
      q[2] = (m[6] + m[2]) * t;  // m(2,0) + m(0,2)
    }
  }
}

// A product the code generator must not fuse into the add that follows.  In a unit compiled with -ffp-contract=fast (the FAST step
// unit, which includes this file through obs_row.h) the backend contracts every multiply-add it sees, whatever the pragma says; an empty
// asm makes the product opaque there.  Elsewhere it is the plain product.
__device__ __forceinline__ double mrs_unfused(double x) {
#if defined(MRS_FAST) && MRS_FAST
  asm("" : "+v"(x));
#endif
  return x;
}

// component c of R^T v (odom.twist.twist.linear, src/uav_system_ros.cpp:356); R row-major
__device__ __forceinline__ double body_velocity(const double R[9], const double v[3], int c) {
#pragma clang fp contract(off)
  return (mrs_unfused(R[c] * v[0]) + mrs_unfused(R[3 + c] * v[1])) + mrs_unfused(R[6 + c] * v[2]);
}
