// rollout_device.inc — device-resident rollouts (mrs_swarm_rollout_device): a run of fused steps that reads a new command row before
// each step and writes an observation row after it, so a planner's horizon of H steps is one launch instead of 3H.
//
// Included at the end of step_kernel_fast.hip and step_kernel_literal.hip, after step_device.inc: the kernels below are the *_multi
// kernels of that file with a sub-step hook (step_kernel_body's HK), so each flavour compiles the step body once more and nothing else.
// Per UAV of the range and step t, a launch does what `setInput(cmd[t]); makeStep(dt); getState()` does (uav_system.hpp:175-248,
// :304-380, :386): the hook writes command row t into the F_CMD columns at the top of sub-step t — in *_multi kernels the cascade and
// the motor stage load their commands from those columns — and writes observation row t from the lane's registers after post_step
// (obs_row.h: the rows of mrs_swarm_gather_device, bit for bit).  UAVs outside the range are stepped with their own commands.
#include "obs_row.h"

namespace {

// what an observation row reads of a lane (obs_row.h): the state after the sub-step from registers, the IMU of post_step, and the rpm
// columns the motor stage stored during this sub-step.  A lane on hold is not stepped: its IMU is the column's.
template <class SW>
struct LaneObs {
  const SW&   sw;
  const Lane& L;
  unsigned    off8;
  int         nm;
  bool        imu_col;
  __device__ __forceinline__ double x(int c) const { return L.y[c]; }
  __device__ __forceinline__ double v(int c) const { return L.y[3 + c]; }
  __device__ __forceinline__ double R(int c) const { return L.y[6 + c]; }
  __device__ __forceinline__ double omega(int c) const { return L.y[15 + c]; }
  __device__ __forceinline__ double imu(int c) const { return imu_col ? sw.ld(F_IMU + c, off8) : L.imu[c]; }
  __device__ __forceinline__ double rpm(int m) const { return sw.ld(F_RPM + m, off8); }
  __device__ __forceinline__ int    n_motors() const { return nm; }
};

// The sub-step hook of a rollout launch.  Row (t, k) belongs to UAV first + k; t = r.t0 + s.  The dtype is a wave-uniform branch.
struct RolloutHook {
  RolloutDev r;

  __device__ __forceinline__ bool mine(int i) const { return (unsigned)(i - r.first) < (unsigned)r.count; }
  __device__ __forceinline__ size_t at(int i, int s, int stride) const {
    return ((size_t)(r.t0 + s) * (size_t)r.count + (size_t)(i - r.first)) * (size_t)stride;  // 64-bit: T x count x stride passes 2^31
  }
  // command row of sub-step s into the F_CMD columns (mrs_swarm_set_input_device's k_scatter_cmd); FP32 is widened exactly
  template <class SW>
  __device__ __forceinline__ void cmd(const SW& sw, int i, int s) const {
    if (!mine(i)) return;
    const unsigned off8 = (unsigned)i * 8u;
    const size_t   a    = at(i, s, r.cmd_stride);
    if (r.f32) {
      const float* p = static_cast<const float*>(r.cmd) + a;
#pragma unroll
      for (int j = 0; j < F_FF - F_CMD; j++)
        if (j < r.width) sw.st(F_CMD + j, off8, (double)p[j]);
    } else {
      const double* p = static_cast<const double*>(r.cmd) + a;
#pragma unroll
      for (int j = 0; j < F_FF - F_CMD; j++)
        if (j < r.width) sw.st(F_CMD + j, off8, p[j]);
    }
  }
  template <class SW, class PT>
  __device__ __forceinline__ void cmd_lane(const SW&, PT&, int, const Lane&, int) const {}
  template <class Src>
  __device__ __forceinline__ void write_obs(const Src& src, int i, int s) const {
    const size_t a = at(i, s, r.obs_stride);
    if (r.f32)
      mrs_obs_row(src, r.groups, static_cast<float*>(r.obs) + a);
    else
      mrs_obs_row(src, r.groups, static_cast<double*>(r.obs) + a);
  }
  // observation row of sub-step s, after post_step
  template <class SW, class PT>
  __device__ __forceinline__ void obs(const SW& sw, PT& P, int i, const Lane& L, int s) const {
    if (r.groups == 0u || !mine(i)) return;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, P.n_motors, false};
    write_obs(src, i, s);
  }
  // once per lane, after the wave-uniform exits: the range takes the new mode (the flag word is stored behind the steps).  A UAV on hold
  // is not stepped (UavSystemRos::makeStep), but the loop this call stands for still writes its commands and gathers its unchanged
  // state: the last command row of the launch, one row of the unchanged state per sub-step, the flag word — and the lane is done.
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int substeps) const {
    if (!mine(i)) return false;
    L.flags = (L.flags & ~FLAG_MODE_MASK) | r.mode_bits;
    if (!(L.flags & FLAG_HOLD)) return false;
    cmd(sw, i, substeps - 1);
    if (r.groups != 0u) {
      const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[L.flags >> FLAG_TYPE_SHIFT].n_motors, true};
      for (int s = 0; s < substeps; s++) write_obs(src, i, s);
    }
    sw.F[i] = L.flags;
    return true;
  }
};

}  // namespace

// The five shapes of the *_multi kernels: cascade or model-only, pointer- or buffer-addressed columns, and the mixed-airframe blocks.
// The pointer-addressed model-only kernel gets one wave per SIMD's registers: with two it spills (36-108 B of scratch per lane), and
// it only serves swarms whose state passes 4 GiB.
#define MRS_ROLLOUT_KERNEL(name, bounds, CASCADE, UNIFORM, BUF)                                                                       \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, int substeps, RolloutDev r) { \
    const CollDev none{};                                                                                                          \
    int  blk_;                                                                                                                     \
    bool took_;                                                                                                                    \
    step_kernel_body<CASCADE, UNIFORM, 1, true, MRS_SU, false, false, false>(SwarmAcc<BUF>(sw), dt, inv_dt, substeps, none, blk_, took_, \
                                                                             RolloutHook{r});                                      \
  }
MRS_ROLLOUT_KERNEL(mrs_uav_rollout, (64, 1), true, true, false)
MRS_ROLLOUT_KERNEL(mrs_uav_rollout_buf, (64, 1), true, true, true)
MRS_ROLLOUT_KERNEL(mrs_uav_model_rollout, (64, 1), false, true, false)
MRS_ROLLOUT_KERNEL(mrs_uav_model_rollout_buf, (64, MRS_WAVES_PER_SIMD), false, true, true)
MRS_ROLLOUT_KERNEL(mrs_uav_rollout_mixed, (64), true, false, false)
#undef MRS_ROLLOUT_KERNEL

// Longest run of steps one rollout launch takes: a longer rollout is split into launches of at most this many steps, so that no launch
// runs unboundedly long (64 cascade steps of 1 M UAVs take a few milliseconds).
constexpr int kRolloutMaxSteps = 64;

// n_steps steps of the whole swarm with the rows of `r` (r.t0 is set here).  variant: 0 every input mode, 1 model only (no UAV in a
// cascade mode), as mrs_launch_step; the buffer / pointer choice is that of mrs_launch_step (MRS_NO_BUFFER_ADDRESSING forces pointers).
extern "C" hipError_t KNAME(mrs_launch_rollout)(SwarmDev sw, RolloutDev r, double dt, int n_steps, int variant, hipStream_t st) {
  const int nb = (sw.n + 63) / 64;
  if (nb <= 0 || n_steps <= 0) return hipSuccess;
  sw.blk0 = 0;
  const dim3        g(nb), b(64);
  const double      inv_dt = 1.0 / dt;
  static const bool no_buf = getenv("MRS_NO_BUFFER_ADDRESSING") != nullptr;
  const bool        buf    = !no_buf && (unsigned long long)F_COUNT * (unsigned long long)sw.npad * 8ull < (1ull << 32);
  for (int t0 = 0; t0 < n_steps; t0 += kRolloutMaxSteps) {
    const int sub = n_steps - t0 < kRolloutMaxSteps ? n_steps - t0 : kRolloutMaxSteps;
    r.t0          = t0;
    if (variant == 1) {
      if (buf)
        hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout_buf), g, b, 0, st, sw, dt, inv_dt, sub, r);
      else
        hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout), g, b, 0, st, sw, dt, inv_dt, sub, r);
    } else {
      if (buf)
        hipLaunchKernelGGL(KNAME(mrs_uav_rollout_buf), g, b, 0, st, sw, dt, inv_dt, sub, r);
      else
        hipLaunchKernelGGL(KNAME(mrs_uav_rollout), g, b, 0, st, sw, dt, inv_dt, sub, r);
    }
    if (sw.n_mixed > 0) hipLaunchKernelGGL(KNAME(mrs_uav_rollout_mixed), dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, sub, r);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
