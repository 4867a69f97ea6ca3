// rollout_rate_device.inc — control-rate rollouts (mrs_swarm_rollout_rate_device): the rollout kernels of rollout_device.inc with a hook
// that reads a command row every cmd_every steps and writes an observation row every obs_every steps.  At a control rate setInput
// latches (uav_system.hpp:175-248): the F_CMD columns keep command block t / cmd_every through its steps (:304-380), and getState (:386)
// is asked for once per obs_every steps.
//
// Included behind rollout_device.inc (LaneObs, kRolloutMaxSteps).  Kernels of their own, not two more words in RolloutDev: the step
// kernels are short of scalar registers, and with the rates in the plain hook the plain cascade rollout measured 4-6 % slower in FAST
// (MEASUREMENTS §7.4).  mrs_swarm_rollout_device therefore keeps its kernels instruction for instruction.

namespace {

// The sub-step hook of a control-rate rollout launch.  Row (j, k) belongs to UAV first + k and the launch's j-th due sub-step.  Which
// sub-steps read a command row or write an observation row is the launch's schedule (RolloutRateDev): the test, the block index and the
// dtype are wave-uniform, so a sub-step inside a held command and inside an observation block loads nothing from the caller's rows and
// stores nothing to them.
struct RolloutRateHook {
  RolloutRateDev r;

  __device__ __forceinline__ bool mine(int i) const { return (unsigned)(i - r.first) < (unsigned)r.count; }
  __device__ __forceinline__ size_t at(int i, int blk, int stride) const {
    return ((size_t)blk * (size_t)r.count + (size_t)(i - r.first)) * (size_t)stride;  // 64-bit: blocks x count x stride passes 2^31
  }
  // a schedule word as this sub-step sees it: the empty asm keeps its fields from being pulled out of the sub-step loop as scalar
  // registers of their own (the word alone lives through the loop)
  static __device__ __forceinline__ uint32_t fresh_word(uint32_t w) {
    asm volatile("" : "+s"(w));
    return w;
  }
  // sub-step s (< 64) is the j-th due one of the schedule w (-1: it is not due)
  static __device__ __forceinline__ int due(uint32_t w, int s) {
    const unsigned x = (unsigned)s - MRS_RO_S0(w);
    const unsigned j = (x * MRS_RO_M(w)) >> 12;
    return ((unsigned)s >= MRS_RO_S0(w) && j * MRS_RO_P(w) == x) ? (int)j : -1;
  }
  // due sub-steps of the schedule w among the first `substeps`
  static __device__ __forceinline__ int due_count(uint32_t w, int substeps) {
    if ((unsigned)substeps <= MRS_RO_S0(w)) return 0;
    return (int)((((unsigned)substeps - 1u - MRS_RO_S0(w)) * MRS_RO_M(w)) >> 12) + 1;
  }
  // command row block `blk` into the F_CMD columns (mrs_swarm_set_input_device's k_scatter_cmd); FP32 is widened exactly
  template <class SW>
  __device__ __forceinline__ void cmd_row(const SW& sw, int i, int blk, uint32_t w) const {
    const unsigned off8  = (unsigned)i * 8u;
    const size_t   a     = at(i, blk, r.cmd_stride);
    const int      width = (int)(MRS_RO_HI(w) & 31u);
    if (MRS_RO_HI(w) & 32u) {
      const float* p = static_cast<const float*>(r.cmd) + a;
#pragma unroll
      for (int j = 0; j < F_FF - F_CMD; j++)
        if (j < width) sw.st(F_CMD + j, off8, (double)p[j]);
    } else {
      const double* p = static_cast<const double*>(r.cmd) + a;
#pragma unroll
      for (int j = 0; j < F_FF - F_CMD; j++)
        if (j < width) sw.st(F_CMD + j, off8, p[j]);
    }
  }
  // top of sub-step s: the command row of the block that starts here; inside a block the columns hold the command as they stand
  template <class SW>
  __device__ __forceinline__ void cmd(const SW& sw, int i, int s) const {
    if (!mine(i)) return;
    const uint32_t w = fresh_word(r.cmd_sched);
    const int      j = due(w, s);
    if (j < 0) return;
    cmd_row(sw, i, j, w);
  }
  template <class SW, class PT>
  __device__ __forceinline__ void cmd_lane(const SW&, PT&, int, const Lane&, int) const {}
  template <class Src>
  __device__ __forceinline__ void write_obs(const Src& src, int i, int blk, uint32_t groups, uint32_t cmd_word) const {
    const size_t a = at(i, blk, r.obs_stride);
    if (MRS_RO_HI(cmd_word) & 32u)
      mrs_obs_row(src, groups, static_cast<float*>(r.obs) + a);
    else
      mrs_obs_row(src, groups, static_cast<double*>(r.obs) + a);
  }
  // after post_step of sub-step s: the observation row of the block that ends here
  template <class SW, class PT>
  __device__ __forceinline__ void obs(const SW& sw, PT& P, int i, const Lane& L, int s) const {
    const uint32_t w = fresh_word(r.obs_sched);
    const int      j = due(w, s);
    if (MRS_RO_HI(w) == 0u || j < 0 || !mine(i)) return;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, P.n_motors, false};
    write_obs(src, i, j, MRS_RO_HI(w), fresh_word(r.cmd_sched));
  }
  // once per lane, after the wave-uniform exits: the range takes the new mode (the flag word is stored behind the steps).  A UAV on hold
  // is not stepped (UavSystemRos::makeStep), but the loop this call stands for still writes its commands and gathers its unchanged
  // state: the row of the last command block that starts in this launch (if one does), one row of the unchanged state per observation
  // block that ends in it, the flag word — and the lane is done.
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int substeps) const {
    if (!mine(i)) return false;
    L.flags = (L.flags & ~FLAG_MODE_MASK) | r.mode_bits;
    if (!(L.flags & FLAG_HOLD)) return false;
    const int starts = due_count(r.cmd_sched, substeps);
    if (starts > 0) cmd_row(sw, i, starts - 1, r.cmd_sched);
    if (MRS_RO_HI(r.obs_sched) != 0u) {
      const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[L.flags >> FLAG_TYPE_SHIFT].n_motors, true};
      const int         ends = due_count(r.obs_sched, substeps);
      for (int b = 0; b < ends; b++) write_obs(src, i, b, MRS_RO_HI(r.obs_sched), r.cmd_sched);
    }
    sw.F[i] = L.flags;
    return true;
  }
};

}  // namespace

// The five shapes of rollout_device.inc once more, with the launch bounds chosen there.
#define MRS_ROLLOUT_RATE_KERNEL(name, bounds, CASCADE, UNIFORM, BUF)                                                                  \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, int substeps, RolloutRateDev r) { \
    const CollDev none{};                                                                                                          \
    int  blk_;                                                                                                                     \
    bool took_;                                                                                                                    \
    step_kernel_body<CASCADE, UNIFORM, 1, true, MRS_SU, false, false, false>(SwarmAcc<BUF>(sw), dt, inv_dt, substeps, none, blk_, took_, \
                                                                             RolloutRateHook{r});                                  \
  }
MRS_ROLLOUT_RATE_KERNEL(mrs_uav_rollout_rate, (64, 1), true, true, false)
MRS_ROLLOUT_RATE_KERNEL(mrs_uav_rollout_rate_buf, (64, 1), true, true, true)
MRS_ROLLOUT_RATE_KERNEL(mrs_uav_model_rollout_rate, (64, 1), false, true, false)
MRS_ROLLOUT_RATE_KERNEL(mrs_uav_model_rollout_rate_buf, (64, MRS_WAVES_PER_SIMD), false, true, true)
MRS_ROLLOUT_RATE_KERNEL(mrs_uav_rollout_rate_mixed, (64), true, false, false)
#undef MRS_ROLLOUT_RATE_KERNEL

// n_steps steps of the whole swarm with the rows of `r` (whose cmd / obs point at row block 0, and whose schedule words hold the width,
// dtype and groups of the call; the schedule bits and first blocks are set here, per launch): command block j starts at step
// j * cmd_every, observation block j ends with step (j + 1) * obs_every - 1; block boundaries fall anywhere inside and across launches,
// and a launch inside one held command reads no command row at all.  variant: 0 every input mode, 1 model only (no UAV in a cascade
// mode), as mrs_launch_step; the buffer / pointer choice is that of mrs_launch_step (MRS_NO_BUFFER_ADDRESSING forces pointers).
extern "C" hipError_t KNAME(mrs_launch_rollout_rate)(SwarmDev sw, RolloutRateDev r, double dt, int n_steps, int cmd_every, int obs_every, int variant,
                                                hipStream_t st) {
  static_assert(kRolloutMaxSteps <= 64, "a launch's schedule: s0 < 64, p <= 64 (RolloutRateDev)");
  const int nb = (sw.n + 63) / 64;
  if (nb <= 0 || n_steps <= 0 || cmd_every <= 0 || obs_every <= 0) return hipSuccess;
  sw.blk0 = 0;
  const dim3        g(nb), b(64);
  const double      inv_dt = 1.0 / dt;
  static const bool no_buf = getenv("MRS_NO_BUFFER_ADDRESSING") != nullptr;
  const bool        buf    = !no_buf && (unsigned long long)F_COUNT * (unsigned long long)sw.npad * 8ull < (1ull << 32);
  const RolloutRateDev  call   = r;
  const size_t      elem   = (MRS_RO_HI(call.cmd_sched) & 32u) ? sizeof(float) : sizeof(double);
  for (int t0 = 0; t0 < n_steps; t0 += kRolloutMaxSteps) {
    const int sub = n_steps - t0 < kRolloutMaxSteps ? n_steps - t0 : kRolloutMaxSteps;
    // the first sub-step that starts a command block, and the first that ends an observation block; none in this launch: width / groups 0
    const int       cs0 = (cmd_every - t0 % cmd_every) % cmd_every, os0 = obs_every - 1 - t0 % obs_every;
    const long long cb0 = ((long long)t0 + cs0) / cmd_every, ob0 = t0 / obs_every;
    r.cmd_sched = cs0 < sub ? (call.cmd_sched & 0xFF000000u) | mrs_ro_sched(cs0, cmd_every) : (call.cmd_sched & (32u << 24));
    r.obs_sched = os0 < sub ? (call.obs_sched & 0xFF000000u) | mrs_ro_sched(os0, obs_every) : 0u;
    r.cmd       = !call.cmd ? nullptr : static_cast<const char*>(call.cmd) + (size_t)cb0 * (size_t)call.count * (size_t)call.cmd_stride * elem;
    r.obs       = call.obs ? static_cast<char*>(call.obs) + (size_t)ob0 * (size_t)call.count * (size_t)call.obs_stride * elem : nullptr;
    if (variant == 1) {
      if (buf)
        hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout_rate_buf), g, b, 0, st, sw, dt, inv_dt, sub, r);
      else
        hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout_rate), g, b, 0, st, sw, dt, inv_dt, sub, r);
    } else {
      if (buf)
        hipLaunchKernelGGL(KNAME(mrs_uav_rollout_rate_buf), g, b, 0, st, sw, dt, inv_dt, sub, r);
      else
        hipLaunchKernelGGL(KNAME(mrs_uav_rollout_rate), g, b, 0, st, sw, dt, inv_dt, sub, r);
    }
    if (sw.n_mixed > 0) hipLaunchKernelGGL(KNAME(mrs_uav_rollout_rate_mixed), dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, sub, r);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
