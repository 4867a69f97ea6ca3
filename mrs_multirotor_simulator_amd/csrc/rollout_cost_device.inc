// rollout_cost_device.inc — cost rollouts (mrs_swarm_rollout_cost_device): the kernels of rollout_rate_device.inc with a hook that, where
// the rate hook writes an observation row, compares the row's FP64 values with a target row and adds the weighted squared distance to
// the UAV's element of a cost vector.  A sampling-based planner wants one number per sample back from a horizon: the row never leaves
// the registers, and a call stores 8 B per UAV and evaluation where the rate rollout stores a row.
//
// Included behind rollout_force_device.inc (RolloutRateHook's commands and schedule arithmetic, LaneObs, kRolloutMaxSteps).  Kernels of
// their own, for the reason given in rollout_rate_device.inc: none of the three existing rollout calls pays for the targets.
//
// The running sum crosses sub-steps and launches in memory: at every due sub-step the lane reads its cost element, adds the term and
// stores it (the element belongs to one lane; launches follow each other in stream order).  The host zeroes the vector in front of
// the first launch unless the call accumulates, so the kernels know one case only, and the sum is the same however the call is cut
// into launches.

namespace {

struct RolloutCostHook {
  RolloutCostDev r;

  __device__ __forceinline__ bool mine(int i) const { return (unsigned)(i - r.first) < (unsigned)r.count; }
  // the command side is the rate hook's, word for word
  __device__ __forceinline__ RolloutRateHook rate() const {
    return RolloutRateHook{RolloutRateDev{r.cmd, nullptr, r.first, r.count, r.cmd_stride, 0, r.cmd_sched, 0u, r.mode_bits}};
  }
  template <class SW>
  __device__ __forceinline__ void cmd(const SW& sw, int i, int s) const {
    rate().cmd(sw, i, s);
  }
  template <class SW, class PT>
  __device__ __forceinline__ void cmd_lane(const SW&, PT&, int, const Lane&, int) const {}
  // the term of evaluation block `blk` of this launch (obs_row.h).  64-bit row addresses: blocks x count x stride passes 2^31.  The
  // target address is per lane (tgt_row == 0: the same for every lane) and the weight address is wave-uniform; both are read with
  // vector loads, a shared row as a broadcast: scalar loads would hold a row's worth of scalar registers the kernels do not have
  template <class Src>
  __device__ __forceinline__ double term(const Src& src, int i, int blk, uint32_t groups, uint32_t cmd_word) const {
    const size_t ta = (size_t)blk * (size_t)r.tgt_blk + (size_t)(i - r.first) * (size_t)r.tgt_row;
    const size_t wa = (size_t)blk * (size_t)r.wt_row;
    if (MRS_RO_HI(cmd_word) & 32u)
      return mrs_obs_row_cost(src, groups, static_cast<const float*>(r.target) + ta, static_cast<const float*>(r.weight) + wa);
    return mrs_obs_row_cost(src, groups, static_cast<const double*>(r.target) + ta, static_cast<const double*>(r.weight) + wa);
  }
  // after post_step of sub-step s: the evaluation that is due here, on the values an observation row would hold
  template <class SW, class PT>
  __device__ __forceinline__ void obs(const SW& sw, PT& P, int i, const Lane& L, int s) const {
    if (!mine(i)) return;
    const uint32_t w = RolloutRateHook::fresh_word(r.cost_sched);
    const int      j = RolloutRateHook::due(w, s);
    if (MRS_RO_HI(w) == 0u || j < 0) return;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, P.n_motors, false};
    double*           c = r.cost + (size_t)(i - r.first);
    const double      t = term(src, i, j, MRS_RO_HI(w), RolloutRateHook::fresh_word(r.cmd_sched));
    *c                  = *c + t;
  }
  // once per lane (RolloutRateHook::enter): a UAV on hold is not stepped, but the loop this call stands for still writes its commands
  // and evaluates its unchanged state: one term per evaluation that falls into this launch, added in order
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int substeps) const {
    if (!mine(i)) return false;
    L.flags = (L.flags & ~FLAG_MODE_MASK) | r.mode_bits;
    if (!(L.flags & FLAG_HOLD)) return false;
    const int starts = RolloutRateHook::due_count(r.cmd_sched, substeps);
    if (starts > 0) rate().cmd_row(sw, i, starts - 1, r.cmd_sched);
    if (MRS_RO_HI(r.cost_sched) != 0u) {
      const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[L.flags >> FLAG_TYPE_SHIFT].n_motors, true};
      const int         ends = RolloutRateHook::due_count(r.cost_sched, substeps);
      double*           c    = r.cost + (size_t)(i - r.first);
      double            sum  = *c;
      for (int b = 0; b < ends; b++) sum = sum + term(src, i, b, MRS_RO_HI(r.cost_sched), r.cmd_sched);
      *c = sum;
    }
    sw.F[i] = L.flags;
    return true;
  }
};

}  // namespace

// The five shapes of rollout_device.inc a fourth time, with the launch bounds chosen there.
#define MRS_ROLLOUT_COST_KERNEL(name, bounds, CASCADE, UNIFORM, BUF)                                                                  \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, int substeps, RolloutCostDev r) { \
    const CollDev none{};                                                                                                          \
    int  blk_;                                                                                                                     \
    bool took_;                                                                                                                    \
    step_kernel_body<CASCADE, UNIFORM, 1, true, MRS_SU, false, false, false>(SwarmAcc<BUF>(sw), dt, inv_dt, substeps, none, blk_, took_, \
                                                                             RolloutCostHook{r});                                  \
  }
MRS_ROLLOUT_COST_KERNEL(mrs_uav_rollout_cost, (64, 1), true, true, false)
MRS_ROLLOUT_COST_KERNEL(mrs_uav_rollout_cost_buf, (64, 1), true, true, true)
MRS_ROLLOUT_COST_KERNEL(mrs_uav_model_rollout_cost, (64, 1), false, true, false)
MRS_ROLLOUT_COST_KERNEL(mrs_uav_model_rollout_cost_buf, (64, MRS_WAVES_PER_SIMD), false, true, true)
MRS_ROLLOUT_COST_KERNEL(mrs_uav_rollout_cost_mixed, (64), true, false, false)
#undef MRS_ROLLOUT_COST_KERNEL

// n_steps steps of the whole swarm with the rows of `r` (whose cmd / target / weight point at row block 0, whose schedule words hold the
// width, dtype and groups of the call, and whose tgt_blk / tgt_row / wt_row are the call's; the schedule bits and first blocks are set
// here, per launch, as mrs_launch_rollout_rate sets them): evaluation j falls behind step (j + 1) * cost_every - 1.  r.cost must hold
// the sums the call starts from.  variant and the buffer / pointer choice as mrs_launch_rollout_rate.
extern "C" hipError_t KNAME(mrs_launch_rollout_cost)(SwarmDev sw, RolloutCostDev r, double dt, int n_steps, int cmd_every, int cost_every, int variant,
                                                     hipStream_t st) {
  static_assert(kRolloutMaxSteps <= 64, "a launch's schedule: s0 < 64, p <= 64 (RolloutRateDev)");
  const int nb = (sw.n + 63) / 64;
  if (nb <= 0 || n_steps <= 0 || cmd_every <= 0 || cost_every <= 0) return hipSuccess;
  sw.blk0 = 0;
  const dim3           g(nb), b(64);
  const double         inv_dt = 1.0 / dt;
  static const bool    no_buf = getenv("MRS_NO_BUFFER_ADDRESSING") != nullptr;
  const bool           buf    = !no_buf && (unsigned long long)F_COUNT * (unsigned long long)sw.npad * 8ull < (1ull << 32);
  const RolloutCostDev call   = r;
  const size_t         elem   = (MRS_RO_HI(call.cmd_sched) & 32u) ? sizeof(float) : sizeof(double);
  for (int t0 = 0; t0 < n_steps; t0 += kRolloutMaxSteps) {
    const int sub = n_steps - t0 < kRolloutMaxSteps ? n_steps - t0 : kRolloutMaxSteps;
    // the first sub-step that starts a command block, and the first an evaluation falls behind; none in this launch: width / groups 0
    const int       cs0 = (cmd_every - t0 % cmd_every) % cmd_every, es0 = cost_every - 1 - t0 % cost_every;
    const long long cb0 = ((long long)t0 + cs0) / cmd_every, eb0 = t0 / cost_every;
    r.cmd_sched  = cs0 < sub ? (call.cmd_sched & 0xFF000000u) | mrs_ro_sched(cs0, cmd_every) : (call.cmd_sched & (32u << 24));
    r.cost_sched = es0 < sub ? (call.cost_sched & 0xFF000000u) | mrs_ro_sched(es0, cost_every) : 0u;
    r.cmd    = !call.cmd ? nullptr : static_cast<const char*>(call.cmd) + (size_t)cb0 * (size_t)call.count * (size_t)call.cmd_stride * elem;
    r.target = static_cast<const char*>(call.target) + (size_t)eb0 * (size_t)call.tgt_blk * elem;
    r.weight = static_cast<const char*>(call.weight) + (size_t)eb0 * (size_t)call.wt_row * elem;
    if (variant == 1) {
      if (buf)
        hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout_cost_buf), g, b, 0, st, sw, dt, inv_dt, sub, r);
      else
        hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout_cost), g, b, 0, st, sw, dt, inv_dt, sub, r);
    } else {
      if (buf)
        hipLaunchKernelGGL(KNAME(mrs_uav_rollout_cost_buf), g, b, 0, st, sw, dt, inv_dt, sub, r);
      else
        hipLaunchKernelGGL(KNAME(mrs_uav_rollout_cost), g, b, 0, st, sw, dt, inv_dt, sub, r);
    }
    if (sw.n_mixed > 0) hipLaunchKernelGGL(KNAME(mrs_uav_rollout_cost_mixed), dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, sub, r);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
