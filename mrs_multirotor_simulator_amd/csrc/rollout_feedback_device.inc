// rollout_feedback_device.inc — feedback rollouts (mrs_swarm_rollout_feedback_device): the kernels of rollout_cost_device.inc with a
// hook that, where the cost hook reads a command row, FORMS the command from the state the lane holds: at the top of the sub-step that
// starts command block b the F_CMD columns take  cmd_row + G · (ref_row − obs_row),  obs_row being the FP64 observation row of
// fb_groups BEFORE the step (obs_row.h: mrs_obs_row_feedback).  A caller whose samples are controllers (a gain per UAV, a nominal
// command plus time-varying gains, one law over many initial states) closes the loop inside the launch instead of through a gather, a
// matrix product and a set_input per tick.  The cost side is the cost hook's, word for word.
//
// Included behind rollout_cost_device.inc (RolloutCostHook's obs / term, RolloutRateHook's schedule arithmetic, LaneObs,
// kRolloutMaxSteps).  Kernels of their own, for the reason given in rollout_rate_device.inc: no existing call pays for the gains.
//
// The values an observation row holds BEFORE sub-step s: the state registers; the IMU of the previous sub-step's post_step, and at
// sub-step 0 the IMU column (what the launch before, or the caller, left there); the rpm columns as the previous sub-step's motor
// stage stored them.  The feedback has no memory: a launch needs nothing of the launch before it but the state.

namespace {

struct RolloutFeedbackHook {
  RolloutFeedbackDev r;

  __device__ __forceinline__ bool mine(int i) const { return (unsigned)(i - r.first) < (unsigned)r.count; }
  // the evaluation side is the cost hook's (its command side is not used)
  __device__ __forceinline__ RolloutCostHook cost() const {
    return RolloutCostHook{
        RolloutCostDev{nullptr, r.first, r.count, 0, r.cmd_sched, r.cost_sched, r.mode_bits, r.target, r.weight, r.cost, r.tgt_blk, r.tgt_row, r.wt_row}};
  }
  // u = cmd_row + G (ref_row - obs_row) of command block `blk` of this launch into the F_CMD columns, as RolloutRateHook::cmd_row stores
  // a row.  64-bit element offsets: blocks x payload x row width x count passes 2^31.  The gain address is wave-uniform when the gains
  // are shared (gain_lane == 0) and is read with vector loads all the same, as a broadcast, for the reason RolloutCostHook::term gives:
  // scalar loads would hold a gain matrix's worth of scalar registers the kernels do not have.
  template <class SW, class Src>
  __device__ __forceinline__ void fb_row(const SW& sw, const Src& src, int i, int blk, uint32_t w) const {
    const unsigned off8  = (unsigned)i * 8u;
    const int      width = (int)(MRS_RO_HI(w) & 31u);
    const size_t   k     = (size_t)(i - r.first);
    const size_t   ca    = ((size_t)blk * (size_t)r.count + k) * (size_t)r.cmd_stride;
    const size_t   ra    = (size_t)blk * (size_t)r.ref_blk + k * (size_t)r.ref_row;
    const size_t   ga    = (size_t)blk * (size_t)r.gain_blk + k * (size_t)r.gain_lane;
    const uint32_t fbw   = RolloutRateHook::fresh_word(r.fb_word);
    const size_t   g_col = (size_t)r.gain_col, g_row = (size_t)(fbw >> 8) * g_col;
    double         u[F_FF - F_CMD];
    if (MRS_RO_HI(w) & 32u) {
      const float* p = static_cast<const float*>(r.cmd) + ca;
#pragma unroll
      for (int j = 0; j < F_FF - F_CMD; j++) u[j] = j < width ? (double)p[j] : 0.0;
      mrs_obs_row_feedback(src, fbw & 0xFFu, static_cast<const float*>(r.ref) + ra, static_cast<const float*>(r.gain) + ga, g_col, g_row, width, u);
    } else {
      const double* p = static_cast<const double*>(r.cmd) + ca;
#pragma unroll
      for (int j = 0; j < F_FF - F_CMD; j++) u[j] = j < width ? p[j] : 0.0;
      mrs_obs_row_feedback(src, fbw & 0xFFu, static_cast<const double*>(r.ref) + ra, static_cast<const double*>(r.gain) + ga, g_col, g_row, width, u);
    }
#pragma unroll
    for (int j = 0; j < F_FF - F_CMD; j++)
      if (j < width) sw.st(F_CMD + j, off8, u[j]);
  }
  template <class SW>
  __device__ __forceinline__ void cmd(const SW&, int, int) const {}
  // top of sub-step s: the command of the block that starts here, from the state before the sub-step; inside a block the columns hold
  // the command as they stand (the feedback is sampled at the command rate).  A launch in which no block starts has width 0.
  template <class SW, class PT>
  __device__ __forceinline__ void cmd_lane(const SW& sw, PT& P, int i, const Lane& L, int s) const {
    if (!mine(i)) return;
    const uint32_t w = RolloutRateHook::fresh_word(r.cmd_sched);
    const int      j = RolloutRateHook::due(w, s);
    if ((MRS_RO_HI(w) & 31u) == 0u || j < 0) return;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, P.n_motors, s == 0};
    fb_row(sw, src, i, j, w);
  }
  template <class SW, class PT>
  __device__ __forceinline__ void obs(const SW& sw, PT& P, int i, const Lane& L, int s) const {
    cost().obs(sw, P, i, L, s);
  }
  // once per lane (RolloutCostHook::enter): a UAV on hold is not stepped, but the loop this call stands for still forms and writes its
  // commands from its unchanged state, of which the one of the last block that starts in this launch stays, and evaluates its cost
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int substeps) const {
    if (!mine(i)) return false;
    L.flags = (L.flags & ~FLAG_MODE_MASK) | r.mode_bits;
    if (!(L.flags & FLAG_HOLD)) return false;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[L.flags >> FLAG_TYPE_SHIFT].n_motors, true};
    if ((MRS_RO_HI(r.cmd_sched) & 31u) != 0u) {
      const int starts = RolloutRateHook::due_count(r.cmd_sched, substeps);
      if (starts > 0) fb_row(sw, src, i, starts - 1, r.cmd_sched);
    }
    if (MRS_RO_HI(r.cost_sched) != 0u) {
      const RolloutCostHook ch   = cost();
      const int             ends = RolloutRateHook::due_count(r.cost_sched, substeps);
      double*               c    = r.cost + (size_t)(i - r.first);
      double                sum  = *c;
      for (int b = 0; b < ends; b++) sum = sum + ch.term(src, i, b, MRS_RO_HI(r.cost_sched), r.cmd_sched);
      *c = sum;
    }
    sw.F[i] = L.flags;
    return true;
  }
};

}  // namespace

// The five shapes of rollout_device.inc a fifth time.  The launch bounds are this file's own: they start from those chosen there.
#define MRS_ROLLOUT_FEEDBACK_KERNEL(name, bounds, CASCADE, UNIFORM, BUF)                                                              \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, int substeps, RolloutFeedbackDev r) { \
    const CollDev none{};                                                                                                          \
    int  blk_;                                                                                                                     \
    bool took_;                                                                                                                    \
    step_kernel_body<CASCADE, UNIFORM, 1, true, MRS_SU, false, false, false>(SwarmAcc<BUF>(sw), dt, inv_dt, substeps, none, blk_, took_, \
                                                                             RolloutFeedbackHook{r});                              \
  }
MRS_ROLLOUT_FEEDBACK_KERNEL(mrs_uav_rollout_feedback, (64, 1), true, true, false)
MRS_ROLLOUT_FEEDBACK_KERNEL(mrs_uav_rollout_feedback_buf, (64, 1), true, true, true)
MRS_ROLLOUT_FEEDBACK_KERNEL(mrs_uav_model_rollout_feedback, (64, 1), false, true, false)
MRS_ROLLOUT_FEEDBACK_KERNEL(mrs_uav_model_rollout_feedback_buf, (64, MRS_WAVES_PER_SIMD), false, true, true)
MRS_ROLLOUT_FEEDBACK_KERNEL(mrs_uav_rollout_feedback_mixed, (64), true, false, false)
#undef MRS_ROLLOUT_FEEDBACK_KERNEL

// n_steps steps of the whole swarm with the rows of `r` (whose cmd / gain / ref / target / weight point at row block 0, whose schedule
// words hold the width, dtype and groups of the call, and whose block and row distances are the call's; the schedule bits and first
// blocks are set here, per launch, as mrs_launch_rollout_cost sets them): command block j starts at step j * cmd_every and brings its
// gain and setpoint blocks with it (gain_blk / ref_blk 0: one block serves the call), evaluation j falls behind step
// (j + 1) * cost_every - 1 (cost_sched without groups: no evaluation at all).  variant and the buffer / pointer choice as
// mrs_launch_rollout_rate.
extern "C" hipError_t KNAME(mrs_launch_rollout_feedback)(SwarmDev sw, RolloutFeedbackDev r, double dt, int n_steps, int cmd_every, int cost_every,
                                                         int variant, hipStream_t st) {
  static_assert(kRolloutMaxSteps <= 64, "a launch's schedule: s0 < 64, p <= 64 (RolloutRateDev)");
  const int nb = (sw.n + 63) / 64;
  if (nb <= 0 || n_steps <= 0 || cmd_every <= 0 || cost_every <= 0) return hipSuccess;
  sw.blk0 = 0;
  const dim3               g(nb), b(64);
  const double             inv_dt = 1.0 / dt;
  static const bool        no_buf = getenv("MRS_NO_BUFFER_ADDRESSING") != nullptr;
  const bool               buf    = !no_buf && (unsigned long long)F_COUNT * (unsigned long long)sw.npad * 8ull < (1ull << 32);
  const RolloutFeedbackDev call   = r;
  const size_t             elem   = (MRS_RO_HI(call.cmd_sched) & 32u) ? sizeof(float) : sizeof(double);
  for (int t0 = 0; t0 < n_steps; t0 += kRolloutMaxSteps) {
    const int sub = n_steps - t0 < kRolloutMaxSteps ? n_steps - t0 : kRolloutMaxSteps;
    // the first sub-step that starts a command block, and the first an evaluation falls behind; none in this launch: width / groups 0
    const int       cs0 = (cmd_every - t0 % cmd_every) % cmd_every, es0 = cost_every - 1 - t0 % cost_every;
    const long long cb0 = ((long long)t0 + cs0) / cmd_every, eb0 = t0 / cost_every;
    r.cmd_sched  = cs0 < sub ? (call.cmd_sched & 0xFF000000u) | mrs_ro_sched(cs0, cmd_every) : (call.cmd_sched & (32u << 24));
    r.cost_sched = es0 < sub ? (call.cost_sched & 0xFF000000u) | mrs_ro_sched(es0, cost_every) : 0u;
    r.cmd    = !call.cmd ? nullptr : static_cast<const char*>(call.cmd) + (size_t)cb0 * (size_t)call.count * (size_t)call.cmd_stride * elem;
    r.gain   = !call.gain ? nullptr : static_cast<const char*>(call.gain) + (size_t)cb0 * (size_t)call.gain_blk * elem;
    r.ref    = !call.ref ? nullptr : static_cast<const char*>(call.ref) + (size_t)cb0 * (size_t)call.ref_blk * elem;
    r.target = !call.target ? nullptr : static_cast<const char*>(call.target) + (size_t)eb0 * (size_t)call.tgt_blk * elem;
    r.weight = !call.weight ? nullptr : static_cast<const char*>(call.weight) + (size_t)eb0 * (size_t)call.wt_row * elem;
    if (variant == 1) {
      if (buf)
        hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout_feedback_buf), g, b, 0, st, sw, dt, inv_dt, sub, r);
      else
        hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout_feedback), g, b, 0, st, sw, dt, inv_dt, sub, r);
    } else {
      if (buf)
        hipLaunchKernelGGL(KNAME(mrs_uav_rollout_feedback_buf), g, b, 0, st, sw, dt, inv_dt, sub, r);
      else
        hipLaunchKernelGGL(KNAME(mrs_uav_rollout_feedback), g, b, 0, st, sw, dt, inv_dt, sub, r);
    }
    if (sw.n_mixed > 0) hipLaunchKernelGGL(KNAME(mrs_uav_rollout_feedback_mixed), dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, sub, r);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
