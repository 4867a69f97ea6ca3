// rollout_cost_device.inc — cost rollouts (mrs_swarm_rollout_cost_device) and feedback rollouts (mrs_swarm_rollout_feedback_device).
//
// A cost rollout is a control-rate rollout whose hook, where the rate hook writes an observation row, compares the row's FP64 values with
// a target row and adds the weighted squared distance to the UAV's element of a cost vector.  A sampling-based planner wants one number
// per sample back from a horizon: the row never leaves the registers, and a call stores 8 B per UAV and evaluation where the rate
// rollout stores a row.
//
// The running sum crosses sub-steps and launches in memory: at every due sub-step the lane reads its cost element, adds the term and
// stores it (the element belongs to one lane; launches follow each other in stream order).  The host zeroes the vector in front of
// the first launch unless the call accumulates, so the kernels know one case only, and the sum is the same however the call is cut
// into launches.
//
// A feedback rollout is a cost rollout whose hook, where the cost hook reads a command row, FORMS the command from the state the lane
// holds: at the top of the sub-step that starts command block b the F_CMD columns take  cmd_row + G · (ref_row − obs_row),  obs_row
// being the FP64 observation row of fb_groups BEFORE the step (obs_row.h: mrs_obs_row_feedback).  A caller whose samples are
// controllers (a gain per UAV, a nominal command plus time-varying gains, one law over many initial states) closes the loop inside the
// launch instead of through a gather, a matrix product and a set_input per tick.  The cost side is the cost hook's, word for word.
//
// The values an observation row holds BEFORE sub-step s: the state registers; the IMU of the previous sub-step's post_step, and at
// sub-step 0 the IMU column (what the launch before, or the caller, left there); the rpm columns as the previous sub-step's motor
// stage stored them.  The feedback has no memory: a launch needs nothing of the launch before it but the state.
//
// Included behind rollout_rate_device.inc (RolloutHookBase, MRS_ROLLOUT_FAMILY, launch_rollout).  Two families with kernels of their
// own, for the reason given in rollout_device.inc: no other rollout call pays for the targets, and none for the gains.

namespace {

struct RolloutCostHook : RolloutHookBase<RolloutCostDev> {
  // the command side is the rate hook's, word for word
  __device__ __forceinline__ RolloutRateHook rate() const {
    return RolloutRateHook{{RolloutRateDev{r.cmd, nullptr, r.first, r.count, r.cmd_stride, 0, r.cmd_sched, 0u, r.mode_bits}}};
  }
  template <class SW>
  __device__ __forceinline__ void cmd(const SW& sw, int i, int s) const {
    rate().cmd(sw, i, s);
  }
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
    const uint32_t w = fresh_word(r.cost_sched);
    const int      j = mrs_ro_due(w, s);
    if (MRS_RO_HI(w) == 0u || j < 0) return;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, P.n_motors, false};
    double*           c = r.cost + (size_t)(i - r.first);
    const double      t = term(src, i, j, MRS_RO_HI(w), fresh_word(r.cmd_sched));
    *c                  = *c + t;
  }
  // once per lane (RolloutRateHook::enter): a UAV on hold is not stepped, but the loop this call stands for still writes its commands
  // and evaluates its unchanged state: one term per evaluation that falls into this launch, added in order
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int substeps) const {
    if (!held(i, L)) return false;
    const int starts = mrs_ro_due_count(r.cmd_sched, substeps);
    if (starts > 0) rate().cmd_row(sw, i, starts - 1, r.cmd_sched);
    if (MRS_RO_HI(r.cost_sched) != 0u) {
      const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[L.flags >> FLAG_TYPE_SHIFT].n_motors, true};
      const int         ends = mrs_ro_due_count(r.cost_sched, substeps);
      double*           c    = r.cost + (size_t)(i - r.first);
      double            sum  = *c;
      for (int b = 0; b < ends; b++) sum = sum + term(src, i, b, MRS_RO_HI(r.cost_sched), r.cmd_sched);
      *c = sum;
    }
    return held_done(sw, i, L);
  }
};

struct RolloutFeedbackHook : RolloutHookBase<RolloutFeedbackDev> {
  // the evaluation side is the cost hook's (its command side is not used)
  __device__ __forceinline__ RolloutCostHook cost() const {
    return RolloutCostHook{
        {RolloutCostDev{nullptr, r.first, r.count, 0, r.cmd_sched, r.cost_sched, r.mode_bits, r.target, r.weight, r.cost, r.tgt_blk, r.tgt_row, r.wt_row}}};
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
    const uint32_t fbw   = fresh_word(r.fb_word);
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
    const uint32_t w = fresh_word(r.cmd_sched);
    const int      j = mrs_ro_due(w, s);
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
    if (!held(i, L)) return false;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[L.flags >> FLAG_TYPE_SHIFT].n_motors, true};
    if ((MRS_RO_HI(r.cmd_sched) & 31u) != 0u) {
      const int starts = mrs_ro_due_count(r.cmd_sched, substeps);
      if (starts > 0) fb_row(sw, src, i, starts - 1, r.cmd_sched);
    }
    if (MRS_RO_HI(r.cost_sched) != 0u) {
      const RolloutCostHook ch   = cost();
      const int             ends = mrs_ro_due_count(r.cost_sched, substeps);
      double*               c    = r.cost + (size_t)(i - r.first);
      double                sum  = *c;
      for (int b = 0; b < ends; b++) sum = sum + ch.term(src, i, b, MRS_RO_HI(r.cost_sched), r.cmd_sched);
      *c = sum;
    }
    return held_done(sw, i, L);
  }
};

}  // namespace

MRS_ROLLOUT_FAMILY(_cost, RolloutCostDev, RolloutCostHook)
MRS_ROLLOUT_FAMILY(_feedback, RolloutFeedbackDev, RolloutFeedbackHook)

// The launchers below take `r` with its row pointers at row block 0, with the width, dtype and groups of the call in the top bytes of
// its schedule words and with the call's block and row distances, and give each launch its schedule bits and the rows of its first due
// blocks (mrs_ro_launch_sched): command block j starts at step j * cmd_every, evaluation j falls behind step (j + 1) * cost_every - 1.
// r.cost must hold the sums the call starts from.  variant as launch_rollout's.

// the command and the evaluation side of a launch; returns the call's block of the launch's first due command
template <class Dev>
static long long rollout_cost_launch(Dev& l, int t0, int sub, int cmd_every, int cost_every) {
  const size_t        elem = (MRS_RO_HI(l.cmd_sched) & 32u) ? sizeof(float) : sizeof(double);
  const mrs_ro_launch c = mrs_ro_launch_sched(l.cmd_sched, t0, sub, cmd_every, true), e = mrs_ro_launch_sched(l.cost_sched, t0, sub, cost_every, false);
  l.cmd_sched = c.word, l.cost_sched = e.word;
  l.cmd    = rollout_rows(l.cmd, c.blk0, (size_t)l.count * (size_t)l.cmd_stride, elem);
  l.target = rollout_rows(l.target, e.blk0, (size_t)l.tgt_blk, elem);
  l.weight = rollout_rows(l.weight, e.blk0, (size_t)l.wt_row, elem);
  return c.blk0;
}

extern "C" hipError_t KNAME(mrs_launch_rollout_cost)(SwarmDev sw, RolloutCostDev r, double dt, int n_steps, int cmd_every, int cost_every, int variant,
                                                     hipStream_t st) {
  if (cmd_every <= 0 || cost_every <= 0) return hipSuccess;
  return launch_rollout(KNAME(k_rollout_cost), sw, r, dt, n_steps, variant, st,
                        [=](RolloutCostDev& l, int t0, int sub) { rollout_cost_launch(l, t0, sub, cmd_every, cost_every); });
}

// A command block brings its gain and setpoint blocks with it (gain_blk / ref_blk 0: one block serves the call); cost_sched without
// groups: no evaluation at all.
extern "C" hipError_t KNAME(mrs_launch_rollout_feedback)(SwarmDev sw, RolloutFeedbackDev r, double dt, int n_steps, int cmd_every, int cost_every,
                                                         int variant, hipStream_t st) {
  if (cmd_every <= 0 || cost_every <= 0) return hipSuccess;
  return launch_rollout(KNAME(k_rollout_feedback), sw, r, dt, n_steps, variant, st, [=](RolloutFeedbackDev& l, int t0, int sub) {
    const size_t    elem = (MRS_RO_HI(l.cmd_sched) & 32u) ? sizeof(float) : sizeof(double);
    const long long cb0  = rollout_cost_launch(l, t0, sub, cmd_every, cost_every);
    l.gain = rollout_rows(l.gain, cb0, (size_t)l.gain_blk, elem);
    l.ref  = rollout_rows(l.ref, cb0, (size_t)l.ref_blk, elem);
  });
}
