// rollout_tick_feedback_device.inc — feedback tick rollouts (mrs_swarm_rollout_tick_feedback_device): the four single-GPU *_coll kernels
// of step_device.inc once more, with a hook that, where the cost tick hook reads the command row block starting at this tick, FORMS the
// command from the state the lane holds:  cmd_row + G · (ref_row − obs_row),  obs_row being the FP64 observation row of fb_groups BEFORE
// the step (obs_row.h: mrs_obs_row_feedback over the lane's registers, as the feedback rollouts), and whose evaluation side is the cost
// tick hook's, word for word.  One launch is one tick of timerMain (src/multirotor_simulator.cpp:211-217): the collision tick that
// followed the previous step is evaluated from the neighbour lists (:295-359), then makeStep.
//
// Where the command is formed.  The loop this call stands for gathers the row before the step, with the collision tick of the previous
// tick still pending; the fused launch forms it in enter(), ahead of MRS_COLLIDE_EVAL.  Both see the same row: the evaluation writes the
// F_FEXT columns and the crash bit of the flag word and nothing else (step_device.inc: MRS_COLLIDE_EVAL), and no observation group reads
// either (obs_row.h: position, velocity, attitude, body rates, the IMU column and the rpm columns).  What a row holds before the step:
// the state registers of the prologue, the IMU column as the launch before (or the caller) left it, the rpm columns likewise.  The
// feedback has no memory: a launch needs nothing of the launch before it but the state.
//
// Replay.  A no-op launch (stale lists) leaves before any hook call: it writes no command, adds nothing and leaves the state alone.  The
// host replays it with the same descriptor; the replayed launch sees the state the no-op left, forms the same command and adds once.
// The host zeroes the cost vector once, in front of the call's first launch and outside the launch log (unless the call accumulates).
//
// A tick without the fused form is one step of the feedback rollout kernels with this tick's pointers followed by the crash add
// (tick_single.hip), and gives the same bits: the law and the two adds round alike in every kernel and in both step units.
//
// Included behind rollout_cost_device.inc (LaneObs, the feedback arithmetic's users) and in front of rollout_tick_cost_device.inc.  The
// host computes each tick's pointers; the hook reads its descriptor where it needs it through the kernel-argument segment, as the kernels
// read CollDev (fresh(), CollKernArgs): the descriptor sits BEHIND CollDev and does not move it.

namespace {

typedef const __attribute__((address_space(4))) RolloutTickFeedbackDev CRolloutTickFeedbackDev;
DEV CRolloutTickFeedbackDev& fresh(CRolloutTickFeedbackDev& r) {
  CRolloutTickFeedbackDev* q = &r;
  asm volatile("" : "+s"(q));
  return *q;
}
struct RolloutTickFeedbackKernArgs {  // layout of the kernels' argument segment: CollKernArgs, then the descriptor
  SwarmDev               sw;
  double                 dt, inv_dt;
  CollDev                cd;
  RolloutTickFeedbackDev r;
};
static_assert(offsetof(RolloutTickFeedbackKernArgs, cd) == offsetof(CollKernArgs, cd), "the descriptor must not move CollDev");

struct RolloutTickFeedbackHook {
  CRolloutTickFeedbackDev* r0;

  // rows of FP32 / FP64 elements: 64-bit element offsets (count x stride passes 2^31)
  static __device__ __forceinline__ size_t at(int k, int stride) { return (size_t)k * (size_t)stride; }

  // Once per lane, behind the wave-uniform exits (a no-op launch never gets here) and ahead of the collision evaluation: the range takes
  // the new mode, and the command of a block that starts at this tick is formed from the registers of the prologue (the IMU is the
  // column's: one launch is one step) and goes into the F_CMD columns AND into the registers the prologue preloaded from those columns,
  // as in the tick rollout's hook.  Held and crashed UAVs get their commands, formed from their state as it stands, like every other UAV
  // of the range.  The gain address is wave-uniform when the gains are shared (gain_lane 0, gain_col 1) and is read with vector loads
  // all the same, as a broadcast; per-UAV gains are UAV-minor (gain_col = count), one coalesced request per gain element and wave.
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int) const {
    CRolloutTickFeedbackDev& r = fresh(*r0);
    const int                k = i - r.first;
    if ((unsigned)k >= (unsigned)r.count) return false;
    L.flags = (L.flags & ~FLAG_MODE_MASK) | r.mode_bits;
    if (!r.cmd) return false;  // (wave-uniform) inside a held command block the columns hold the command as they stand
    const unsigned    off8  = (unsigned)i * 8u;
    const int         width = (int)(r.cmd_word & 31u);
    const uint32_t    fbw   = r.fb_word;
    const size_t      ca = at(k, r.cmd_stride), ra = at(k, r.ref_row), ga = at(k, r.gain_lane);
    const size_t      g_col = (size_t)r.gain_col, g_row = (size_t)(fbw >> 8) * g_col;
    const LaneObs<SW> src{sw, L, off8, sw.T[L.flags >> FLAG_TYPE_SHIFT].n_motors, true};
    double            u[F_FF - F_CMD];
    if (r.cmd_word & 32u) {
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
      if (j < width) {
        sw.st(F_CMD + j, off8, u[j]);
        if (j < 4) L.pre_cmd[j] = u[j];
      }
    return false;
  }
  template <class SW>
  __device__ __forceinline__ void cmd(const SW&, int, int) const {}
  template <class SW, class PT>
  __device__ __forceinline__ void cmd_lane(const SW&, PT&, int, const Lane&, int) const {}

  // The evaluation of UAV first + k, RolloutTickCostHook::eval restated on this descriptor (a shared text would be a template over the
  // descriptor type, and the cost tick kernels are kept as they compile today): the term, the lane's cost element, the two adds, the
  // store.  Target and weight are read with vector loads, a shared row as a broadcast; the dtype is a wave-uniform branch.
  template <class Src>
  __device__ __forceinline__ void eval(CRolloutTickFeedbackDev& r, const Src& src, int k, uint32_t flags) const {
#pragma clang fp contract(off)
    double* const c   = r.cost + (size_t)k;
    double        sum = *c;
    if (r.groups != 0u) {  // (wave-uniform)
      const size_t ta = at(k, r.tgt_row);
      double       t;
      if (r.cmd_word & 32u)
        t = mrs_obs_row_cost(src, r.groups, static_cast<const float*>(r.target) + ta, static_cast<const float*>(r.weight));
      else
        t = mrs_obs_row_cost(src, r.groups, static_cast<const double*>(r.target) + ta, static_cast<const double*>(r.weight));
      sum = sum + mrs_unfused(t);
    }
    // performed whenever the flag is set, whatever crash_cost is (0, negative, non-finite)
    if (flags & FLAG_CRASHED) sum = mrs_unfused(sum) + r.crash_cost;
    *c = sum;
  }
  // After post_step: the lane's flag word holds every collision up to the previous tick — UavSystem::hasCrashed at the instant the cost
  // tick rollout evaluates, before this tick's handleCollisions.
  template <class SW, class PT>
  __device__ __forceinline__ void obs(const SW& sw, PT& P, int i, const Lane& L, int) const {
    CRolloutTickFeedbackDev& r = fresh(*r0);
    const int                k = i - r.first;
    if ((unsigned)k >= (unsigned)r.count) return;
    if (!r.cost) return;  // (wave-uniform) no evaluation ends with this tick
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, P.n_motors, false};
    eval(r, src, k, L.flags);
  }
  // A UAV on hold is not iterated but takes part in the collisions: enter() has formed and written its command from its unchanged
  // state; the last thing its lane does is the flag word with the new mode and the evaluation of that state (the IMU is the column's),
  // with the crash add if this tick's evaluation or an earlier one set its flag.  `fl` as in the tick rollout's hook.
  template <class SW>
  __device__ __forceinline__ void held(const SW& sw, int i, const Lane& L, uint32_t fl) const {
    CRolloutTickFeedbackDev& r = fresh(*r0);
    const int                k = i - r.first;
    if ((unsigned)k >= (unsigned)r.count) return;
    fl      = (fl & ~FLAG_MODE_MASK) | r.mode_bits;
    sw.F[i] = fl;
    if (!r.cost) return;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[fl >> FLAG_TYPE_SHIFT].n_motors, true};
    eval(r, src, k, fl);
  }
};

}  // namespace

// The four single-GPU *_coll shapes of step_device.inc (COLL, not SHARD, one step), with their launch bounds and accessors.
#define MRS_ROLLOUT_TICK_FEEDBACK_KERNEL(name, bounds, CASCADE, UNIFORM, ACC, SU)                                                     \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, CollDev /*read in place*/,  \
                                                                  RolloutTickFeedbackDev /*read in place*/) {                         \
    typedef const __attribute__((address_space(4))) char CChar;                                                                       \
    CChar*    args = (CChar*)__builtin_amdgcn_kernarg_segment_ptr();                                                                  \
    CCollDev* cdk  = (CCollDev*)(args + offsetof(RolloutTickFeedbackKernArgs, cd));                                                   \
    int       blk_;                                                                                                                   \
    bool      took_;                                                                                                                  \
    step_kernel_body<CASCADE, UNIFORM, 1, false, SU, true, false, false>(                                                             \
        ACC(sw), dt, inv_dt, 1, *cdk, blk_, took_,                                                                                    \
        RolloutTickFeedbackHook{(CRolloutTickFeedbackDev*)(args + offsetof(RolloutTickFeedbackKernArgs, r))});                        \
  }
MRS_ROLLOUT_TICK_FEEDBACK_KERNEL(mrs_uav_rollout_tick_feedback_buf, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccBuf, MRS_SU)
MRS_ROLLOUT_TICK_FEEDBACK_KERNEL(mrs_uav_model_rollout_tick_feedback_buf, (64, MRS_WAVES_PER_SIMD), false, true, SwarmAccBuf, MRS_SU)
MRS_ROLLOUT_TICK_FEEDBACK_KERNEL(mrs_uav_rollout_tick_feedback, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccPtr, MRS_SU)
MRS_ROLLOUT_TICK_FEEDBACK_KERNEL(mrs_uav_rollout_tick_feedback_mixed, (64, MRS_WAVES_PER_SIMD), true, false, SwarmAccPtr, MRS_SU)
#undef MRS_ROLLOUT_TICK_FEEDBACK_KERNEL

// One tick of the whole swarm: the fused step + collision-evaluation launch of mrs_launch_step_coll (single GPU) with the command and the
// evaluation of `r`.  variant and the buffer / pointer choice as there (rollout_buffer_addressing).
extern "C" hipError_t KNAME(mrs_launch_rollout_tick_feedback)(SwarmDev sw, CollDev cd, RolloutTickFeedbackDev r, double dt, int variant,
                                                              hipStream_t st) {
  const int nb = (sw.n + 63) / 64;
  if (nb <= 0) return hipSuccess;
  sw.blk0 = 0;
  const dim3   g(nb), b(64);
  const double inv_dt = 1.0 / dt;
  const bool   buf    = rollout_buffer_addressing(sw);
  if (buf && variant == 1)
    hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout_tick_feedback_buf), g, b, 0, st, sw, dt, inv_dt, cd, r);
  else if (buf)
    hipLaunchKernelGGL(KNAME(mrs_uav_rollout_tick_feedback_buf), g, b, 0, st, sw, dt, inv_dt, cd, r);
  else
    hipLaunchKernelGGL(KNAME(mrs_uav_rollout_tick_feedback), g, b, 0, st, sw, dt, inv_dt, cd, r);
  if (sw.n_mixed > 0) hipLaunchKernelGGL(KNAME(mrs_uav_rollout_tick_feedback_mixed), dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, cd, r);
  return hipGetLastError();
}
