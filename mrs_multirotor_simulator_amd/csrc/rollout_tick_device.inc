// rollout_tick_device.inc — the tick rollout families: tick rollouts (mrs_swarm_rollout_tick_device), cost tick rollouts
// (mrs_swarm_rollout_tick_cost_device) and feedback tick rollouts (mrs_swarm_rollout_tick_feedback_device).  Each family is the four
// single-GPU *_coll kernels of step_device.inc once more, with a hook.  One launch is one tick of timerMain
// (src/multirotor_simulator.cpp:211-217): the collision tick that followed the previous step is evaluated from the neighbour lists
// (:295-359), then makeStep; what a hook writes is what `setInput; makeStep; getState / hasCrashed` see (uav_system.hpp:175-248,
// :304-380, :386), before this tick's handleCollisions.
//   tick      reads the command row block that starts at this tick, writes the observation and crash row blocks that end with it;
//   cost      reads the command rows alike and, where the tick hook writes a row and a crash byte, adds to one FP64 number per UAV: the
//             weighted squared distance of the row from a target row (obs_row.h: mrs_obs_row_cost over the lane's registers, as the cost
//             rollouts), and behind it crash_cost when the UAV's crash flag is set.  No row and no crash byte leaves the registers;
//   feedback  evaluates as the cost hook does and FORMS the command from the state the lane holds:  cmd_row + G · (ref_row − obs_row),
//             obs_row being the FP64 observation row of fb_groups BEFORE the step (obs_row.h: mrs_obs_row_feedback, as the feedback
//             rollouts).
//
// Included last, behind rollout_cost_device.inc (LaneObs, the feedback arithmetic's users).  The host computes each tick's pointers
// (tick_single.hip), so the hooks have no schedule words; a hook reads its descriptor where it needs it through the kernel-argument
// segment, as the kernels read CollDev (fresh(), CollKernArgs): the descriptor sits BEHIND CollDev and does not move it.
//
// Replay.  A no-op launch (stale lists) leaves before any hook call: it writes nothing into the caller's rows, writes no command, adds
// nothing, does not touch the cost element and leaves the state alone.  The host replays it with the same descriptor.  The cost element
// is read, added to and stored, so a launch must add exactly once: the replayed launch does, and the host zeroes the vector once, in
// front of the call's first launch and outside the launch log (unless the call accumulates), so a replay does not zero again.  The sum
// is that of the loop whatever stalls inside the call.  The feedback has no memory — a launch needs nothing of the launch before it
// but the state — so the replayed launch sees the state the no-op left, forms the same command and adds once.
//
// The two adds of an evaluation are two FP64 additions with a rounding each, the term first, in both step units, and the feedback law
// rounds alike in every kernel: a tick without the fused form is one step of the rate, cost or feedback rollout kernels with this
// tick's pointers, followed by the crash bytes or the one-lane-per-UAV crash add (tick_single.hip, device_io.hip), and gives the same
// rows and the same bits.
//
// Where the feedback command is formed.  The loop the call stands for gathers the row before the step, with the collision tick of the
// previous tick still pending; the fused launch forms it in enter(), ahead of MRS_COLLIDE_EVAL.  Both see the same row: the evaluation
// writes the F_FEXT columns and the crash bit of the flag word and nothing else (step_device.inc: MRS_COLLIDE_EVAL), and no
// observation group reads either (obs_row.h: position, velocity, attitude, body rates, the IMU column and the rpm columns).  What a
// row holds before the step: the state registers of the prologue, the IMU column as the launch before (or the caller) left it, the rpm
// columns likewise.

namespace {

// What the tick hooks hold and do alike.  Dev is the family's descriptor (swarm_layout.h: RolloutTickDev, RolloutTickCostDev,
// RolloutTickFeedbackDev), which name the range (first, count), the command rows (cmd, cmd_stride, cmd_word) and mode_bits alike, and
// the two costed ones the evaluation (target, weight, cost, tgt_row, groups, crash_cost).  A member is compiled for the families that
// call it.  As in RolloutHookBase the call structure is flat: enter, obs and held call the helpers below and nothing forwards in
// between, and their range test and their stores stand in their own bodies: with the head of held() (range test, mode bits, the store
// of the flag word) behind a call that answers "inside the range" the kernels got a second exec region and other code.
template <class Dev>
struct RolloutTickHookBase {
  typedef const __attribute__((address_space(4))) Dev CDev;
  static constexpr bool kOnCollKernels = true;  // rides on the single-GPU COLL kernels (step_kernel_body's static_assert)
  CDev* r0;                                     // into the kernel-argument segment

  static __device__ __forceinline__ CDev& fresh(CDev& r) {
    CDev* q = &r;
    asm volatile("" : "+s"(q));
    return *q;
  }
  // rows of FP32 / FP64 elements: 64-bit element offsets (count x stride passes 2^31)
  static __device__ __forceinline__ size_t at(int k, int stride) { return (size_t)k * (size_t)stride; }
  static __device__ __forceinline__ bool   mine(CDev& r, int k) { return (unsigned)k < (unsigned)r.count; }

  // the flag word of a UAV of the range: it takes the new mode
  static __device__ __forceinline__ uint32_t with_mode(CDev& r, uint32_t flags) { return (flags & ~FLAG_MODE_MASK) | r.mode_bits; }
  // a command row: FP32 is widened exactly
  template <class T>
  static __device__ __forceinline__ void cmd_row(const T* p, int width, double (&c)[F_FF - F_CMD]) {
#pragma unroll
    for (int j = 0; j < F_FF - F_CMD; j++)
      if (j < width) c[j] = (double)p[j];
  }
  // the command into the F_CMD columns (mrs_swarm_set_input_device's k_scatter_cmd) AND into the registers the prologue preloaded from
  // those columns, which the cascade and the motor stage read instead
  template <class SW>
  static __device__ __forceinline__ void cmd_store(const SW& sw, unsigned off8, Lane& L, int width, const double (&c)[F_FF - F_CMD]) {
#pragma unroll
    for (int j = 0; j < F_FF - F_CMD; j++)
      if (j < width) {
        sw.st(F_CMD + j, off8, c[j]);
        if (j < 4) L.pre_cmd[j] = c[j];
      }
  }
  // Once per lane, behind the wave-uniform exits (a no-op launch never gets here): the range takes the new mode (the flag word is stored
  // behind the step as any flag change is), and the command row of a block that starts at this tick goes into the columns and the
  // registers.  Held and crashed UAVs get their commands like every other UAV of the range.
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int) const {
    CDev&     r = fresh(*r0);
    const int k = i - r.first;
    if (!mine(r, k)) return false;
    L.flags = with_mode(r, L.flags);
    if (!r.cmd) return false;  // (wave-uniform) inside a held command block the columns hold the command as they stand
    const unsigned off8  = (unsigned)i * 8u;
    const int      width = (int)(r.cmd_word & 31u);
    const size_t   a     = at(k, r.cmd_stride);
    double         c[F_FF - F_CMD];
    if (r.cmd_word & 32u)
      cmd_row(static_cast<const float*>(r.cmd) + a, width, c);
    else
      cmd_row(static_cast<const double*>(r.cmd) + a, width, c);
    cmd_store(sw, off8, L, width, c);
    return false;
  }
  template <class SW>
  __device__ __forceinline__ void cmd(const SW&, int, int) const {}
  template <class SW, class PT>
  __device__ __forceinline__ void cmd_lane(const SW&, PT&, int, const Lane&, int) const {}

  // The evaluation of UAV first + k: the term, the lane's cost element, the two adds, the store.  The target address is per lane
  // (tgt_row == 0: the same for every lane) and the weight address is wave-uniform; both are read with vector loads, a shared row as a
  // broadcast (scalar loads would hold a row's worth of scalar registers the kernels do not have).  The dtype is a wave-uniform branch.
  template <class Src>
  static __device__ __forceinline__ void tick_eval(CDev& r, const Src& src, int k, uint32_t flags) {
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
};

// obs() runs after post_step: the collision evaluation has had its chance in either crash mode (before the cascade, or between the
// cascade and the motors), so the lane's flag word holds every collision up to the previous tick — UavSystem::hasCrashed at the instant
// the row is taken or the cost evaluated, before this tick's handleCollisions.

// held(): a UAV on hold is not iterated but takes part in the collisions: the last thing its lane does, behind the evaluation and the
// position records, is the flag word with the new mode and what the hook writes of its unchanged state (the IMU is the column's).  `fl`
// is the word the kernel keeps for a held UAV: the one it loaded, and the crash bit of this evaluation (nothing else of the UAV changes
// — the lane's own copy has already dropped FLAG_VPREV_SPLIT for a step that does not happen).

// Its own: the observation row and the crash byte of UAV first + k.
struct RolloutTickHook : RolloutTickHookBase<RolloutTickDev> {
  template <class Src>
  static __device__ __forceinline__ void rows(CDev& r, const Src& src, int k, uint32_t flags) {
    if (r.obs) {
      const size_t a = at(k, r.obs_stride);
      if (r.cmd_word & 32u)
        mrs_obs_row(src, r.groups, static_cast<float*>(r.obs) + a);
      else
        mrs_obs_row(src, r.groups, static_cast<double*>(r.obs) + a);
    }
    if (r.crashed) r.crashed[k] = (flags & FLAG_CRASHED) ? 1 : 0;
  }
  template <class SW, class PT>
  __device__ __forceinline__ void obs(const SW& sw, PT& P, int i, const Lane& L, int) const {
    CDev&     r = fresh(*r0);
    const int k = i - r.first;
    if (!mine(r, k)) return;
    if (!r.obs && !r.crashed) return;  // (wave-uniform) no block ends with this tick
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, P.n_motors, false};
    rows(r, src, k, L.flags);
  }
  template <class SW>
  __device__ __forceinline__ void held(const SW& sw, int i, const Lane& L, uint32_t fl) const {
    CDev&     r = fresh(*r0);
    const int k = i - r.first;
    if (!mine(r, k)) return;
    fl      = with_mode(r, fl);
    sw.F[i] = fl;
    if (!r.obs && !r.crashed) return;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[fl >> FLAG_TYPE_SHIFT].n_motors, true};
    rows(r, src, k, fl);
  }
};

// The evaluation side of the two costed families: tick_eval where the tick hook writes its rows, for a held UAV with the crash add if
// this tick's evaluation or an earlier one set its flag.  The cost tick hook is this and the base's command row.
template <class Dev>
struct RolloutTickEvalHook : RolloutTickHookBase<Dev> {
  typedef RolloutTickHookBase<Dev> Base;
  typedef typename Base::CDev      CDev;
  template <class SW, class PT>
  __device__ __forceinline__ void obs(const SW& sw, PT& P, int i, const Lane& L, int) const {
    CDev&     r = Base::fresh(*this->r0);
    const int k = i - r.first;
    if (!Base::mine(r, k)) return;
    if (!r.cost) return;  // (wave-uniform) no evaluation ends with this tick (or in the whole call)
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, P.n_motors, false};
    Base::tick_eval(r, src, k, L.flags);
  }
  template <class SW>
  __device__ __forceinline__ void held(const SW& sw, int i, const Lane& L, uint32_t fl) const {
    CDev&     r = Base::fresh(*this->r0);
    const int k = i - r.first;
    if (!Base::mine(r, k)) return;
    fl      = Base::with_mode(r, fl);
    sw.F[i] = fl;
    if (!r.cost) return;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[fl >> FLAG_TYPE_SHIFT].n_motors, true};
    Base::tick_eval(r, src, k, fl);
  }
};
struct RolloutTickCostHook : RolloutTickEvalHook<RolloutTickCostDev> {};

// Its own: the command of a block that starts at this tick is formed, ahead of the collision evaluation, from the registers of the
// prologue (the IMU is the column's: one launch is one step).  Held and crashed UAVs get their commands, formed from their state as it
// stands, like every other UAV of the range.  The gain address is wave-uniform when the gains are shared (gain_lane 0, gain_col 1) and
// is read with vector loads all the same, as a broadcast; per-UAV gains are UAV-minor (gain_col = count), one coalesced request per
// gain element and wave.  The nominal row is read here and not through cmd_row: the law takes a whole row, zero behind the payload, and
// with the read behind a call the feedback kernels compile to other code (every other shared member leaves them as they were).
struct RolloutTickFeedbackHook : RolloutTickEvalHook<RolloutTickFeedbackDev> {
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int) const {
    CDev&     r = fresh(*r0);
    const int k = i - r.first;
    if (!mine(r, k)) return false;
    L.flags = with_mode(r, L.flags);
    if (!r.cmd) return false;  // (wave-uniform) no command block starts at this tick
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
    cmd_store(sw, off8, L, width, u);
    return false;
  }
};

// layout of a tick family's argument segment: CollKernArgs, then the descriptor
template <class Dev>
struct RolloutTickKernArgs {
  SwarmDev sw;
  double   dt, inv_dt;
  CollDev  cd;
  Dev      r;
};

}  // namespace

// A family of tick kernels: the four single-GPU *_coll shapes of step_device.inc once more (COLL, not SHARD, one step), with their
// launch bounds and accessors, and the family's descriptor and hook.  Every family has kernels of its own (RolloutKernels).
template <class Dev>
struct RolloutTickKernels {
  typedef void (*Kernel)(SwarmDev, double, double, CollDev, Dev);
  Kernel cascade_buf, model_buf, cascade, mixed;
};
#define MRS_ROLLOUT_TICK_SHAPE(name, bounds, CASCADE, UNIFORM, ACC, SU, DevType, HookType)                                             \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, CollDev /*read in place*/,   \
                                                                  DevType /*read in place*/) {                                         \
    typedef const __attribute__((address_space(4))) char CChar;                                                                        \
    CChar*    args = (CChar*)__builtin_amdgcn_kernarg_segment_ptr();                                                                   \
    CCollDev* cdk  = (CCollDev*)(args + offsetof(RolloutTickKernArgs<DevType>, cd));                                                   \
    HookType  hk{};                                                                                                                    \
    hk.r0 = (HookType::CDev*)(args + offsetof(RolloutTickKernArgs<DevType>, r));                                                       \
    int  blk_;                                                                                                                         \
    bool took_;                                                                                                                        \
    step_kernel_body<CASCADE, UNIFORM, 1, false, SU, true, false, false>(ACC(sw), dt, inv_dt, 1, *cdk, blk_, took_, hk);               \
  }
#define MRS_ROLLOUT_TICK_FAMILY(infix, DevType, HookType)                                                                              \
  static_assert(offsetof(RolloutTickKernArgs<DevType>, cd) == offsetof(CollKernArgs, cd), "the descriptor must not move CollDev");     \
  MRS_ROLLOUT_TICK_SHAPE(mrs_uav_rollout_tick##infix##_buf, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccBuf, MRS_SU, DevType, HookType)       \
  MRS_ROLLOUT_TICK_SHAPE(mrs_uav_model_rollout_tick##infix##_buf, (64, MRS_WAVES_PER_SIMD), false, true, SwarmAccBuf, MRS_SU, DevType, HookType) \
  MRS_ROLLOUT_TICK_SHAPE(mrs_uav_rollout_tick##infix, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccPtr, MRS_SU, DevType, HookType)             \
  MRS_ROLLOUT_TICK_SHAPE(mrs_uav_rollout_tick##infix##_mixed, (64, MRS_WAVES_PER_SIMD), true, false, SwarmAccPtr, MRS_SU, DevType, HookType)    \
  static const RolloutTickKernels<DevType> KNAME(k_rollout_tick##infix) = {                                                            \
      KNAME(mrs_uav_rollout_tick##infix##_buf), KNAME(mrs_uav_model_rollout_tick##infix##_buf), KNAME(mrs_uav_rollout_tick##infix),    \
      KNAME(mrs_uav_rollout_tick##infix##_mixed)};
MRS_ROLLOUT_TICK_FAMILY(_feedback, RolloutTickFeedbackDev, RolloutTickFeedbackHook)
MRS_ROLLOUT_TICK_FAMILY(_cost, RolloutTickCostDev, RolloutTickCostHook)
MRS_ROLLOUT_TICK_FAMILY(, RolloutTickDev, RolloutTickHook)

// One tick of the whole swarm with the kernels `k` of one family: the fused step + collision-evaluation launch of mrs_launch_step_coll
// (single GPU) with what `r` names of this tick.  variant and the buffer / pointer choice as there (rollout_buffer_addressing).
template <class Dev>
static hipError_t launch_rollout_tick(const RolloutTickKernels<Dev>& k, SwarmDev sw, const CollDev& cd, const Dev& r, double dt, int variant,
                                      hipStream_t st) {
  const int nb = (sw.n + 63) / 64;
  if (nb <= 0) return hipSuccess;
  sw.blk0 = 0;
  const dim3   g(nb), b(64);
  const double inv_dt = 1.0 / dt;
  const bool   buf    = rollout_buffer_addressing(sw);
  hipLaunchKernelGGL(buf ? (variant == 1 ? k.model_buf : k.cascade_buf) : k.cascade, g, b, 0, st, sw, dt, inv_dt, cd, r);
  if (sw.n_mixed > 0) hipLaunchKernelGGL(k.mixed, dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, cd, r);
  return hipGetLastError();
}
extern "C" hipError_t KNAME(mrs_launch_rollout_tick_feedback)(SwarmDev sw, CollDev cd, RolloutTickFeedbackDev r, double dt, int variant,
                                                              hipStream_t st) {
  return launch_rollout_tick(KNAME(k_rollout_tick_feedback), sw, cd, r, dt, variant, st);
}
extern "C" hipError_t KNAME(mrs_launch_rollout_tick_cost)(SwarmDev sw, CollDev cd, RolloutTickCostDev r, double dt, int variant, hipStream_t st) {
  return launch_rollout_tick(KNAME(k_rollout_tick_cost), sw, cd, r, dt, variant, st);
}
extern "C" hipError_t KNAME(mrs_launch_rollout_tick)(SwarmDev sw, CollDev cd, RolloutTickDev r, double dt, int variant, hipStream_t st) {
  return launch_rollout_tick(KNAME(k_rollout_tick), sw, cd, r, dt, variant, st);
}
