// rollout_tick_cost_device.inc — cost tick rollouts (mrs_swarm_rollout_tick_cost_device): the four single-GPU *_coll kernels of
// step_device.inc once more, with a hook that reads the command row block starting at this tick as the tick hook does and, where the
// tick hook writes an observation row and a crash byte, adds to one FP64 number per UAV: the weighted squared distance of the row from a
// target row (obs_row.h: mrs_obs_row_cost over the lane's registers, as the cost rollouts), and behind it crash_cost when the UAV's crash
// flag is set.  One launch is one tick of timerMain (src/multirotor_simulator.cpp:211-217): the collision tick that followed the
// previous step is evaluated from the neighbour lists (:295-359), then makeStep; the evaluation sees what `makeStep; getState /
// hasCrashed` see, before this tick's handleCollisions.  No row and no crash byte leaves the registers.
//
// The two adds are two FP64 additions with a rounding each, the term first, in both step units: a tick without the fused form is one
// step of the cost rollout kernels (the term) followed by a one-lane-per-UAV add kernel (device_io.hip: the crash add) and gives the
// same bits.
//
// Replay.  The cost element is read, added to and stored: a launch must add exactly once.  A no-op launch (stale lists) leaves before
// any hook call, so it adds nothing and does not touch the element; the host replays it with the same descriptor, and the replayed
// launch adds once.  The host zeroes the vector once, in front of the call's first launch and outside the launch log (unless the call
// accumulates): a replay does not zero again.  So the sum is that of the loop whatever stalls inside the call.
//
// Included behind rollout_cost_device.inc (LaneObs) and in front of rollout_tick_device.inc.  The host computes each tick's pointers
// (tick_single.hip); the hook reads its descriptor where it needs it through the kernel-argument segment, as the kernels read CollDev
// (fresh(), CollKernArgs): the descriptor sits BEHIND CollDev and does not move it.

namespace {

typedef const __attribute__((address_space(4))) RolloutTickCostDev CRolloutTickCostDev;
DEV CRolloutTickCostDev& fresh(CRolloutTickCostDev& r) {
  CRolloutTickCostDev* q = &r;
  asm volatile("" : "+s"(q));
  return *q;
}
struct RolloutTickCostKernArgs {  // layout of the kernels' argument segment: CollKernArgs, then the descriptor
  SwarmDev           sw;
  double             dt, inv_dt;
  CollDev            cd;
  RolloutTickCostDev r;
};
static_assert(offsetof(RolloutTickCostKernArgs, cd) == offsetof(CollKernArgs, cd), "the descriptor must not move CollDev");

struct RolloutTickCostHook {
  CRolloutTickCostDev* r0;

  // rows of FP32 / FP64 elements: 64-bit element offsets (count x stride passes 2^31)
  static __device__ __forceinline__ size_t at(int k, int stride) { return (size_t)k * (size_t)stride; }

  // Once per lane, behind the wave-uniform exits (a no-op launch never gets here): the range takes the new mode, and the command row of
  // a block that starts at this tick goes into the F_CMD columns AND into the registers the prologue preloaded from those columns, as
  // in the tick rollout's hook.  Held and crashed UAVs get their commands like every other UAV of the range.
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int) const {
    CRolloutTickCostDev& r = fresh(*r0);
    const int            k = i - r.first;
    if ((unsigned)k >= (unsigned)r.count) return false;
    L.flags = (L.flags & ~FLAG_MODE_MASK) | r.mode_bits;
    if (!r.cmd) return false;  // (wave-uniform) inside a held command block the columns hold the command as they stand
    const unsigned off8  = (unsigned)i * 8u;
    const int      width = (int)(r.cmd_word & 31u);
    const size_t   a     = at(k, r.cmd_stride);
    double         c[F_FF - F_CMD];
    if (r.cmd_word & 32u) {
      const float* p = static_cast<const float*>(r.cmd) + a;
#pragma unroll
      for (int j = 0; j < F_FF - F_CMD; j++)
        if (j < width) c[j] = (double)p[j];
    } else {
      const double* p = static_cast<const double*>(r.cmd) + a;
#pragma unroll
      for (int j = 0; j < F_FF - F_CMD; j++)
        if (j < width) c[j] = p[j];
    }
#pragma unroll
    for (int j = 0; j < F_FF - F_CMD; j++)
      if (j < width) {
        sw.st(F_CMD + j, off8, c[j]);
        if (j < 4) L.pre_cmd[j] = c[j];
      }
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
  __device__ __forceinline__ void eval(CRolloutTickCostDev& r, const Src& src, int k, uint32_t flags) const {
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
  // After post_step: the collision evaluation has had its chance in either crash mode, so the lane's flag word holds every collision
  // up to the previous tick — UavSystem::hasCrashed at the instant the tick rollout takes its crash row, before this tick's
  // handleCollisions.
  template <class SW, class PT>
  __device__ __forceinline__ void obs(const SW& sw, PT& P, int i, const Lane& L, int) const {
    CRolloutTickCostDev& r = fresh(*r0);
    const int            k = i - r.first;
    if ((unsigned)k >= (unsigned)r.count) return;
    if (!r.cost) return;  // (wave-uniform) no evaluation ends with this tick
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, P.n_motors, false};
    eval(r, src, k, L.flags);
  }
  // A UAV on hold is not iterated but takes part in the collisions: the last thing its lane does is the flag word with the new mode and
  // the evaluation of its unchanged state (the IMU is the column's), with the crash add if this tick's evaluation or an earlier one set
  // its flag.  `fl` as in the tick rollout's hook.
  template <class SW>
  __device__ __forceinline__ void held(const SW& sw, int i, const Lane& L, uint32_t fl) const {
    CRolloutTickCostDev& r = fresh(*r0);
    const int            k = i - r.first;
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
#define MRS_ROLLOUT_TICK_COST_KERNEL(name, bounds, CASCADE, UNIFORM, ACC, SU)                                                         \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, CollDev /*read in place*/,  \
                                                                  RolloutTickCostDev /*read in place*/) {                             \
    typedef const __attribute__((address_space(4))) char CChar;                                                                       \
    CChar*    args = (CChar*)__builtin_amdgcn_kernarg_segment_ptr();                                                                  \
    CCollDev* cdk  = (CCollDev*)(args + offsetof(RolloutTickCostKernArgs, cd));                                                       \
    int       blk_;                                                                                                                   \
    bool      took_;                                                                                                                  \
    step_kernel_body<CASCADE, UNIFORM, 1, false, SU, true, false, false>(                                                             \
        ACC(sw), dt, inv_dt, 1, *cdk, blk_, took_, RolloutTickCostHook{(CRolloutTickCostDev*)(args + offsetof(RolloutTickCostKernArgs, r))}); \
  }
MRS_ROLLOUT_TICK_COST_KERNEL(mrs_uav_rollout_tick_cost_buf, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccBuf, MRS_SU)
MRS_ROLLOUT_TICK_COST_KERNEL(mrs_uav_model_rollout_tick_cost_buf, (64, MRS_WAVES_PER_SIMD), false, true, SwarmAccBuf, MRS_SU)
MRS_ROLLOUT_TICK_COST_KERNEL(mrs_uav_rollout_tick_cost, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccPtr, MRS_SU)
MRS_ROLLOUT_TICK_COST_KERNEL(mrs_uav_rollout_tick_cost_mixed, (64, MRS_WAVES_PER_SIMD), true, false, SwarmAccPtr, MRS_SU)
#undef MRS_ROLLOUT_TICK_COST_KERNEL

// One tick of the whole swarm: the fused step + collision-evaluation launch of mrs_launch_step_coll (single GPU) with the evaluation of
// `r`.  variant and the buffer / pointer choice as there (rollout_buffer_addressing).
extern "C" hipError_t KNAME(mrs_launch_rollout_tick_cost)(SwarmDev sw, CollDev cd, RolloutTickCostDev r, double dt, int variant, hipStream_t st) {
  const int nb = (sw.n + 63) / 64;
  if (nb <= 0) return hipSuccess;
  sw.blk0 = 0;
  const dim3   g(nb), b(64);
  const double inv_dt = 1.0 / dt;
  const bool   buf    = rollout_buffer_addressing(sw);
  if (buf && variant == 1)
    hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout_tick_cost_buf), g, b, 0, st, sw, dt, inv_dt, cd, r);
  else if (buf)
    hipLaunchKernelGGL(KNAME(mrs_uav_rollout_tick_cost_buf), g, b, 0, st, sw, dt, inv_dt, cd, r);
  else
    hipLaunchKernelGGL(KNAME(mrs_uav_rollout_tick_cost), g, b, 0, st, sw, dt, inv_dt, cd, r);
  if (sw.n_mixed > 0) hipLaunchKernelGGL(KNAME(mrs_uav_rollout_tick_cost_mixed), dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, cd, r);
  return hipGetLastError();
}
