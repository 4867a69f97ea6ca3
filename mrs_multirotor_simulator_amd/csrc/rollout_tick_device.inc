// rollout_tick_device.inc — tick rollouts (mrs_swarm_rollout_tick_device): the four single-GPU *_coll kernels of step_device.inc with a
// hook that reads the command row block starting at this tick and writes the observation and crash row blocks ending with it.  One
// launch is one tick of timerMain (src/multirotor_simulator.cpp:211-217): the collision tick that followed the previous step is
// evaluated from the neighbour lists (:295-359), then makeStep; the rows are what `setInput; makeStep; getState / hasCrashed` see
// (uav_system.hpp:175-248, :304-380, :386).
//
// Included behind rollout_cost_device.inc (LaneObs).  The host computes each launch's row pointers (tick_single.hip), so the hook has
// no schedule words; it reads its descriptor where it needs it through the kernel-argument segment, as the kernels read CollDev
// (fresh(), CollKernArgs): the descriptor sits BEHIND CollDev and does not move it.  A no-op launch (stale lists) leaves before any
// hook call and writes nothing into the caller's rows: the host replays it with the same descriptor.

namespace {

typedef const __attribute__((address_space(4))) RolloutTickDev CRolloutTickDev;
DEV CRolloutTickDev& fresh(CRolloutTickDev& r) {
  CRolloutTickDev* q = &r;
  asm volatile("" : "+s"(q));
  return *q;
}
struct RolloutTickKernArgs {  // layout of the tick-rollout kernels' argument segment: CollKernArgs, then the descriptor
  SwarmDev       sw;
  double         dt, inv_dt;
  CollDev        cd;
  RolloutTickDev r;
};
static_assert(offsetof(RolloutTickKernArgs, cd) == offsetof(CollKernArgs, cd), "the descriptor must not move CollDev");

struct RolloutTickHook {
  CRolloutTickDev* r0;

  // rows of FP32 / FP64 elements: 64-bit element offsets (count x stride passes 2^31)
  static __device__ __forceinline__ size_t at(int k, int stride) { return (size_t)k * (size_t)stride; }

  // Once per lane, behind the wave-uniform exits (a no-op launch never gets here): the range takes the new mode, and the command row of
  // a block that starts at this tick goes into the F_CMD columns (mrs_swarm_set_input_device's k_scatter_cmd; FP32 widened exactly)
  // AND into the registers the prologue preloaded from those columns, which the cascade and the motor stage read instead.  Held and
  // crashed UAVs get their commands like every other UAV of the range.  The flag word is stored behind the step as any flag change is.
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int) const {
    CRolloutTickDev& r = fresh(*r0);
    const int        k = i - r.first;
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

  // the observation row and the crash byte of UAV i
  template <class Src>
  __device__ __forceinline__ void rows(CRolloutTickDev& r, const Src& src, int k, uint32_t flags) const {
    if (r.obs) {
      const size_t a = at(k, r.obs_stride);
      if (r.cmd_word & 32u)
        mrs_obs_row(src, r.groups, static_cast<float*>(r.obs) + a);
      else
        mrs_obs_row(src, r.groups, static_cast<double*>(r.obs) + a);
    }
    if (r.crashed) r.crashed[k] = (flags & FLAG_CRASHED) ? 1 : 0;
  }
  // After post_step: the collision evaluation has had its chance in either crash mode (before the cascade, or between the cascade and
  // the motors), so the lane's flag word holds every collision up to the previous tick — UavSystem::hasCrashed at the instant the row
  // is taken, before this tick's handleCollisions.
  template <class SW, class PT>
  __device__ __forceinline__ void obs(const SW& sw, PT& P, int i, const Lane& L, int) const {
    CRolloutTickDev& r = fresh(*r0);
    const int        k = i - r.first;
    if ((unsigned)k >= (unsigned)r.count) return;
    if (!r.obs && !r.crashed) return;  // (wave-uniform) no block ends with this tick
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, P.n_motors, false};
    rows(r, src, k, L.flags);
  }
  // A UAV on hold is not iterated but takes part in the collisions: the last thing its lane does, behind the evaluation and the position
  // records, is the rows of its unchanged state (the IMU is the column's) and the flag word with the new mode.  `fl` is the word the
  // kernel keeps for a held UAV: the one it loaded, and the crash bit of this evaluation (nothing else of the UAV changes — the lane's
  // own copy has already dropped FLAG_VPREV_SPLIT for a step that does not happen).
  template <class SW>
  __device__ __forceinline__ void held(const SW& sw, int i, const Lane& L, uint32_t fl) const {
    CRolloutTickDev& r = fresh(*r0);
    const int        k = i - r.first;
    if ((unsigned)k >= (unsigned)r.count) return;
    fl      = (fl & ~FLAG_MODE_MASK) | r.mode_bits;
    sw.F[i] = fl;
    if (!r.obs && !r.crashed) return;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[fl >> FLAG_TYPE_SHIFT].n_motors, true};
    rows(r, src, k, fl);
  }
};

}  // namespace

// The four single-GPU *_coll shapes of step_device.inc once more (COLL, not SHARD, one step), with their launch bounds and accessors.
#define MRS_ROLLOUT_TICK_KERNEL(name, bounds, CASCADE, UNIFORM, ACC, SU)                                                              \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, CollDev /*read in place*/,  \
                                                                  RolloutTickDev /*read in place*/) {                                 \
    typedef const __attribute__((address_space(4))) char CChar;                                                                       \
    CChar*    args = (CChar*)__builtin_amdgcn_kernarg_segment_ptr();                                                                  \
    CCollDev* cdk  = (CCollDev*)(args + offsetof(RolloutTickKernArgs, cd));                                                           \
    int       blk_;                                                                                                                   \
    bool      took_;                                                                                                                  \
    step_kernel_body<CASCADE, UNIFORM, 1, false, SU, true, false, false>(ACC(sw), dt, inv_dt, 1, *cdk, blk_, took_,                   \
                                                                         RolloutTickHook{(CRolloutTickDev*)(args + offsetof(RolloutTickKernArgs, r))}); \
  }
MRS_ROLLOUT_TICK_KERNEL(mrs_uav_rollout_tick_buf, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccBuf, MRS_SU)
MRS_ROLLOUT_TICK_KERNEL(mrs_uav_model_rollout_tick_buf, (64, MRS_WAVES_PER_SIMD), false, true, SwarmAccBuf, MRS_SU)
MRS_ROLLOUT_TICK_KERNEL(mrs_uav_rollout_tick, (64, MRS_WAVES_PER_SIMD), true, true, SwarmAccPtr, MRS_SU)
MRS_ROLLOUT_TICK_KERNEL(mrs_uav_rollout_tick_mixed, (64, MRS_WAVES_PER_SIMD), true, false, SwarmAccPtr, MRS_SU)
#undef MRS_ROLLOUT_TICK_KERNEL

// One tick of the whole swarm: the fused step + collision-evaluation launch of mrs_launch_step_coll (single GPU) with the rows of `r`.
// variant and the buffer / pointer choice as there (rollout_buffer_addressing).
extern "C" hipError_t KNAME(mrs_launch_rollout_tick)(SwarmDev sw, CollDev cd, RolloutTickDev r, double dt, int variant, hipStream_t st) {
  const int nb = (sw.n + 63) / 64;
  if (nb <= 0) return hipSuccess;
  sw.blk0 = 0;
  const dim3   g(nb), b(64);
  const double inv_dt = 1.0 / dt;
  const bool   buf    = rollout_buffer_addressing(sw);
  if (buf && variant == 1)
    hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout_tick_buf), g, b, 0, st, sw, dt, inv_dt, cd, r);
  else if (buf)
    hipLaunchKernelGGL(KNAME(mrs_uav_rollout_tick_buf), g, b, 0, st, sw, dt, inv_dt, cd, r);
  else
    hipLaunchKernelGGL(KNAME(mrs_uav_rollout_tick), g, b, 0, st, sw, dt, inv_dt, cd, r);
  if (sw.n_mixed > 0) hipLaunchKernelGGL(KNAME(mrs_uav_rollout_tick_mixed), dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, cd, r);
  return hipGetLastError();
}
