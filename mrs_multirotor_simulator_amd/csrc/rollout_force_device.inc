// rollout_force_device.inc — control-rate rollouts under scheduled external forces (mrs_swarm_rollout_force_device): the kernels of
// rollout_rate_device.inc with a hook that also latches a force row every force_every steps.  UavSystem::applyForce
// (uav_system.hpp:293-298) latches external_force_ (multirotor_model.hpp:292-295), which enters v_dot at :346: here the F_FEXT columns,
// which the motor stage of the fused kernels reloads in every sub-step once SwarmDev::opts bit 0 is set.
//
// Included behind rollout_rate_device.inc (RolloutRateHook's schedule arithmetic, LaneObs, kRolloutMaxSteps).  Kernels of their own
// once more, for the reason given there: the third schedule costs scalar registers, and neither mrs_swarm_rollout_device nor
// mrs_swarm_rollout_rate_device pays for it — both keep their kernels instruction for instruction.

namespace {

// The sub-step hook of a force rollout launch: RolloutRateHook with a third schedule.  Row (j, k) of each kind belongs to UAV first + k
// and the launch's j-th due sub-step of that kind; the tests, block indices and the dtype are wave-uniform.
struct RolloutForceHook {
  RolloutForceDev r;

  __device__ __forceinline__ bool mine(int i) const { return (unsigned)(i - r.first) < (unsigned)r.count; }
  __device__ __forceinline__ size_t at(int i, int blk, int stride) const {
    return ((size_t)blk * (size_t)r.count + (size_t)(i - r.first)) * (size_t)stride;  // 64-bit: blocks x count x stride passes 2^31
  }
  // command row block `blk` into the F_CMD columns (RolloutRateHook::cmd_row)
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
  // force row block `blk` into the F_FEXT columns (mrs_swarm_apply_force_device's k_scatter_force); FP32 is widened exactly.  The
  // three loads are issued before the first store.
  template <class SW>
  __device__ __forceinline__ void force_row(const SW& sw, int i, int blk, uint32_t cmd_word) const {
    const unsigned off8 = (unsigned)i * 8u;
    const size_t   a    = at(i, blk, r.force_stride);
    double         f[3];
    if (MRS_RO_HI(cmd_word) & 32u) {
      const float* p = static_cast<const float*>(r.force) + a;
#pragma unroll
      for (int c = 0; c < 3; c++) f[c] = (double)p[c];
    } else {
      const double* p = static_cast<const double*>(r.force) + a;
#pragma unroll
      for (int c = 0; c < 3; c++) f[c] = p[c];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) sw.st(F_FEXT + c, off8, f[c]);
  }
  // top of sub-step s: the command row and the force row of the blocks that start here, ahead of the cascade and of the motor stage's
  // reload of the F_FEXT columns (same lane, program order); inside a block the columns hold what they hold
  template <class SW>
  __device__ __forceinline__ void cmd(const SW& sw, int i, int s) const {
    if (!mine(i)) return;
    {
      const uint32_t w = RolloutRateHook::fresh_word(r.cmd_sched);
      const int      j = RolloutRateHook::due(w, s);
      if (j >= 0) cmd_row(sw, i, j, w);
    }
    const uint32_t w = RolloutRateHook::fresh_word(r.force_sched);
    const int      j = RolloutRateHook::due(w, s);
    if (MRS_RO_HI(w) == 0u || j < 0) return;
    force_row(sw, i, j, RolloutRateHook::fresh_word(r.cmd_sched));
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
  // after post_step of sub-step s: the observation row of the block that ends here (RolloutRateHook::obs)
  template <class SW, class PT>
  __device__ __forceinline__ void obs(const SW& sw, PT& P, int i, const Lane& L, int s) const {
    const uint32_t w = RolloutRateHook::fresh_word(r.obs_sched);
    const int      j = RolloutRateHook::due(w, s);
    if (MRS_RO_HI(w) == 0u || j < 0 || !mine(i)) return;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, P.n_motors, false};
    write_obs(src, i, j, MRS_RO_HI(w), RolloutRateHook::fresh_word(r.cmd_sched));
  }
  // once per lane (RolloutRateHook::enter): a UAV on hold is not stepped, but the loop this call stands for still writes its commands
  // and forces and gathers its unchanged state — the rows of the last command block and of the last force block that start in this
  // launch (if one does), one row per observation block that ends in it, the flag word.
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int substeps) const {
    if (!mine(i)) return false;
    L.flags = (L.flags & ~FLAG_MODE_MASK) | r.mode_bits;
    if (!(L.flags & FLAG_HOLD)) return false;
    const int starts = RolloutRateHook::due_count(r.cmd_sched, substeps);
    if (starts > 0) cmd_row(sw, i, starts - 1, r.cmd_sched);
    if (MRS_RO_HI(r.force_sched) != 0u) {
      const int fstarts = RolloutRateHook::due_count(r.force_sched, substeps);
      if (fstarts > 0) force_row(sw, i, fstarts - 1, r.cmd_sched);
    }
    if (MRS_RO_HI(r.obs_sched) != 0u) {
      const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[L.flags >> FLAG_TYPE_SHIFT].n_motors, true};
      const int         ends = RolloutRateHook::due_count(r.obs_sched, substeps);
      for (int b = 0; b < ends; b++) write_obs(src, i, b, MRS_RO_HI(r.obs_sched), r.cmd_sched);
    }
    sw.F[i] = L.flags;
    return true;
  }
};

}  // namespace

// The five shapes of rollout_device.inc a third time, with the launch bounds chosen there.
#define MRS_ROLLOUT_FORCE_KERNEL(name, bounds, CASCADE, UNIFORM, BUF)                                                                  \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, int substeps, RolloutForceDev r) { \
    const CollDev none{};                                                                                                          \
    int  blk_;                                                                                                                     \
    bool took_;                                                                                                                    \
    step_kernel_body<CASCADE, UNIFORM, 1, true, MRS_SU, false, false, false>(SwarmAcc<BUF>(sw), dt, inv_dt, substeps, none, blk_, took_, \
                                                                             RolloutForceHook{r});                                 \
  }
MRS_ROLLOUT_FORCE_KERNEL(mrs_uav_rollout_force, (64, 1), true, true, false)
MRS_ROLLOUT_FORCE_KERNEL(mrs_uav_rollout_force_buf, (64, 1), true, true, true)
MRS_ROLLOUT_FORCE_KERNEL(mrs_uav_model_rollout_force, (64, 1), false, true, false)
MRS_ROLLOUT_FORCE_KERNEL(mrs_uav_model_rollout_force_buf, (64, MRS_WAVES_PER_SIMD), false, true, true)
MRS_ROLLOUT_FORCE_KERNEL(mrs_uav_rollout_force_mixed, (64), true, false, false)
#undef MRS_ROLLOUT_FORCE_KERNEL

// n_steps steps of the whole swarm with the rows of `r` (whose cmd / obs / force point at row block 0, and whose schedule words hold the
// widths, dtype and groups of the call; the schedule bits and first blocks are set here, per launch, as mrs_launch_rollout_rate sets
// two): force block j starts at step j * force_every; a launch inside one force block reads no force row at all.  sw.opts bit 0 must be
// set: the motor stage reads the F_FEXT columns only then.
extern "C" hipError_t KNAME(mrs_launch_rollout_force)(SwarmDev sw, RolloutForceDev r, double dt, int n_steps, int cmd_every, int obs_every,
                                                      int force_every, int variant, hipStream_t st) {
  static_assert(kRolloutMaxSteps <= 64, "a launch's schedule: s0 < 64, p <= 64 (RolloutRateDev)");
  const int nb = (sw.n + 63) / 64;
  if (nb <= 0 || n_steps <= 0 || cmd_every <= 0 || obs_every <= 0 || force_every <= 0) return hipSuccess;
  sw.blk0 = 0;
  const dim3            g(nb), b(64);
  const double          inv_dt = 1.0 / dt;
  static const bool     no_buf = getenv("MRS_NO_BUFFER_ADDRESSING") != nullptr;
  const bool            buf    = !no_buf && (unsigned long long)F_COUNT * (unsigned long long)sw.npad * 8ull < (1ull << 32);
  const RolloutForceDev call   = r;
  const size_t          elem   = (MRS_RO_HI(call.cmd_sched) & 32u) ? sizeof(float) : sizeof(double);
  for (int t0 = 0; t0 < n_steps; t0 += kRolloutMaxSteps) {
    const int sub = n_steps - t0 < kRolloutMaxSteps ? n_steps - t0 : kRolloutMaxSteps;
    // the first sub-steps that start a command block, end an observation block and start a force block; none in this launch: width 0
    const int       cs0 = (cmd_every - t0 % cmd_every) % cmd_every, os0 = obs_every - 1 - t0 % obs_every;
    const int       fs0 = (force_every - t0 % force_every) % force_every;
    const long long cb0 = ((long long)t0 + cs0) / cmd_every, ob0 = t0 / obs_every, fb0 = ((long long)t0 + fs0) / force_every;
    r.cmd_sched   = cs0 < sub ? (call.cmd_sched & 0xFF000000u) | mrs_ro_sched(cs0, cmd_every) : (call.cmd_sched & (32u << 24));
    r.obs_sched   = os0 < sub ? (call.obs_sched & 0xFF000000u) | mrs_ro_sched(os0, obs_every) : 0u;
    r.force_sched = (fs0 < sub && call.force) ? (3u << 24) | mrs_ro_sched(fs0, force_every) : 0u;
    r.cmd   = !call.cmd ? nullptr : static_cast<const char*>(call.cmd) + (size_t)cb0 * (size_t)call.count * (size_t)call.cmd_stride * elem;
    r.obs   = call.obs ? static_cast<char*>(call.obs) + (size_t)ob0 * (size_t)call.count * (size_t)call.obs_stride * elem : nullptr;
    r.force = !call.force ? nullptr : static_cast<const char*>(call.force) + (size_t)fb0 * (size_t)call.count * (size_t)call.force_stride * elem;
    if (variant == 1) {
      if (buf)
        hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout_force_buf), g, b, 0, st, sw, dt, inv_dt, sub, r);
      else
        hipLaunchKernelGGL(KNAME(mrs_uav_model_rollout_force), g, b, 0, st, sw, dt, inv_dt, sub, r);
    } else {
      if (buf)
        hipLaunchKernelGGL(KNAME(mrs_uav_rollout_force_buf), g, b, 0, st, sw, dt, inv_dt, sub, r);
      else
        hipLaunchKernelGGL(KNAME(mrs_uav_rollout_force), g, b, 0, st, sw, dt, inv_dt, sub, r);
    }
    if (sw.n_mixed > 0) hipLaunchKernelGGL(KNAME(mrs_uav_rollout_force_mixed), dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, sub, r);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
