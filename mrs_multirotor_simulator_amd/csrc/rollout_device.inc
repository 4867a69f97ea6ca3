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

// What the rollout hooks hold and do alike.  Dev is the family's launch descriptor (swarm_layout.h): all of them name the range
// (first, count), the command rows (cmd, cmd_stride) and mode_bits alike, the scheduled ones cmd_sched, and those that write
// observation rows obs, obs_stride and obs_sched.  A member is compiled for the families that call it; a hook that does something
// else defines the member itself.  cmd and enter call cmd_row, obs and enter call write_obs, and nothing forwards in between; the
// plain hook has its command loop inside cmd().  The kernels' instruction order follows this call structure (a forwarding level more or
// less and the same statements are scheduled differently), and DESIGN.md's register and spill tables are measured on this one.
template <class Dev>
struct RolloutHookBase {
  static constexpr bool kOnCollKernels = false;  // a sub-step hook of the MULTI kernels (step_kernel_body's static_assert)
  Dev r;

  __device__ __forceinline__ bool mine(int i) const { return (unsigned)(i - r.first) < (unsigned)r.count; }
  // row (blk, k) of a scheduled rollout belongs to UAV first + k and the launch's blk-th due sub-step
  __device__ __forceinline__ size_t at(int i, int blk, int stride) const {
    return ((size_t)blk * (size_t)r.count + (size_t)(i - r.first)) * (size_t)stride;  // 64-bit: blocks x count x stride passes 2^31
  }
  // a schedule word as this sub-step sees it: the empty asm keeps its fields from being pulled out of the sub-step loop as scalar
  // registers of their own (the word alone lives through the loop)
  static __device__ __forceinline__ uint32_t fresh_word(uint32_t w) {
    asm volatile("" : "+s"(w));
    return w;
  }
  // ---- scheduled rollouts ----
  // command row block `blk` into the F_CMD columns (mrs_swarm_set_input_device's k_scatter_cmd); FP32 is widened exactly.  `w` is a
  // command schedule word: its top byte holds the width and the dtype
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
  // observation row block `blk` to the caller's buffer; the dtype bit is the command word's
  template <class Src>
  __device__ __forceinline__ void write_obs(const Src& src, int i, int blk, uint32_t groups, uint32_t cmd_word) const {
    const size_t a = at(i, blk, r.obs_stride);
    if (MRS_RO_HI(cmd_word) & 32u)
      mrs_obs_row(src, groups, static_cast<float*>(r.obs) + a);
    else
      mrs_obs_row(src, groups, static_cast<double*>(r.obs) + a);
  }
  // top of sub-step s: the command row of the block that starts here; inside a block the columns hold the command as they stand
  template <class SW>
  __device__ __forceinline__ void cmd(const SW& sw, int i, int s) const {
    if (!mine(i)) return;
    const uint32_t w = fresh_word(r.cmd_sched);
    const int      j = mrs_ro_due(w, s);
    if (j < 0) return;
    cmd_row(sw, i, j, w);
  }
  // after post_step of sub-step s: the observation row of the block that ends here
  template <class SW, class PT>
  __device__ __forceinline__ void obs(const SW& sw, PT& P, int i, const Lane& L, int s) const {
    const uint32_t w = fresh_word(r.obs_sched);
    const int      j = mrs_ro_due(w, s);
    if (MRS_RO_HI(w) == 0u || j < 0 || !mine(i)) return;
    const LaneObs<SW> src{sw, L, (unsigned)i * 8u, P.n_motors, false};
    write_obs(src, i, j, MRS_RO_HI(w), fresh_word(r.cmd_sched));
  }
  // ---- every rollout ----
  template <class SW, class PT>
  __device__ __forceinline__ void cmd_lane(const SW&, PT&, int, const Lane&, int) const {}
  // Head and tail of every enter(), once per lane, after the wave-uniform exits: the range takes the new mode (the flag word is stored
  // behind the steps).  A UAV on hold is not stepped (UavSystemRos::makeStep), but the loop the call stands for still writes its
  // commands and gathers its unchanged state: held() tells the hook to do so, and held_done() stores the flag word — the lane is done.
  __device__ __forceinline__ bool held(int i, Lane& L) const {
    if (!mine(i)) return false;
    L.flags = (L.flags & ~FLAG_MODE_MASK) | r.mode_bits;
    return (L.flags & FLAG_HOLD) != 0u;
  }
  template <class SW>
  __device__ __forceinline__ bool held_done(const SW& sw, int i, const Lane& L) const {
    sw.F[i] = L.flags;
    return true;
  }
};

// The sub-step hook of a rollout launch.  Row (t, k) belongs to UAV first + k; t = r.t0 + s.  The dtype is a wave-uniform branch.
// Its own: the t0 addressing, and the width and dtype as descriptor fields (no schedule word).
struct RolloutHook : RolloutHookBase<RolloutDev> {
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
  // a held UAV: the last command row of the launch, one row of the unchanged state per sub-step
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int substeps) const {
    if (!held(i, L)) return false;
    cmd(sw, i, substeps - 1);
    if (r.groups != 0u) {
      const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[L.flags >> FLAG_TYPE_SHIFT].n_motors, true};
      for (int s = 0; s < substeps; s++) write_obs(src, i, s);
    }
    return held_done(sw, i, L);
  }
};

}  // namespace

// A family of rollout kernels: the five shapes of the *_multi kernels — cascade or model-only, pointer- or buffer-addressed columns, and
// the mixed-airframe blocks — with the family's descriptor and hook.  Every family has kernels of its own, not a hook that serves
// several: the step kernels are short of scalar registers, and with the rates in the plain hook the plain cascade rollout measured
// 4-6 % slower in FAST (MEASUREMENTS §7.4), so no call pays for what another call's hook holds.
// The pointer-addressed model-only kernel gets one wave per SIMD's registers: with two it spills (36-108 B of scratch per lane), and
// it only serves swarms whose state passes 4 GiB.
template <class Dev>
struct RolloutKernels {
  typedef void (*Kernel)(SwarmDev, double, double, int, Dev);
  Kernel cascade, cascade_buf, model, model_buf, mixed;
};
#define MRS_ROLLOUT_SHAPE(name, bounds, CASCADE, UNIFORM, BUF, DevType, HookType)                                                      \
  extern "C" __global__ void __launch_bounds__ bounds KNAME(name)(SwarmDev sw, double dt, double inv_dt, int substeps, DevType r) {    \
    const CollDev none{};                                                                                                          \
    int  blk_;                                                                                                                     \
    bool took_;                                                                                                                    \
    step_kernel_body<CASCADE, UNIFORM, 1, true, MRS_SU, false, false, false>(SwarmAcc<BUF>(sw), dt, inv_dt, substeps, none, blk_, took_, \
                                                                             HookType{{r}});                                       \
  }
#define MRS_ROLLOUT_FAMILY(infix, DevType, HookType)                                                                                   \
  MRS_ROLLOUT_SHAPE(mrs_uav_rollout##infix, (64, 1), true, true, false, DevType, HookType)                                             \
  MRS_ROLLOUT_SHAPE(mrs_uav_rollout##infix##_buf, (64, 1), true, true, true, DevType, HookType)                                        \
  MRS_ROLLOUT_SHAPE(mrs_uav_model_rollout##infix, (64, 1), false, true, false, DevType, HookType)                                      \
  MRS_ROLLOUT_SHAPE(mrs_uav_model_rollout##infix##_buf, (64, MRS_WAVES_PER_SIMD), false, true, true, DevType, HookType)                \
  MRS_ROLLOUT_SHAPE(mrs_uav_rollout##infix##_mixed, (64), true, false, false, DevType, HookType)                                       \
  static const RolloutKernels<DevType> KNAME(k_rollout##infix) = {                                                                     \
      KNAME(mrs_uav_rollout##infix), KNAME(mrs_uav_rollout##infix##_buf), KNAME(mrs_uav_model_rollout##infix),                         \
      KNAME(mrs_uav_model_rollout##infix##_buf), KNAME(mrs_uav_rollout##infix##_mixed)};
MRS_ROLLOUT_FAMILY(, RolloutDev, RolloutHook)

// Longest run of steps one rollout launch takes: a longer rollout is split into launches of at most this many steps, so that no launch
// runs unboundedly long (64 cascade steps of 1 M UAVs take a few milliseconds).
constexpr int kRolloutMaxSteps = 64;
static_assert(kRolloutMaxSteps <= 64, "a launch's schedule: s0 < 64, p <= 64 (RolloutRateDev)");

// the buffer / pointer choice of mrs_launch_step (MRS_NO_BUFFER_ADDRESSING forces pointers)
static bool rollout_buffer_addressing(const SwarmDev& sw) {
  static const bool no_buf = getenv("MRS_NO_BUFFER_ADDRESSING") != nullptr;
  return !no_buf && (unsigned long long)F_COUNT * (unsigned long long)sw.npad * 8ull < (1ull << 32);
}

// n_steps steps of the whole swarm with the kernels `k` of one family and the rows of `call`, in launches of at most kRolloutMaxSteps
// steps: prepare(r, t0, sub) makes `r`, which enters as the call's descriptor, the descriptor of the launch that takes the steps
// t0 .. t0 + sub - 1.  variant: 0 every input mode, 1 model only (no UAV in a cascade mode), as mrs_launch_step.
template <class Dev, class Prepare>
static hipError_t launch_rollout(const RolloutKernels<Dev>& k, SwarmDev sw, const Dev& call, double dt, int n_steps, int variant, hipStream_t st,
                                 Prepare prepare) {
  const int nb = (sw.n + 63) / 64;
  if (nb <= 0 || n_steps <= 0) return hipSuccess;
  sw.blk0 = 0;
  const dim3   g(nb), b(64);
  const double inv_dt = 1.0 / dt;
  const bool   buf    = rollout_buffer_addressing(sw);
  const auto   kernel = variant == 1 ? (buf ? k.model_buf : k.model) : (buf ? k.cascade_buf : k.cascade);
  for (int t0 = 0; t0 < n_steps; t0 += kRolloutMaxSteps) {
    const int sub = n_steps - t0 < kRolloutMaxSteps ? n_steps - t0 : kRolloutMaxSteps;
    Dev       r   = call;
    prepare(r, t0, sub);
    hipLaunchKernelGGL(kernel, g, b, 0, st, sw, dt, inv_dt, sub, r);
    if (sw.n_mixed > 0) hipLaunchKernelGGL(k.mixed, dim3(sw.n_mixed), b, 0, st, sw, dt, inv_dt, sub, r);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// the rows of block `blk` of a call's row blocks, which lie `per_blk` elements of `elem` bytes apart (null stays null)
static const void* rollout_rows(const void* rows, long long blk, size_t per_blk, size_t elem) {
  return rows ? static_cast<const char*>(rows) + (size_t)blk * per_blk * elem : nullptr;
}
static void* rollout_rows(void* rows, long long blk, size_t per_blk, size_t elem) {
  return const_cast<void*>(rollout_rows(static_cast<const void*>(rows), blk, per_blk, elem));
}

// The plain rollout: a command row before and an observation row after every step, so a launch needs its first step and no schedule.
extern "C" hipError_t KNAME(mrs_launch_rollout)(SwarmDev sw, RolloutDev r, double dt, int n_steps, int variant, hipStream_t st) {
  return launch_rollout(KNAME(k_rollout), sw, r, dt, n_steps, variant, st, [](RolloutDev& l, int t0, int) { l.t0 = t0; });
}
