// rollout_rate_device.inc — control-rate rollouts (mrs_swarm_rollout_rate_device) and control-rate rollouts under scheduled external forces
// (mrs_swarm_rollout_force_device): the rollout kernels of rollout_device.inc with hooks that read a command row every cmd_every steps,
// write an observation row every obs_every steps and, in the force family, latch a force row every force_every steps.  At a control rate
// setInput latches (uav_system.hpp:175-248): the F_CMD columns keep command block t / cmd_every through its steps (:304-380), and
// getState (:386) is asked for once per obs_every steps.  UavSystem::applyForce (uav_system.hpp:293-298) latches external_force_
// (multirotor_model.hpp:292-295), which enters v_dot at :346: here the F_FEXT columns, which the motor stage of the fused kernels
// reloads in every sub-step once SwarmDev::opts bit 0 is set.
//
// Included behind rollout_device.inc (RolloutHookBase, MRS_ROLLOUT_FAMILY, launch_rollout).  Two families with kernels of their own, for
// the reason given there: the rates cost the plain rollout scalar registers, and the third schedule costs the rate rollout some — both
// mrs_swarm_rollout_device and mrs_swarm_rollout_rate_device keep their kernels instruction for instruction.

namespace {

// The sub-step hook of a control-rate rollout launch.  Row (j, k) belongs to UAV first + k and the launch's j-th due sub-step.  Which
// sub-steps read a command row or write an observation row is the launch's schedule (RolloutRateDev): the test, the block index and the
// dtype are wave-uniform, so a sub-step inside a held command and inside an observation block loads nothing from the caller's rows and
// stores nothing to them.
// cmd and obs are the base's.
struct RolloutRateHook : RolloutHookBase<RolloutRateDev> {
  // a held UAV: the row of the last command block that starts in this launch (if one does), one row of the unchanged state per
  // observation block that ends in it
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int substeps) const {
    if (!held(i, L)) return false;
    const int starts = mrs_ro_due_count(r.cmd_sched, substeps);
    if (starts > 0) cmd_row(sw, i, starts - 1, r.cmd_sched);
    if (MRS_RO_HI(r.obs_sched) != 0u) {
      const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[L.flags >> FLAG_TYPE_SHIFT].n_motors, true};
      const int         ends = mrs_ro_due_count(r.obs_sched, substeps);
      for (int b = 0; b < ends; b++) write_obs(src, i, b, MRS_RO_HI(r.obs_sched), r.cmd_sched);
    }
    return held_done(sw, i, L);
  }
};

// The sub-step hook of a force rollout launch: RolloutRateHook with a third schedule.  Row (j, k) of each kind belongs to UAV first + k
// and the launch's j-th due sub-step of that kind; the tests, block indices and the dtype are wave-uniform.  obs is the base's.
struct RolloutForceHook : RolloutHookBase<RolloutForceDev> {
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
      const uint32_t w = fresh_word(r.cmd_sched);
      const int      j = mrs_ro_due(w, s);
      if (j >= 0) cmd_row(sw, i, j, w);
    }
    const uint32_t w = fresh_word(r.force_sched);
    const int      j = mrs_ro_due(w, s);
    if (MRS_RO_HI(w) == 0u || j < 0) return;
    force_row(sw, i, j, fresh_word(r.cmd_sched));
  }
  // a held UAV (RolloutRateHook::enter) also gets the row of the last force block that starts in this launch (if one does)
  template <class SW>
  __device__ __forceinline__ bool enter(const SW& sw, int i, Lane& L, int substeps) const {
    if (!held(i, L)) return false;
    const int starts = mrs_ro_due_count(r.cmd_sched, substeps);
    if (starts > 0) cmd_row(sw, i, starts - 1, r.cmd_sched);
    if (MRS_RO_HI(r.force_sched) != 0u) {
      const int fstarts = mrs_ro_due_count(r.force_sched, substeps);
      if (fstarts > 0) force_row(sw, i, fstarts - 1, r.cmd_sched);
    }
    if (MRS_RO_HI(r.obs_sched) != 0u) {
      const LaneObs<SW> src{sw, L, (unsigned)i * 8u, sw.T[L.flags >> FLAG_TYPE_SHIFT].n_motors, true};
      const int         ends = mrs_ro_due_count(r.obs_sched, substeps);
      for (int b = 0; b < ends; b++) write_obs(src, i, b, MRS_RO_HI(r.obs_sched), r.cmd_sched);
    }
    return held_done(sw, i, L);
  }
};

}  // namespace

MRS_ROLLOUT_FAMILY(_rate, RolloutRateDev, RolloutRateHook)
MRS_ROLLOUT_FAMILY(_force, RolloutForceDev, RolloutForceHook)

// The launchers below take `r` with cmd / obs / force at row block 0 and with the width, dtype and groups of the call in the top bytes
// of its schedule words, and give each launch its schedule bits and the rows of its first due blocks (mrs_ro_launch_sched): command
// block j starts at step j * cmd_every, observation block j ends with step (j + 1) * obs_every - 1; block boundaries fall anywhere
// inside and across launches, and a launch inside one held command reads no command row at all.  variant as launch_rollout's.

// the command and the observation side of a launch
template <class Dev>
static void rollout_rate_launch(Dev& l, int t0, int sub, int cmd_every, int obs_every) {
  const size_t        elem = (MRS_RO_HI(l.cmd_sched) & 32u) ? sizeof(float) : sizeof(double);
  const mrs_ro_launch c = mrs_ro_launch_sched(l.cmd_sched, t0, sub, cmd_every, true), o = mrs_ro_launch_sched(l.obs_sched, t0, sub, obs_every, false);
  l.cmd_sched = c.word, l.obs_sched = o.word;
  l.cmd = rollout_rows(l.cmd, c.blk0, (size_t)l.count * (size_t)l.cmd_stride, elem);
  l.obs = rollout_rows(l.obs, o.blk0, (size_t)l.count * (size_t)l.obs_stride, elem);
}

extern "C" hipError_t KNAME(mrs_launch_rollout_rate)(SwarmDev sw, RolloutRateDev r, double dt, int n_steps, int cmd_every, int obs_every, int variant,
                                                hipStream_t st) {
  if (cmd_every <= 0 || obs_every <= 0) return hipSuccess;
  return launch_rollout(KNAME(k_rollout_rate), sw, r, dt, n_steps, variant, st,
                        [=](RolloutRateDev& l, int t0, int sub) { rollout_rate_launch(l, t0, sub, cmd_every, obs_every); });
}

// Force block j starts at step j * force_every; a launch inside one force block reads no force row at all, and a call without force rows
// none in any launch.  sw.opts bit 0 must be set: the motor stage reads the F_FEXT columns only then.
extern "C" hipError_t KNAME(mrs_launch_rollout_force)(SwarmDev sw, RolloutForceDev r, double dt, int n_steps, int cmd_every, int obs_every,
                                                      int force_every, int variant, hipStream_t st) {
  if (cmd_every <= 0 || obs_every <= 0 || force_every <= 0) return hipSuccess;
  return launch_rollout(KNAME(k_rollout_force), sw, r, dt, n_steps, variant, st, [=](RolloutForceDev& l, int t0, int sub) {
    const size_t        elem = (MRS_RO_HI(l.cmd_sched) & 32u) ? sizeof(float) : sizeof(double);
    const mrs_ro_launch f    = mrs_ro_launch_sched(3u << 24, t0, sub, force_every, true);
    rollout_rate_launch(l, t0, sub, cmd_every, obs_every);
    l.force_sched = l.force ? f.word : 0u;
    l.force       = rollout_rows(l.force, f.blk0, (size_t)l.count * (size_t)l.force_stride, elem);
  });
}
