// swarm_layout.h — device data layout shared by the host library and the kernels.
//
// State lives in HBM as field-major SoA FP64: S[field * npad + uav] (npad = n rounded up to 64), so
// lane l of a wavefront reads uav base+l of every field with one coalesced 512-B request.  Per-UAV
// flags are one u32.  Per-airframe constants ("types") sit in a small table that the step kernel
// reads through the scalar cache (one type per wavefront iteration — see step_device.inc).
#pragma once
#include <stdint.h>

#define MRS_MAXM 8

// ---- SoA field indices (doubles) ----
enum {
  F_X     = 0,   // 3  position                      MultirotorModel::State::x      multirotor_model.hpp:92
  F_V     = 3,   // 3  velocity                                     ::v                                   :93
  F_VPREV = 6,   // 3                                               ::v_prev                              :94
  F_R     = 9,   // 9  rotation matrix, row-major                   ::R                                   :95
  F_W     = 18,  // 3  body rates                                   ::omega                               :96
  F_RPM   = 21,  // 8  motor rpm (first n_motors used)              ::motor_rpm                           :97
  F_IMU   = 29,  // 3  imu_acceleration_                                                                  :139
  F_FEXT  = 32,  // 3  external_force_                                                                    :142
  F_INITZ = 35,  // 1  _initial_pos_(2)                                                                   :145
  F_PID   = 36,  // 24 {position,velocity,attitude,rate} x {x,y,z} x {last_error_, integral_}  pid.hpp:20-21
  F_CMD   = 60,  // 10 payload of the active input (layout per mode, see mrs_swarm.h)   uav_system.hpp:99-108
  F_FF    = 70,  // 16 four feed-forward slots x {vec3, heading(_rate)}                 uav_system.hpp:112-115
  F_COUNT = 86
};

// ---- per-UAV flag word ----
#define FLAG_CRASHED   0x1u        // UavSystem::crashed_                    uav_system.hpp:80
#define FLAG_TAKEOFF   0x2u        // params_.takeoff_patch_enabled (mutated by step())  multirotor_model.hpp:264-276
#define FLAG_MODE_SHIFT 2          // 4 bits: UavSystem::active_input_       uav_system.hpp:95
#define FLAG_MODE_MASK (0xFu << FLAG_MODE_SHIFT)
#define FLAG_FF_SHIFT  6           // 4 bits: which std::optional feed-forwards hold a value
#define FLAG_FF_MASK   (0xFu << FLAG_FF_SHIFT)
#define FLAG_VPREV_SPLIT 0x400u   // v_prev differs from v: the F_VPREV column is authoritative.  After every step v_prev == v
                                  // (multirotor_model.hpp:281), so the step kernel neither reads nor writes F_VPREV unless
                                  // MultirotorModel::setState changed v in between (:424-433 leaves v_prev alone)
#define FLAG_HOLD       0x800u     // UavSystemRos: the model is not iterated (no input yet / input timed out, and
                                  // iterate_without_input == false)            src/uav_system_ros.cpp:265
#define FLAG_TYPE_SHIFT 16         // 16 bits: index into the type table
#define MRS_MAX_TYPES  65536

// ---- per-type constants (device copy; everything the kernels need, pre-derived on the host with the
//      reference's own operation order so the values are bit-identical to computing them per step) ----
struct TypeParams {
  int32_t n_motors, ground_enabled, desaturation, _pad;
  double  g, mass, inv_mass, min_rpm, max_rpm;
  double  kf_n;       // kf * n_motors                                  acceleration_controller.hpp:92
  double  resist_k;   // ((air_resistance_coeff * M_PI) * arm) * arm    multirotor_model.hpp:337 (prefix of the product chain)
  double  hover_thr;  // 0.90 * sqrt((mass*g)/(n_motors*kf))            multirotor_model.hpp:266-267
  double  ground_z;
  double  filt_c;     // exp(-dt/motor_time_constant) for the dt of the current launch   :244
  double  filt_1mc;   // 1.0 - filt_c
  double  tau;        // motor_time_constant
  double  inv_kf_n, inv_rpm_range;  // FAST flavour: 1/(kf*n_motors), 1/(max_rpm-min_rpm)
  double  arm_length, prop_radius;  // collision criterion             src/multirotor_simulator.cpp:342
  double  J[9], Jinv[9];            // Jinv = Eigen 3x3 cofactor inverse of J     multirotor_model.hpp:350
  double  alloc[4 * MRS_MAXM];      // torque/thrust allocation, row-major 4 x 8  :334
  double  alloc_inv[MRS_MAXM * 4];  // Mixer::allocation_matrix_inv_, n x 4       mixer.hpp:72-101
  double  pos_kp, pos_kd, pos_ki, pos_sat;                 // position_controller.hpp:92-103
  double  vel_kp, vel_kd, vel_ki, vel_sat;                 // velocity_controller.hpp:108-119
  double  att_kp, att_kd, att_ki, att_sat_rp, att_sat_yaw; // attitude_controller.hpp:160-171
  double  rate_kp[3], rate_kd[3], rate_ki[3];              // gains * J(i,i), rate_controller.hpp:56-65
  // displacement bound of the sharded collision tick ("prediction"): |acceleration| over the coming steps is at most
  //   pred_a0 + pred_thr * |allocation*rpm^2 thrust of this step| + (listed partners) * |rebounce| + pred_drag * speed^2
  double  pred_a0;    // g + 1.5 * (sum_m alloc[3][m]) * max_rpm^2 / mass; +inf when the bound cannot be given (a negative thrust column)
  double  pred_thr;   // 1.5 / mass (times the thrust of the current step: covers motor speeds beyond max_rpm — set by the host, or a lowered max_rpm)
  double  pred_drag;  // |resist_k| / mass
};

// ---- device view of a swarm ----
// SwarmDev::opts bit 1: a later launch of the same mrs_swarm_step_n call steps every UAV of this launch again before anybody can read
// the F_IMU columns, so this launch does not store them (the IMU value is an output only: no step reads it).  Plain step kernels
// only; the *_coll / sharded kernels and the rollout kernels never see the bit and do not test it.
#define MRS_OPT_IMU_DEAD 2u
#define MRS_FUSE_MAX 4  // deepest fused plain step launch (step_device.inc *_fuseD)
struct PosRecord;
struct SwarmDev {
  double*             S;      // F_COUNT x npad
  uint32_t*           F;      // npad
  const TypeParams*   T;      // type table
  unsigned long long* diag;   // 4 counters (mrs_diag_t order)
  const uint32_t*     BT;     // per 64-UAV block: airframe type (0xFFFF = mixed types) | n_motors << 16
  const int32_t*      MB;     // indices of the mixed blocks (n_mixed entries)
  int32_t             n, npad, n_mixed;
  uint32_t            opts;   // bit 0: some UAV may carry a non-zero external force (else the F_FEXT columns are not read);
                              // MRS_OPT_IMU_DEAD: set by the host on its copy, per launch
  // skin test of the collision pass's neighbour lists (collide.hip); vl_flag == nullptr: no lists are live
  const PosRecord*    vl_rec;   // per-UAV record holding the position at the last list rebuild
  uint32_t*           vl_flag;  // set to 1 when some UAV is farther than sqrt(vl_lim2) from that position
  double              vl_lim2;
  int32_t             blk0;     // step kernels: first 64-UAV block of this launch (a step may be split over two streams)
  int32_t             fast;     // MRS_ARITH_FAST swarm: the stand-alone collision passes use the FAST force expression too (collide_device.inc)
};

// ---- one launch of a device-resident rollout (mrs_swarm_rollout_device, rollout_device.inc): caller-owned rows of a run of steps ----
struct RolloutDev {
  const void* cmd;         // command row (t, k) at element ((t * count) + k) * cmd_stride: setInput payload of UAV first + k before step t
  void*       obs;         // observation row (t, k) at element ((t * count) + k) * obs_stride: the `groups` of UAV first + k after step t
  int32_t     first, count;
  int32_t     cmd_stride, width, obs_stride;
  int32_t     t0;          // the rollout step of the launch's first sub-step
  uint32_t    mode_bits;   // input mode << FLAG_MODE_SHIFT
  uint32_t    groups;      // MRS_OBS_* (0: no observation rows)
  int32_t     f32;         // rows are FP32 (else FP64)
};

// ---- one launch of a control-rate rollout (mrs_swarm_rollout_rate_device, rollout_rate_device.inc) ----
// Command row block j is held for cmd_every steps and observation row block j is written after step (j + 1) * obs_every - 1
// (mrs_swarm_rollout_rate_device).  A launch takes at most 64 sub-steps, so whatever the two rates are, the sub-steps of ONE launch that
// read a command row (or write an observation row) are s0, s0 + p, s0 + 2p, ... with s0 < 64 and p <= 64 (a rate of 64 or more: at
// most one such sub-step, p = 64).  The host hands each launch that schedule and the row pointers of its first due blocks, so the
// kernel neither divides nor knows the rollout step.  The step kernels are short of scalar registers — every word that lives through
// the sub-step loop is paid for in spills — so a schedule shares ONE word with the small fields its hook needs anyway.
#define MRS_RO_S0(w) ((w) & 63u)                      // first due sub-step of the launch
#define MRS_RO_P(w) ((((w) >> 6) & 63u) + 1u)          // distance of two due sub-steps, 1..64
#define MRS_RO_M(w) ((((w) >> 12) & 4095u) + 1u)       // (x * M) >> 12 == x / P for every x < 64 (mrs_ro_sched)
#define MRS_RO_HI(w) ((w) >> 24)                       // cmd_sched: width | f32 << 5; obs_sched: the MRS_OBS_* groups
struct RolloutRateDev {
  const void* cmd;         // command rows of the launch's FIRST due block; row (j, k) at element ((j * count) + k) * cmd_stride behind it:
                           // the setInput payload of UAV first + k from the launch's j-th due sub-step on
  void*       obs;         // likewise: the `groups` of UAV first + k after the launch's j-th due sub-step
  int32_t     first, count;
  int32_t     cmd_stride, obs_stride;
  uint32_t    cmd_sched;   // MRS_RO_S0 / P / M | payload width << 24 | rows are FP32 << 29.  Width 0: no command row in this launch
  uint32_t    obs_sched;   // MRS_RO_S0 / P / M | groups << 24.  Groups 0: no observation row in this launch
  uint32_t    mode_bits;   // input mode << FLAG_MODE_SHIFT
};
// the schedule bits of a launch whose first due sub-step is s0 (< 64), for a rate of `every` steps
inline uint32_t mrs_ro_sched(int s0, int every) {
  const uint32_t p = every < 64 ? (uint32_t)every : 64u;
  const uint32_t m = p == 1u ? 4096u : 4096u / p + 1u;  // x / p == (x * m) >> 12 for x < 64: the error x * (m - 4096 / p) / 4096 < 64 / 4096 <= 1 / p
  return (uint32_t)s0 | (p - 1u) << 6 | (m - 1u) << 12;
}
// How a hook reads a schedule word: one text for the kernels and for the host (tests/cpp/rollout_sched_test.cpp).
#if defined(__HIP__)
#define MRS_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define MRS_HD inline
#endif
// sub-step s (< 64) is the j-th due one of the schedule w (-1: it is not due)
MRS_HD int mrs_ro_due(uint32_t w, int s) {
  const unsigned x = (unsigned)s - MRS_RO_S0(w);
  const unsigned j = (x * MRS_RO_M(w)) >> 12;
  return ((unsigned)s >= MRS_RO_S0(w) && j * MRS_RO_P(w) == x) ? (int)j : -1;
}
// due sub-steps of the schedule w among the first `substeps`
MRS_HD int mrs_ro_due_count(uint32_t w, int substeps) {
  if ((unsigned)substeps <= MRS_RO_S0(w)) return 0;
  return (int)((((unsigned)substeps - 1u - MRS_RO_S0(w)) * MRS_RO_M(w)) >> 12) + 1;
}
// One schedule of the launch that takes the steps t0 .. t0 + sub - 1 (sub <= 64) of a call, from the call's word (its top byte: width and
// dtype, groups, or 3 for a force row) and its rate.  Blocks of a START schedule begin at a due step (commands, forces: block j from step
// j * every on), blocks of an END schedule end with one (observations, evaluations: block j behind step (j + 1) * every - 1).  `word`
// is the launch's schedule word and `blk0` the call's block of its first due sub-step: the launch's rows start there.  No due step in
// the launch: a start schedule keeps the dtype bit alone (the command word's; a force word has none and becomes 0), an end schedule is 0.
struct mrs_ro_launch {
  uint32_t  word;
  long long blk0;
};
inline mrs_ro_launch mrs_ro_launch_sched(uint32_t call_word, int t0, int sub, int every, bool start) {
  const int       s0   = start ? (every - t0 % every) % every : every - 1 - t0 % every;
  const long long blk0 = start ? ((long long)t0 + s0) / every : t0 / every;
  if (s0 < sub) return {(call_word & 0xFF000000u) | mrs_ro_sched(s0, every), blk0};
  return {start ? call_word & (32u << 24) : 0u, blk0};
}
// The same two schedules where one launch is one tick and the host works out each tick's blocks (the tick rollouts): the block of
// `n_blocks` blocks of `every` ticks each that STARTS at tick t (commands, gains, setpoints: block j at tick j * every), and the one
// that ENDS with tick t (observation and crash rows, evaluations: block j at tick (j + 1) * every - 1).  -1: none does.
inline long long mrs_tick_block_start(int t, int every, long long n_blocks) {
  return t >= 0 && t % every == 0 && t / every < n_blocks ? t / every : -1;
}
inline long long mrs_tick_block_end(int t, int every, long long n_blocks) {
  return t >= 0 && (t + 1) % every == 0 && (t + 1) / every <= n_blocks ? (t + 1) / every - 1 : -1;
}

// ---- one launch of a control-rate rollout under scheduled external forces (mrs_swarm_rollout_force_device, rollout_rate_device.inc) ----
// RolloutRateDev and a third schedule: force row block j (applyForce, world frame, N) is latched in the F_FEXT columns from step
// j * force_every on.  The dtype bit stays in cmd_sched.
struct RolloutForceDev {
  const void* cmd;
  void*       obs;
  int32_t     first, count;
  int32_t     cmd_stride, obs_stride;
  uint32_t    cmd_sched;
  uint32_t    obs_sched;
  uint32_t    mode_bits;
  const void* force;         // force rows of the launch's FIRST due block; row (j, k) at element ((j * count) + k) * force_stride behind it
  int32_t     force_stride;
  uint32_t    force_sched;   // MRS_RO_S0 / P / M | 3 << 24.  Width 0: no force row in this launch
};

// ---- one launch of a cost rollout (mrs_swarm_rollout_cost_device, rollout_cost_device.inc) ----
// RolloutRateDev's command side, and in place of observation rows an evaluation schedule: after the launch's j-th due sub-step the
// observation row of UAV first + k is compared with target row (j, k) under weight row j, and the term is added to cost[k].
struct RolloutCostDev {
  const void* cmd;
  int32_t     first, count;
  int32_t     cmd_stride;
  uint32_t    cmd_sched;   // as RolloutRateDev's (the dtype bit serves commands, targets and weights)
  uint32_t    cost_sched;  // MRS_RO_S0 / P / M | groups << 24.  Groups 0: no evaluation in this launch
  uint32_t    mode_bits;
  const void* target;      // target rows of the launch's FIRST due evaluation; row (j, k) at element j * tgt_blk + k * tgt_row behind it
  const void* weight;      // weight rows likewise; row j at element j * wt_row
  double*     cost;        // cost[k]: the running sum of UAV first + k, read and written by its lane at every due sub-step
  uint64_t    tgt_blk;     // count * target_stride, or the row width when all UAVs share one target row per evaluation
  int32_t     tgt_row;     // target_stride, or 0: shared targets
  int32_t     wt_row;      // weight_stride, or 0: one weight row for every evaluation
};

// ---- one launch of a feedback rollout (mrs_swarm_rollout_feedback_device, rollout_cost_device.inc) ----
// RolloutCostDev, whose command side becomes the NOMINAL command, and the gains and setpoints of the launch's command blocks: at the
// launch's j-th due command sub-step the F_CMD columns of UAV first + k take cmd row (j, k) + G(j, k) (ref row (j, k) - observation
// row of fb_groups).  G(j, k)[c][col] sits at element j * gain_blk + k * gain_lane + (c * row width + col) * gain_col of `gain`:
// shared gains are dense [payload, row width] matrices (gain_lane 0, gain_col 1), per-UAV gains are UAV-minor
// [payload, row width, count] (gain_lane 1, gain_col count), so that a wave's load of one gain element is one coalesced request.
struct RolloutFeedbackDev {
  const void* cmd;
  int32_t     first, count;
  int32_t     cmd_stride;
  uint32_t    cmd_sched;   // as RolloutRateDev's (the dtype bit serves commands, gains, setpoints, targets and weights)
  uint32_t    cost_sched;  // as RolloutCostDev's.  Groups 0: no evaluation in this launch (or in the whole call: target, weight, cost null)
  uint32_t    mode_bits;
  const void* target;
  const void* weight;
  double*     cost;
  uint64_t    tgt_blk;
  int32_t     tgt_row;
  int32_t     wt_row;
  const void* gain;        // gains of the launch's FIRST due command block
  const void* ref;         // setpoint rows likewise; row (j, k) at element j * ref_blk + k * ref_row
  uint64_t    gain_blk;    // elements between two gain blocks; 0: one block serves every command block
  uint64_t    ref_blk;     // count * ref_stride, or the row width when all UAVs share one row per block; 0: one block serves all
  uint32_t    gain_col;    // 1, or count: per-UAV gains
  int32_t     gain_lane;   // 0, or 1: per-UAV gains
  int32_t     ref_row;     // ref_stride, or 0: shared setpoints
  uint32_t    fb_word;     // fb_groups | row width of fb_groups << 8
};

// ---- the rows of ONE tick of a tick rollout (mrs_swarm_rollout_tick_device, rollout_tick_device.inc) ----
// One launch is one tick, so the host works out each launch's row blocks itself: no schedule words.  The descriptor travels with the
// launch's record in the stall / replay log (mrs_swarm::TickRec): a replayed launch writes the rows its no-op did not.
struct RolloutTickDev {
  const void* cmd;         // the command row block that starts at this tick (row k at element k * cmd_stride), or null: none starts
  void*       obs;         // the observation row block that ends with this tick (row k at element k * obs_stride), or null
  uint8_t*    crashed;     // the crash row block that ends with this tick (byte k), or null
  int32_t     first, count;
  int32_t     cmd_stride, obs_stride;
  uint32_t    cmd_word;    // payload width | rows are FP32 << 5 (commands and observations)
  uint32_t    groups;      // MRS_OBS_* of the observation rows
  uint32_t    mode_bits;   // input mode << FLAG_MODE_SHIFT
  int32_t     _pad;
};

// ---- ONE tick of a cost tick rollout (mrs_swarm_rollout_tick_cost_device, rollout_tick_device.inc) ----
// RolloutTickDev's command side, and in place of row blocks the evaluation that ends with this tick: the observation row of UAV first + k
// is compared with its target row under the weight row, the term is added to cost[k], and crash_cost is added behind it when the UAV's
// crash flag is set.  The host works out the pointers of each tick: no schedule words.  The descriptor travels with the launch's record
// in the stall / replay log: a replayed launch adds what its no-op did not.
struct RolloutTickCostDev {
  const void* cmd;         // the command row block that starts at this tick (row k at element k * cmd_stride), or null: none starts
  const void* target;      // the target row block of the evaluation that ends with this tick (row k at element k * tgt_row), or null
  const void* weight;      // its weight row, or null
  double*     cost;        // cost[k]: the running sum of UAV first + k, or null: no evaluation ends with this tick
  int32_t     first, count;
  int32_t     cmd_stride;
  int32_t     tgt_row;     // target_stride, or 0: all UAVs share the target row
  int32_t     wt_row;      // weight_stride, or 0: one weight row for every evaluation (the host's: the kernels read `weight` as it is)
  int32_t     width;       // elements of a row of `groups` (the host's)
  uint32_t    cmd_word;    // payload width | rows are FP32 << 5 (commands, targets and weights)
  uint32_t    groups;      // MRS_OBS_* of the cost; 0: the crash add alone (target and weight null)
  uint32_t    mode_bits;   // input mode << FLAG_MODE_SHIFT
  int32_t     _pad;
  double      crash_cost;
};

// ---- ONE tick of a feedback tick rollout (mrs_swarm_rollout_tick_feedback_device, rollout_tick_device.inc) ----
// RolloutTickCostDev whose command side becomes the NOMINAL command, with the gains and setpoints of the command block that starts at
// this tick: the F_CMD columns of UAV first + k take cmd row k + G(k) (ref row k - the observation row of fb_groups before the step).
// G(k)[c][col] sits at element k * gain_lane + (c * row width + col) * gain_col of `gain`, as RolloutFeedbackDev's.  The host works out
// the pointers of each tick, the gain and setpoint blocks included (one block serving every command block: the same pointer at every
// start): no block distances and no rate words.  The descriptor travels with the launch's record in the stall / replay log: a replayed
// launch sees the state its no-op left alone, forms the same command and adds once.
struct RolloutTickFeedbackDev {
  const void* cmd;         // the nominal command row block that starts at this tick (row k at element k * cmd_stride), or null: none starts
  const void* gain;        // the gains of that block, or null
  const void* ref;         // its setpoint rows (row k at element k * ref_row), or null
  const void* target;      // the target row block of the evaluation that ends with this tick (row k at element k * tgt_row), or null
  const void* weight;      // its weight row, or null
  double*     cost;        // cost[k]: the running sum of UAV first + k, or null: no evaluation ends with this tick (or in the whole call)
  int32_t     first, count;
  int32_t     cmd_stride;
  int32_t     ref_row;     // ref_stride, or 0: all UAVs share the setpoint row
  int32_t     tgt_row;     // target_stride, or 0: all UAVs share the target row
  int32_t     gain_lane;   // 0, or 1: per-UAV gains
  uint32_t    gain_col;    // 1, or count: per-UAV gains (UAV-minor)
  uint32_t    fb_word;     // fb_groups | row width of fb_groups << 8
  uint32_t    cmd_word;    // payload width | rows are FP32 << 5 (commands, gains, setpoints, targets and weights)
  uint32_t    groups;      // MRS_OBS_* of the cost; 0: the crash add alone (target and weight null)
  uint32_t    mode_bits;   // input mode << FLAG_MODE_SHIFT
  int32_t     _pad;
  double      crash_cost;
};

// 48-byte record exchanged for the collision pass (single- and multi-GPU): everything
// MultirotorSimulator::handleCollisions reads of the partner UAV (src/multirotor_simulator.cpp:339-350)
struct PosRecord {
  double x, y, z;
  double mass, arm_length, prop_radius;
};

// ---- fused step + collision evaluation (step_device.inc *_coll kernels; buffers owned by CollideWork, collide_work.h) ----
// A collision tick between two neighbour searches is evaluated by the NEXT step kernel: its prologue reads the positions of
// the listed partners as they were after the previous step, forms the force / crash flag handleCollisions would have
// latched (src/multirotor_simulator.cpp:321-358) and the step consumes it from registers.  Positions are double-buffered in
// their own 32-B records so that the partners' values do not change under a running launch.
struct Pos4 {
  double x, y, z, w;  // position records: w = airframe type.  The HEADER record of an export block is read as 32-bit words instead:
                      // word 0 = smallest stall index the rank knows of, word 1 = smallest warning index (0: none) — MRS_HDR_*
};
#define MRS_HDR_STALL 0
#define MRS_HDR_WARN  1
#define MRS_HDR_ERROR 2  // the rank's CTL_ERROR bits: every rank's call fails when any rank's kernels reported an error
// one record of the halo exchange of a search tick (collide.hip mrs_collide_halo_*): a PosRecord + the UAV's index on its rank
struct HaloEntry {
  double             x, y, z, mass, arm_length, prop_radius;
  unsigned long long j, pad;  // (header entry of a block: j = entries that follow, pad = flags)
};
struct PartnerConst {
  double mass, arm_length, prop_radius, _pad;
};
#define MRS_NBR_FOREIGN 0x80000000u  // neighbour-list entry: index into the gathered export buffer instead of a local UAV index
#define MRS_NO_SLOT     0xFFFFFFFFu

// control words of the list state machine (device copy `ctl`, mirrored to pinned host memory `hostw` for the first two)
enum {
  CTL_STALL = 0,     // 0, or the tick index of the launch after which the lists stopped being usable (every later launch is a no-op)
  CTL_PROGRESS = 1,  // tick index of the last launch that started
  CTL_OVERFLOW = 2,  // UAVs with more than LIST_CAP listed neighbours at the last search
  CTL_BADSLOT = 3,   // export-set translation: foreign neighbours that their owner does not export (must stay 0: the relation is symmetric)
  CTL_EXPORTS = 4,   // export-set search: number of own UAVs that some other rank lists
  CTL_WARN = 5,      // tick index of the last launch in which some UAV was beyond the WARNING part of its skin: the host schedules the
                     // next search ahead of time, in stream order, instead of waiting for the stall (host mirror only)
  // split sharded ticks (interior / boundary launches on two streams): the boundary chain mirrors what it knows into host
  // words of its own — one writer per word at any time; the host takes the smaller non-zero of a pair
  CTL_STALL2 = 6,
  CTL_WARN2 = 7,
  CTL_ERROR = 8,     // bit 0: a bounded in-kernel wait ran out; bit 1: a UAV left its skin without the displacement bound announcing it;
                     // bits 8-9: the same, reported by SOME rank of the sharded swarm (folded from the export headers, MRS_HDR_ERROR)
  CTL_I_STARTED = 9, // tick index of the last interior launch that has started (so the interior launch before it is complete)
  CTL_NBND = 11,     // 64-UAV blocks of this rank that hold a boundary UAV (set by the search)
  CTL_NL1 = 12,      // interior blocks that list a UAV of a boundary block (MRS_BLK_LAYER1; set by the search, sent to the host with its head words)
  CTL_PRED = 13,     // set by the search when some own UAV may leave its skin within MRS_PRED_HORIZON steps (the ticks after the search are then serial)
  CTL_WORDS = 16
};
// class of a 64-UAV block in a split sharded tick (set by every search from the neighbour lists)
#define MRS_BLK_BOUNDARY 1u  // some UAV of the block lists a foreign UAV: the block is stepped by the boundary launch
#define MRS_BLK_LAYER1   2u  // interior block, some UAV of it lists a UAV of a boundary block: waits for that block's epoch word
#define MRS_PRED_HORIZON 4u  // steps by which "may leave its skin" is announced ahead (why 4: DESIGN §5)
// peer-window exchange (transport_peer.hip k_peer_allgather): the windows of all ranks as this process addresses them
#define MRS_MAX_PEERS 64
struct MrsPeerWindows {
  void* win[MRS_MAX_PEERS];
};
enum { MRS_PART_FULL = 0, MRS_PART_INTERIOR = 1, MRS_PART_BOUNDARY = 2 };

struct CollDev {
  const uint32_t*     nbr;      // [LIST_CAP][n]: row k, UAV i at nbr[k * n + i]; ascending partner order
  const uint32_t*     nbr_cnt;  // [n]
  const PosRecord*    rec;      // [n] records of the last search: skin-test reference position + airframe constants of local partners
  const Pos4*         p_in;     // [n] positions after the previous step
  Pos4*               p_out;    // [n] positions after this step
  uint32_t*           ctl;      // CTL_WORDS control words
  volatile uint32_t*  hostw;    // pinned host mirror of ctl[CTL_STALL], ctl[CTL_PROGRESS]
  // export-set exchange (world > 1): every rank's block of the gathered buffer is [header][cap] Pos4 records
  const Pos4*         g_pos;    // [world * (1 + cap)] gathered export positions of the previous tick
  const PartnerConst* g_const;  // [world * (1 + cap)] airframe constants of the exported UAVs (fixed between searches)
  Pos4*               send;     // [1 + cap] this rank's block of the next all-gather
  const uint32_t*     exp_slot; // [n] export slot of every own UAV (MRS_NO_SLOT: nobody else lists it)
  double              rebounce, lim2, lim2_warn;
  uint32_t            tau;      // tick index of this launch (1, 2, ... since the host last drained the stream)
  int32_t             n, eval, crash, world, block;  // block = 1 + cap
  int32_t             write_force, part;             // latch the evaluated force in the F_ext columns as well; MRS_PART_*
  // split sharded ticks: block classes, the boundary launch's block list, per-block epoch words (tick index of the last launch that
  // finished the block), and the displacement bound's step-dependent factors
  const uint32_t*     blk_class;  // [blocks]
  const uint32_t*     blk_list;   // [blocks]: the boundary blocks from the front, the layer-1 blocks from the back
  uint32_t*           epoch;      // [blocks]
  uint32_t            n_bnd, n_l1;  // n_l1 > 0 (interior launch): the grid is n_l1 + blocks, its first n_l1 blocks take the layer-1 blocks of the list
  double              pred_hdt;   // horizon * dt; < 0: nothing is announced (serial protocol, MRS_SHARD_SPLIT=0: every launch tests exactly)
  double              pred_lim;   // sqrt(lim2)
};
