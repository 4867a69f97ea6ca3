/*
 * mrs_swarm.h — C ABI of the MI355X-native multi-UAV stepper (libmrs_swarm.so).
 *
 * Drop-in boundary for the reference's UavSystem::makeStep() hot path: a whole swarm of
 * mrs_multirotor_simulator::UavSystem objects lives on one GPU as SoA FP64 state; every entry point
 * below replaces the per-UAV C++ call named next to it (paths relative to /root/reference).
 * Plain C types, caller-owned host buffers, int return codes (MRS_OK == 0) — the reference itself
 * signals no errors on this path.  The header-only C++ facade
 * include/mrs_multirotor_simulator/uav_system/uav_system.hpp re-exports the reference's class
 * names on top of this ABI.
 *
 * There is NO CPU fallback: every compute entry point fails with MRS_ERR_HIP when no gfx950 device
 * is usable.
 */
#ifndef MRS_SWARM_H
#define MRS_SWARM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRS_MAX_MOTORS 8

enum { MRS_OK = 0, MRS_ERR_ARG = 1, MRS_ERR_HIP = 2, MRS_ERR_RANGE = 3, MRS_ERR_TYPES = 4 };

/* UavSystem::INPUT_MODE — include/mrs_multirotor_simulator/uav_system/uav_system.hpp:19-32 */
enum {
  MRS_INPUT_UNKNOWN = 0,
  MRS_ACTUATOR_CMD,
  MRS_CONTROL_GROUP_CMD,
  MRS_ATTITUDE_RATE_CMD,
  MRS_ATTITUDE_CMD,
  MRS_TILT_HDG_RATE_CMD,
  MRS_ACCELERATION_HDG_RATE_CMD,
  MRS_ACCELERATION_HDG_CMD,
  MRS_VELOCITY_HDG_RATE_CMD,
  MRS_VELOCITY_HDG_CMD,
  MRS_POSITION_CMD
};

/* the four std::optional feed-forward slots — uav_system.hpp:112-115 */
enum { MRS_FF_VELOCITY_HDG_RATE = 0, MRS_FF_VELOCITY_HDG, MRS_FF_ACCELERATION_HDG_RATE, MRS_FF_ACCELERATION_HDG };

/* multi-GPU collision exchange (mrs_swarm_set_exchange) */
enum { MRS_EXCHANGE_NONE = 0, MRS_EXCHANGE_FULL_GATHER = 1, MRS_EXCHANGE_EXPORT_SETS = 2 };

/* arithmetic flavour of the step kernel */
enum {
  MRS_ARITH_LITERAL = 0, /* reference operation order, no FMA contraction: bit-comparable with a scalar CPU restatement */
  MRS_ARITH_FAST    = 1  /* FMA contraction + reciprocal/triangular simplifications; same results to ~1e-12 relative */
};

/* MultirotorModel::ModelParams — uav_system/multirotor_model.hpp:24-88 (matrices row-major) */
typedef struct {
  int32_t n_motors;
  int32_t ground_enabled;
  int32_t takeoff_patch_enabled;
  int32_t _pad;
  double  g, mass, kf, km, prop_radius, arm_length, body_height, motor_time_constant;
  double  max_rpm, min_rpm, air_resistance_coeff, ground_z;
  double  J[9];
  double  allocation_matrix[4 * MRS_MAX_MOTORS]; /* row r, motor m at [r*MRS_MAX_MOTORS + m] */
} mrs_model_params_t;

typedef struct { int32_t desaturation; int32_t _pad; } mrs_mixer_params_t;                       /* controllers/mixer.hpp:14-17 */
typedef struct { double kp, kd, ki; } mrs_rate_params_t;                                        /* controllers/rate_controller.hpp:14-19 */
typedef struct { double kp, kd, ki, max_rate_roll_pitch, max_rate_yaw; } mrs_attitude_params_t; /* controllers/attitude_controller.hpp:14-21 */
typedef struct { double kp, kd, ki, max_acceleration; } mrs_velocity_params_t;                  /* controllers/velocity_controller.hpp:14-20 */
typedef struct { double kp, kd, ki, max_velocity; } mrs_position_params_t;                      /* controllers/position_controller.hpp:14-20 */

/* per-swarm event counters replacing the std::cout warnings of controllers/attitude_controller.hpp:196,236,245
 * and counting the NaN rollbacks of multirotor_model.hpp:228-233 */
typedef struct {
  uint64_t hdg_rate_denom_small;
  uint64_t projected_norm_small;
  uint64_t yaw_rate_not_finite;
  uint64_t nan_rollback;
} mrs_diag_t;

/* what UavSystemRos publishes per UAV and tick (src/uav_system_ros.cpp:342-466) and MultirotorSimulator::publishPoses
 * (src/multirotor_simulator.cpp:365-389), derived on the device and downloaded as one packed array */
typedef struct {
  double position[3];            /* odom.pose.pose.position                                  :352-354 */
  double orientation[4];         /* x, y, z, w of mrs_lib::AttitudeConverter(state.R) == Eigen::Quaterniond(R)  :350 */
  double velocity_body[3];       /* odom.twist.twist.linear = R^T v                          :356-360 */
  double angular_velocity[3];    /* odom/imu angular velocity = omega                         :362-364,380-382 */
  double linear_acceleration[3]; /* imu.linear_acceleration = getImuAcceleration()            :384-388 */
  double range;                  /* rangefinder: (z - ground_z)/cos(tilt) + 0.01, >40 -> 41, body_z.z <= 0 -> 41  :403-419 */
} mrs_uav_output_t;

/* one entry of MultirotorSimulator::publishPoses' geometry_msgs/PoseArray (src/multirotor_simulator.cpp:380-383): the position and
 * orientation fields of mrs_uav_output_t alone, 56 B (7 doubles, no padding) against its 136 B, bit for bit the same values */
typedef struct {
  double position[3];            /* pose.position = getState().x                              :380-382 */
  double orientation[4];         /* x, y, z, w of mrs_lib::AttitudeConverter(state.R)           :383 */
} mrs_uav_pose_t;

/* MultirotorModel::State (+ what UavSystemRos::makeStep reads right after it: IMU acceleration, crash flag) of one UAV, packed for
 * ONE device-to-host copy of a whole range — multirotor_model.hpp:90-98, src/uav_system_ros.cpp:270-282 */
typedef struct {
  double  x[3], v[3], v_prev[3];
  double  R[9];                  /* row-major */
  double  omega[3];
  double  motor_rpm[MRS_MAX_MOTORS];
  double  imu_acceleration[3];   /* UavSystem::getImuAcceleration — uav_system.hpp:424 */
  int32_t crashed;               /* UavSystem::hasCrashed — uav_system.hpp:286 */
  int32_t n_motors;
} mrs_uav_state_t;

typedef struct mrs_swarm mrs_swarm_t;

/* ---- parameter helpers (host only) ---- */
/* ModelParams::ModelParams() x500 defaults — multirotor_model.hpp:26-66 (ground_z := 0; uninitialised there) */
int mrs_model_params_default(mrs_model_params_t* p);
/* UavSystemRos::calculateInertia — src/uav_system_ros.cpp:664-671 */
int mrs_calculate_inertia(mrs_model_params_t* p);
/* allocation-matrix row scaling applied to the YAML matrix — src/uav_system_ros.cpp:100-103 */
int mrs_scale_allocation(mrs_model_params_t* p);

/* ---- lifetime ---- */
/* std::vector<std::unique_ptr<UavSystemRos>> uavs_ — src/multirotor_simulator.cpp:70,150-157.
 * All UAVs start as UavSystem() (default ctor). device_id < 0 -> current device. */
int mrs_swarm_create(int32_t n_uavs, int32_t device_id, mrs_swarm_t** out);
int mrs_swarm_destroy(mrs_swarm_t* s);
int mrs_swarm_size(const mrs_swarm_t* s, int32_t* n_uavs);
int mrs_swarm_set_arith(mrs_swarm_t* s, int32_t arith);
/* the HIP stream every launch of this swarm goes to (hipStream_t as void*) */
int mrs_swarm_stream(const mrs_swarm_t* s, void** stream);
int mrs_swarm_synchronize(mrs_swarm_t* s);
const char* mrs_last_error(void);

/* ---- construction / parameters ---- */
/* UavSystem ctors — uav_system.hpp:127-153.  params==NULL: UavSystem(void); pos==NULL: UavSystem(params)
 * (no setStatePos); else UavSystem(params, spawn_pos, spawn_heading).  pos: count x 3, heading: count. */
int mrs_swarm_construct(mrs_swarm_t* s, int32_t first, int32_t count, const mrs_model_params_t* params,
                        const double* pos, const double* heading);
/* UavSystem::setParams — uav_system.hpp:404-409 (re-creates all controllers with DEFAULT gains, fresh PIDs) */
int mrs_swarm_set_params(mrs_swarm_t* s, int32_t first, int32_t count, const mrs_model_params_t* params);
/* UavSystem::getParams — uav_system.hpp:395 (takeoff_patch_enabled reflects the flag the step may have cleared) */
int mrs_swarm_get_params(mrs_swarm_t* s, int32_t uav, mrs_model_params_t* out);
/* UavSystem::set{Mixer,RateController,AttitudeController,VelocityController,PositionController}Params —
 * uav_system.hpp:433-451; each resets the PIDs of that controller */
int mrs_swarm_set_mixer_params(mrs_swarm_t* s, int32_t first, int32_t count, const mrs_mixer_params_t* p);
int mrs_swarm_set_rate_params(mrs_swarm_t* s, int32_t first, int32_t count, const mrs_rate_params_t* p);
int mrs_swarm_set_attitude_params(mrs_swarm_t* s, int32_t first, int32_t count, const mrs_attitude_params_t* p);
int mrs_swarm_set_velocity_params(mrs_swarm_t* s, int32_t first, int32_t count, const mrs_velocity_params_t* p);
int mrs_swarm_set_position_params(mrs_swarm_t* s, int32_t first, int32_t count, const mrs_position_params_t* p);
/* UavSystem::getMixerAllocation — uav_system.hpp:415 (n_motors x 4, row-major) */
int mrs_swarm_get_mixer_allocation(mrs_swarm_t* s, int32_t uav, double* out);

/* ---- commands ---- */
/* UavSystem::setInput(...) x11 — uav_system.hpp:175-248.  payload: count x stride doubles per UAV:
 *   ACTUATOR: motors[n_motors] | CONTROL_GROUP: roll,pitch,yaw,throttle | ATTITUDE_RATE: rx,ry,rz,throttle
 *   ATTITUDE: R[9] row-major, throttle | TILT_HDG_RATE: tilt[3], heading_rate, throttle
 *   ACCELERATION_HDG(_RATE) / VELOCITY_HDG(_RATE) / POSITION: vec[3], heading(_rate) | INPUT_UNKNOWN: none */
int mrs_swarm_set_input(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, const double* payload, int32_t stride);
/* Staged form of mrs_swarm_set_input for hosts that refresh every command each tick (the subscriber callbacks of
 * src/uav_system_ros.cpp:679-1022, batched): mrs_swarm_input_staging hands out pinned host memory for count rows of `stride`
 * doubles (row k = the setInput payload of UAV first+k, layouts as above); the caller fills it and mrs_swarm_commit_input sends it
 * with one asynchronous copy (on a copy stream, beside the running step) + one unpack kernel on the swarm's stream — no pageable
 * staging, no per-column copies.  Two row blocks are handed out in turn: a block returned by mrs_swarm_input_staging belongs to
 * the caller until the commit that follows; the call waits only for the COPY of the commit two calls back, never for a step. */
int mrs_swarm_input_staging(mrs_swarm_t* s, int32_t count, int32_t stride, double** rows);
int mrs_swarm_commit_input(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, int32_t stride);

/* UavSystem::setFeedforward(...) x4 — uav_system.hpp:254-272.  payload: vec[3], heading(_rate) */
int mrs_swarm_set_feedforward(mrs_swarm_t* s, int32_t first, int32_t count, int32_t kind, const double* payload, int32_t stride);
/* UavSystem::applyForce — uav_system.hpp:295; force: count x 3 */
int mrs_swarm_apply_force(mrs_swarm_t* s, int32_t first, int32_t count, const double* force);
/* UavSystem::crash / hasCrashed — uav_system.hpp:278,286 */
int mrs_swarm_crash(mrs_swarm_t* s, int32_t first, int32_t count);
/* UavSystemRos::makeStep iterates the model only `if (_iterate_without_input_ || time_last_input_ > 0)` — src/uav_system_ros.cpp:265.
 * hold != 0 excludes the UAVs from mrs_swarm_step* / tick (state, PIDs and IMU stay as they are); collisions still see them. */
int mrs_swarm_set_hold(mrs_swarm_t* s, int32_t first, int32_t count, int32_t hold);
int mrs_swarm_has_crashed(mrs_swarm_t* s, int32_t first, int32_t count, int32_t* out);

/* ---- UavSystemRos semantics that touch device state ---- */
/* UavSystemRos::timeoutInput — src/uav_system_ros.cpp:474-647: the command of every UAV in [first, first+count) is replaced
 * by the safe command of its current input mode (hold position / zero velocity / level attitude / zero rates / zero
 * motors), computed on the device from the current state; heading = mrs_lib::AttitudeConverter(R).getHeading() */
int mrs_swarm_timeout_input(mrs_swarm_t* s, int32_t first, int32_t count);
/* UavSystemRos::callbackSetMass — :1028-1053 (allocation row 2 rescaled by m_new/m_old, inertia recomputed, setParams:
 * controllers fall back to DEFAULT gains with fresh PIDs) */
int mrs_swarm_set_mass(mrs_swarm_t* s, int32_t first, int32_t count, double mass);
/* UavSystemRos::callbackSetGroundZ — :1055-1080 (also through setParams: gains reset) */
int mrs_swarm_set_ground_z(mrs_swarm_t* s, int32_t first, int32_t count, double ground_z);

/* ---- the hot path ---- */
/* for (i) uavs_[i]->makeStep(dt) — src/multirotor_simulator.cpp:211-213 -> UavSystem::makeStep, uav_system.hpp:304-380.
 * Asynchronous on the swarm's stream. */
int mrs_swarm_step(mrs_swarm_t* s, double dt);
/* uavs_[i]->makeStep(dt) for the UAVs [first, first + count) ONLY — src/multirotor_simulator.cpp:212 outside a whole-swarm round
 * (a UAV whose inputs changed after the round's launch, a host that steps one UAV on its own).  Same results as a whole-swarm step
 * of those UAVs; the neighbour lists of the collision pass are rebuilt at the next collision tick. */
int mrs_swarm_step_range(mrs_swarm_t* s, int32_t first, int32_t count, double dt);
/* n_steps consecutive makeStep(dt) rounds; substeps_per_launch > 1 keeps the state in registers across that many
 * steps inside one launch (legal while commands are constant and collisions are off; results identical).  After the call every
 * getter returns what n_steps single mrs_swarm_step calls leave behind; the IMU value (an output no step reads) is stored by the
 * last launch of the call only.  substeps_per_launch is the caller's minimum: with the value 1 the library may still keep the state
 * in registers across steps of the call (no UAV in a cascade mode, no mixed-airframe blocks: launches of up to four steps), and the
 * results are those of single steps, bit for bit; MRS_RUN_FUSION=0 in the environment at mrs_swarm_create restores one launch per step.
 * mrs_swarm_last_step_kernel_ms counts the launches really issued. */
int mrs_swarm_step_n(mrs_swarm_t* s, double dt, int32_t n_steps, int32_t substeps_per_launch);
/* MultirotorSimulator::handleCollisions — src/multirotor_simulator.cpp:295-359 (kd-tree replaced by a spatial hash) */
int mrs_swarm_handle_collisions(mrs_swarm_t* s, int32_t enabled, int32_t crash, double rebounce);
/* n_ticks of the timerMain order: makeStep for all, then handleCollisions — src/multirotor_simulator.cpp:211-217 */
int mrs_swarm_tick_n(mrs_swarm_t* s, double dt, int32_t n_ticks, int32_t enabled, int32_t crash, double rebounce);

/* ---- state access ---- */
/* UavSystem::getState — uav_system.hpp:386 / MultirotorModel::State multirotor_model.hpp:90-98.  Any pointer may be
 * NULL.  x,v,v_prev,omega: count x 3; R: count x 9 row-major; motor_rpm: count x MRS_MAX_MOTORS. */
int mrs_swarm_get_state(mrs_swarm_t* s, int32_t first, int32_t count, double* x, double* v, double* v_prev, double* R,
                        double* omega, double* motor_rpm);
/* the same for a whole range as packed records: one pack kernel, one device-to-host copy (what a per-UAV loop of getState() calls
 * over a pool of UavSystem objects is served from: uav_system.hpp UavPool) */
int mrs_swarm_get_states(mrs_swarm_t* s, int32_t first, int32_t count, mrs_uav_state_t* out);
/* MultirotorModel::setState — multirotor_model.hpp:424-433 (v_prev untouched, like the reference) */
int mrs_swarm_set_state(mrs_swarm_t* s, int32_t first, int32_t count, const double* x, const double* v, const double* R,
                        const double* omega, const double* motor_rpm);
/* MultirotorModel::setStatePos — multirotor_model.hpp:439-446: x, R = AngleAxis(-heading, z) and _initial_pos_; everything else stays */
int mrs_swarm_set_state_pos(mrs_swarm_t* s, int32_t first, int32_t count, const double* pos, const double* heading);
/* the controllers' PID state (layout of mrs_swarm_get_pid): the reference has no accessor for it — needed to copy a UavSystem */
int mrs_swarm_set_pid(mrs_swarm_t* s, int32_t first, int32_t count, const double* pid);
/* an independent copy of the whole swarm on the same device: state, commands, feed-forwards, PIDs, parameters, flags.  The
 * reference's UavSystem is a copy-assignable value (src/uav_system_ros.cpp:105); collision bookkeeping starts afresh in the copy. */
int mrs_swarm_clone(mrs_swarm_t* s, mrs_swarm_t** out);
/* the same with room for more UAVs: the first mrs_swarm_size(s) UAVs are copies, the others UavSystem() — how a pool of
 * UavSystem objects grows (include/mrs_multirotor_simulator/uav_system/uav_system.hpp UavPool) */
int mrs_swarm_clone_resized(mrs_swarm_t* s, int32_t n_uavs, mrs_swarm_t** out);
/* UavSystem copy-assignment between batches: UAVs [src_first, src_first + count) of `src` replace [dst_first, ...) of `dst` — state,
 * command, feed-forwards, PIDs, flags and parameter set.  The swarms must be clones of each other (mrs_swarm_clone[_resized]: their
 * parameter tables agree on every index in use; MRS_ERR_TYPES otherwise) on the same device; ranges of one swarm must not overlap. */
int mrs_swarm_copy_uavs(mrs_swarm_t* dst, int32_t dst_first, mrs_swarm_t* src, int32_t src_first, int32_t count);
/* UavSystem::getImuAcceleration — uav_system.hpp:424 */
int mrs_swarm_get_imu(mrs_swarm_t* s, int32_t first, int32_t count, double* imu);
/* MultirotorModel::getExternalForce — multirotor_model.hpp:452 */
int mrs_swarm_get_external_force(mrs_swarm_t* s, int32_t first, int32_t count, double* force);
/* PID internals for parity checks: count x 24 = {position,velocity,attitude,rate} x {x,y,z} x {last_error, integral} */
int mrs_swarm_get_pid(mrs_swarm_t* s, int32_t first, int32_t count, double* pid);
int mrs_swarm_get_diag(mrs_swarm_t* s, mrs_diag_t* out);
/* publishOdometry + publishIMU + publishRangefinder + publishPoses payloads of UAVs [first, first+count): one pack kernel,
 * one device-to-host copy (src/uav_system_ros.cpp:342-431, src/multirotor_simulator.cpp:365-389) */
int mrs_swarm_get_outputs(mrs_swarm_t* s, int32_t first, int32_t count, mrs_uav_output_t* out);
/* the same payloads without the final host copy: *view points into the library's pinned staging buffer and stays valid until the
 * next mrs_swarm_get_outputs* call on this swarm (publishers fill their messages straight from it) */
int mrs_swarm_get_outputs_view(mrs_swarm_t* s, int32_t first, int32_t count, const mrs_uav_output_t** view);
/* The same payloads PIPELINED with the steps — what a loop that publishes every UAV's odometry / IMU / range every step
 * (src/uav_system_ros.cpp:278-282) and the pose array every tick (src/multirotor_simulator.cpp:215,365-389) should call.
 * mrs_swarm_get_outputs_async returns at once: the pack kernel is queued on the swarm's stream behind every step queued so far, the
 * device-to-host copy runs on a copy stream into one of two pinned blocks.  mrs_swarm_outputs_wait blocks until THAT copy has
 * landed (an event, not a stream synchronisation: steps queued after the _async call keep running — the download of tick t overlaps
 * step t + 1) and hands out the block; it stays valid until the second _async call after this ticket's.  At most two tickets are in
 * flight.  Collision ticks evaluated lazily by the next step launch (mrs_swarm_tick_n) stay lazy: if a launch before the pack turned
 * out to be a no-op (stale neighbour lists), the wait repeats search, launches and pack before it returns — the payload is always
 * the state after the tick the caller packed behind. */
int mrs_swarm_get_outputs_async(mrs_swarm_t* s, int32_t first, int32_t count, int32_t* ticket);
int mrs_swarm_outputs_wait(mrs_swarm_t* s, int32_t ticket, const mrs_uav_output_t** view, int32_t* count);
/* The pose array alone (MultirotorSimulator::publishPoses, src/multirotor_simulator.cpp:215,365-389): the same calls for 56-B
 * mrs_uav_pose_t records, for a host that publishes poses only (0.41x the bytes of mrs_uav_output_t).  The two payloads keep their own
 * staging: a _view stays valid until the next call of ITS kind (a mrs_swarm_get_outputs* call does not invalidate a pose view, nor the
 * reverse).  _async / _wait: the contract of mrs_swarm_get_outputs_async / mrs_swarm_outputs_wait above, with these ticket rules:
 *   - each kind has its own two blocks: at most two pose downloads and two wide ones are in flight, and a pose block stays valid until the
 *     second mrs_swarm_get_poses_async after its ticket's (wide downloads in between do not count);
 *   - tickets of both kinds come from one counter; a wait given a ticket of the other kind, or one whose block has been handed to a
 *     newer download of its kind, fails with MRS_ERR_ARG;
 *   - any number of downloads of either kind may follow one tick: a stall repeats every one of them whose block is still held. */
int mrs_swarm_get_poses(mrs_swarm_t* s, int32_t first, int32_t count, mrs_uav_pose_t* out);
int mrs_swarm_get_poses_view(mrs_swarm_t* s, int32_t first, int32_t count, const mrs_uav_pose_t** view);
int mrs_swarm_get_poses_async(mrs_swarm_t* s, int32_t first, int32_t count, int32_t* ticket);
int mrs_swarm_poses_wait(mrs_swarm_t* s, int32_t ticket, const mrs_uav_pose_t** view, int32_t* count);
/* pipelined downloads of both kinds: packs issued by the _async calls, and packs issued again by a replay after a stall */
int mrs_swarm_get_download_stats(mrs_swarm_t* s, int64_t* issued, int64_t* reissued);

/* ---- multi-GPU collision exchange (one swarm shard per process/GPU) ---- */
/* device pointer + byte size of this shard's packed {x,y,z,mass,arm_length,prop_radius} records (48 B/UAV), refreshed by
 * mrs_swarm_pack_positions; the caller all-gathers them (RCCL) into a buffer of n_total records */
int mrs_swarm_pack_positions(mrs_swarm_t* s, void** dev_ptr, int64_t* n_bytes);
/* same records written to caller-owned device memory (e.g. the send buffer of an RCCL all-gather): n_uavs x 48 B */
int mrs_swarm_pack_positions_to(mrs_swarm_t* s, void* dev_dst);
/* handleCollisions for this shard against ALL gathered records (device pointer, n_total x 48 B);
 * my_offset = index of this shard's first UAV in the gathered order */
int mrs_swarm_handle_collisions_gathered(mrs_swarm_t* s, const void* dev_records, int64_t n_total, int64_t my_offset,
                                         int32_t enabled, int32_t crash, double rebounce);

/* The same exchange done by the library itself, for hosts that do not want to drive the collective: it is issued on the swarm's own
 * stream between the kernels, so a whole run of ticks is one call.  Two exchanges exist (mrs_swarm_set_exchange):
 *   MRS_EXCHANGE_EXPORT_SETS (default) — SURVEY 8e v2, "all-gather of boundary-UAV positions": a tick that repeats the neighbour
 *       search gathers the records another rank can list (those inside its bounding box of the last search; 64 B each — the first
 *       search, and any search whose halo turns out too small, gathers all 48-B records: mrs_swarm_get_search_stats); every tick until
 *       the next search gathers only the UAVs some other rank lists (32 B each, padded to the largest export set), and the collision
 *       tick is evaluated by the next step kernel (as on one GPU);
 *   MRS_EXCHANGE_FULL_GATHER — all 48-B records on every tick.
 * Results are identical.  Shards are equal-count index ranges of the caller's (spatially sorted, see mrs_slab_partition) order.
 * Collective backends:
 *   RCCL, bound at run time from `librccl_path` (NULL = "librccl.so" from the loader path; a process that already holds a HIP
 *       runtime — PyTorch-ROCm ships its own — must name the librccl.so that belongs to THAT runtime):
 *         mrs_rccl_unique_id   : rank 0 creates the 128-byte id and hands it to the other ranks by any host channel
 *         mrs_swarm_comm_init  : collective; this swarm must hold the shard of `rank` (n_total / world UAVs, the first
 *                                n_total % world ranks one more)
 *   a caller-supplied all-gather (mrs_swarm_comm_init_custom): `fn` must enqueue, on `stream`, the all-gather of `bytes_per_rank`
 *       bytes from `send` into `recv` (rank-major) and return 0; every rank calls it the same number of times in the same order
 *   an in-process group (mrs_loopback_group_*): `world` swarms of ONE process, each driven by its own host thread, on one device
 *       ("virtual shards", what the tests use on the one-GPU box) or on several devices of a node without RCCL
 *   mrs_swarm_tick_sharded_n : n_ticks of timerMain on every rank — makeStep, then handleCollisions over ALL n_total UAVs
 *                          (src/multirotor_simulator.cpp:211-217, 295-359); collective; returns with every tick evaluated
 *   mrs_swarm_comm_destroy   : collective */
typedef int (*mrs_allgather_fn)(void* user, const void* send, void* recv, uint64_t bytes_per_rank, void* stream);
typedef struct mrs_loopback_group mrs_loopback_group_t;
int mrs_rccl_unique_id(const char* librccl_path, uint8_t* id128);
int mrs_swarm_comm_init(mrs_swarm_t* s, const char* librccl_path, int32_t world, int32_t rank, const uint8_t* id128, int64_t n_total);
int mrs_swarm_comm_init_custom(mrs_swarm_t* s, int32_t world, int32_t rank, int64_t n_total, mrs_allgather_fn fn, void* user);
int mrs_loopback_group_create(int32_t world, mrs_loopback_group_t** out);
int mrs_loopback_group_destroy(mrs_loopback_group_t* g);
int mrs_swarm_comm_init_loopback(mrs_swarm_t* s, mrs_loopback_group_t* g, int32_t rank, int64_t n_total);
/* test hooks of the sharded tick (tests/test_sharded_chaos_gpu.py):
 *   mrs_loopback_group_set_rendezvous : the group's all-gather without its two host barriers — a rank waits only until every peer
 *       has ARRIVED at the same collective (before the group's first collective);
 *   mrs_swarm_debug_chaos : this rank's host sleeps a random 0..max_sleep_us before every launch and, at random, decides on the
 *       stall / warning words as it read them one launch earlier — host skew the protocol must tolerate (0 switches it off);
 *   mrs_swarm_get_split_stats : ticks this rank ran in the split form (interior and boundary launches on two streams) and the
 *       64-UAV blocks its boundary launch covers since the last search; on a swarm that is not sharded, the steps that
 *       mrs_swarm_step_n launched as two half-swarm launches on two streams */
int mrs_loopback_group_set_rendezvous(mrs_loopback_group_t* g, int32_t on);
int mrs_swarm_debug_chaos(mrs_swarm_t* s, int32_t max_sleep_us, uint64_t seed);
int mrs_swarm_get_split_stats(mrs_swarm_t* s, int64_t* split_ticks, int64_t* boundary_blocks);
/* Neighbour searches of the export-set exchange on this rank: all of them; the ones that ran on a HALO exchange — each rank sends the
 * records that lie inside another rank's box of the last search (plus the distance a UAV may have moved), 64 B each, instead of
 * gathering all 48-B records (MRS_SEARCH_HALO=0 switches that off); the halo searches that had to be repeated on all records (a UAV
 * further from its rank's old hull than the margin, or more entries than the block held); the entries per rank the next one sends.
 * Results do not depend on which exchange a search used. */
int mrs_swarm_get_search_stats(mrs_swarm_t* s, int64_t* searches, int64_t* halo_searches, int64_t* halo_repeats, int64_t* halo_capacity);
/* test / measurement hook: a kernel that keeps `stream` (a hipStream_t of this process) busy for `microseconds` — stands in for the
 * latency of a collective in tools/sharded_rank_cost.py */
int mrs_debug_stream_delay(void* stream, double microseconds);
/* measurement stand-in for ONE rank of a `world`-rank sharded swarm alone on a device (tools/sharded_rank_cost.py): every collective
 * takes `collective_latency_us` of stream time, and the rank's neighbours in the slab order are periodic images of itself
 * `slab_width` metres away — boundary sets, launches and buffer sizes of the real run, none of its physics across the slab faces.
 * Not a simulation backend. */
int mrs_swarm_comm_init_standin(mrs_swarm_t* s, int32_t world, int32_t rank, int64_t n_total, double collective_latency_us, double slab_width);
/* Peer-window exchange — the collectives of the sharded tick as direct writes into the peers' device memory over xGMI, no
 * collective library and no host in the tick (one small kernel per collective on the swarm's stream: push into every peer's
 * window, signal, wait for every peer's signal, pull — csrc/transport_peer.hip k_peer_allgather).  xGMI is point to point: a rank's block
 * reaches every peer in ONE hop, where a ring all-gather pays 2 (world - 1) hops behind its own kernel launch.
 *   mrs_swarm_peer_window_create : allocates this rank's window (4096 + 2 * world * slot bytes, slot = the largest shard's full
 *       gather) and returns its address (`window`, for peers in the same process) and / or its 64-byte IPC handle (`ipc_handle64`,
 *       for peers in other processes: hipIpcMemHandle_t) — either may be NULL;
 *   mrs_swarm_comm_init_peer     : binds the communicator once the caller has carried the addresses / handles to every rank by any
 *       host channel: `windows[q]` (if given and not NULL) is rank q's window as THIS process addresses it (same process, or a
 *       device with peer access enabled), otherwise `ipc_handles + 64 q` is opened.  The entries of the own rank are ignored.
 * Afterwards mrs_swarm_tick_sharded_n / mrs_swarm_comm_destroy as with any other backend (destroy only after every rank's last
 * tick call has returned: peers write into the window until then).  A rank that waits 10 s for a peer's block gives up and the
 * call returns MRS_ERR_HIP.  Ranks of one process must sit on DIFFERENT devices (peer access enabled by the caller): on one device the
 * kernels of different ranks wait for each other, and any runtime call of one rank's host that waits for the whole device (hipFree in a
 * search that grows a buffer) then waits for a peer's kernel that waits for this rank. */
int mrs_swarm_peer_window_create(mrs_swarm_t* s, int32_t world, int32_t rank, int64_t n_total, void** window, uint8_t* ipc_handle64);
int mrs_swarm_comm_init_peer(mrs_swarm_t* s, void* const* windows, const uint8_t* ipc_handles);
int mrs_swarm_set_exchange(mrs_swarm_t* s, int32_t exchange);
int mrs_swarm_tick_sharded_n(mrs_swarm_t* s, double dt, int32_t n_ticks, int32_t enabled, int32_t crash, double rebounce);
int mrs_swarm_comm_destroy(mrs_swarm_t* s);
/* Spatially coherent shards for a swarm addressed by a fixed public index (the reference's uavs_[i]): UAVs sorted by x and cut into
 * `world` equal-count slabs (n_total / world each, the first n_total % world one more).  order[k] = public index of the UAV at
 * position k of the sorted order (rank r holds order[lo_r .. hi_r)); host only. */
int mrs_slab_partition(const double* pos_xyz, int64_t n_total, int32_t world, int64_t* order);
/* A spawn order that follows space, for callers that are free to choose which UAV gets which index (the reference numbers its UAVs in
 * the order of config/uavs.yaml, src/multirotor_simulator.cpp:136-157): order[k] = index, in the caller's numbering, of the UAV that
 * should be spawned k-th, by a Morton key of the neighbour-list cells (edge `cell` metres; <= 0: the library's 2.25 m).  Listed partners
 * and hash buckets of neighbours then share cache lines: -2 % on a collision tick, -7 % on a neighbour search at 100 000 UAVs
 * (profiles/r05_overlapped_ticks_on_ordered_slots.log).  Results do not depend on the order; host only. */
int mrs_cell_order(const double* pos_xyz, int64_t n_total, double cell, int64_t* order);
/* what the communicator of this swarm looks like: ranks as mrs_swarm_comm_init was told and as RCCL itself counts them
 * (ncclCommCount), the exchange in use and the bytes every rank contributes to the per-tick collective */
typedef struct {
  int32_t world, rank;
  int32_t rccl_ranks;       /* ncclCommCount of the communicator (0: no RCCL communicator, e.g. an in-process loopback group) */
  int32_t exchange;         /* MRS_EXCHANGE_* */
  int64_t n_total;
  int64_t bytes_per_tick;   /* bytes this rank sends into the collision collective of an ordinary tick */
  int64_t bytes_per_rebuild; /* bytes it sends on a tick that repeats the neighbour search (export-set exchange only) */
  int64_t export_count, export_capacity; /* export-set exchange: own UAVs some other rank lists / slots of the padded collective */
  int64_t ticks, searches, noop_ticks;   /* sharded ticks so far, how many repeated the search, launches replayed after a stale-list tick */
} mrs_comm_info_t;
int mrs_swarm_comm_info(mrs_swarm_t* s, mrs_comm_info_t* out);

/* collision-pass statistics of mrs_swarm_handle_collisions / mrs_swarm_tick_n: ticks that ran the pass, and how many of them had to
 * repeat the neighbour search (the others reused the neighbour lists of an earlier tick — same results as the reference's per-tick
 * kd-tree, src/multirotor_simulator.cpp:303-317, which this replaces) */
int mrs_swarm_get_collision_stats(mrs_swarm_t* s, int64_t* n_ticks, int64_t* n_rebuilds);

/* how the collision ticks of mrs_swarm_tick_n / step + handle_collisions were evaluated: by the following step launch (fused), how often
 * a launch found the neighbour lists stale (a UAV had left its skin), how many queued launches had to be issued again after it, and
 * how many searches the host queued ahead of time (a UAV close to the edge of its skin) so that no launch found them stale */
int mrs_swarm_get_fused_stats(mrs_swarm_t* s, int64_t* fused_launches, int64_t* stalls, int64_t* replayed_launches, int64_t* searches_ahead);

/* diagnostic hook: the eight control words of the collision pass's neighbour-list state machine (skin flags of the two tick
 * parities, search counter, table-dirty flags, list-overflow counter — collide.hip); synchronises the stream.  tools/collision_words.py */
int mrs_swarm_debug_collision_words(mrs_swarm_t* s, uint32_t* out8);
/* test hook: runs the cascade kernels' own PID device function (PIDController::update, controllers/pid.hpp:67-96) over
 * caller-given sequences on the GPU, one lane per sequence — row-major [n_seq][n_steps] arrays; params = n_seq x
 * {kp, kd, ki, saturation, antiwindup}; event 1 = reset() before the update, 2 = setSaturation(new_sat) before it.
 * tests/test_parity_gpu.py feeds it the golden vectors recorded from the reference's own class. */
int mrs_debug_pid_sequences(int32_t device_id, int32_t arith, int32_t n_seq, int32_t n_steps, const double* params, const double* err,
                            const double* dt, const double* event, const double* new_sat, double* out);

/* one PIDController::update (controllers/pid.hpp:67-96) for each of n independent controllers, on the GPU, with caller-held state:
 * params = n x {kp, kd, ki, saturation, antiwindup}, state = n x {last_error, integral} (updated in place), err / dt / out = n.
 * Backs the stand-alone PIDController class of the header facade. */
int mrs_debug_pid_update(int32_t device_id, int32_t arith, int32_t n, const double* params, double* state, const double* err, const double* dt,
                         double* out);
/* ONE component of the path for the UAVs [first, first + count), on each UAV's own state (x, v, R, omega, motor_rpm, external force),
 * airframe / controller constants and PID state — the device functions the step kernels are made of, run on their own.  Row k of `in`
 * (in_stride doubles) is the input for UAV first + k, row k of `out` receives the result; the PID-bearing controllers update the
 * UAV's PID state like getControlSignal() mutates the reference's controller objects.  Backs the stand-alone L0 classes of the
 * header facade (MultirotorModel, the controllers) and the per-component parity tests.  Matrices row-major.
 *   component                        in                               out                             reference
 *   MRS_COMP_REORTH                  R[9]                             R * L^-1 [9]                    multirotor_model.hpp:249-253, :314-316
 *   MRS_COMP_MODEL_RHS               x[3] v[3] R[9] omega[3]          derivative, same order [18]     MultirotorModel::operator() :301-366
 *   MRS_COMP_MIXER                   roll pitch yaw throttle          motors[8]                       Mixer::getControlSignal mixer.hpp:107-144
 *   MRS_COMP_POSITION                position ref[3]                  velocity[3]                     position_controller.hpp:73-86
 *   MRS_COMP_VELOCITY                velocity ref[3]                  acceleration[3]                 velocity_controller.hpp:68-102
 *   MRS_COMP_ACCELERATION_HDG        acceleration[3] heading          Rd[9] throttle                  acceleration_controller.hpp:44-97
 *   MRS_COMP_ACCELERATION_HDG_RATE   acceleration[3] heading_rate     tilt[3] heading_rate throttle   acceleration_controller.hpp:103-122
 *   MRS_COMP_ATTITUDE                Rd[9] throttle                   rate[3] throttle                attitude_controller.hpp:79-100
 *   MRS_COMP_TILT_HDG_RATE           tilt[3] heading_rate throttle    rate[3] throttle                attitude_controller.hpp:106-145
 *   MRS_COMP_RATE                    rate[3] throttle                 roll pitch yaw throttle         rate_controller.hpp:67-81 */
enum {
  MRS_COMP_REORTH = 1, MRS_COMP_MODEL_RHS, MRS_COMP_MIXER, MRS_COMP_POSITION, MRS_COMP_VELOCITY, MRS_COMP_ACCELERATION_HDG,
  MRS_COMP_ACCELERATION_HDG_RATE, MRS_COMP_ATTITUDE, MRS_COMP_TILT_HDG_RATE, MRS_COMP_RATE
};
int mrs_swarm_debug_component(mrs_swarm_t* s, int32_t component, int32_t first, int32_t count, const double* in, int32_t in_stride, double* out,
                              int32_t out_stride, double dt);

/* measurement hook: average device time (ms) of ONE neighbour search of the single-GPU collision pass (pack + insert, then the
 * list-building query — what replaces nanoflann's per-tick kd-tree build + radius searches, src/multirotor_simulator.cpp:303-326),
 * `reps` searches back to back between two hipEvents on the swarm's stream.  Latches the forces / crash flags of
 * handleCollisions(true, crash, rebounce) on the current positions. */
int mrs_swarm_debug_search_ms(mrs_swarm_t* s, int32_t reps, int32_t crash, double rebounce, double* avg_ms);

/* test hook: ONE forced neighbour search on the current positions (it latches the forces / crash flags of
 * handleCollisions(true, crash, rebounce)), then the lists it built: count[i] = listed neighbours of UAV i (0 for a UAV with
 * more neighbours than a list holds), nbr[r * n + i] = the r-th of them in ascending index, r < min(count[i], *list_cap); rows >= count[i]
 * hold stale values.  `nbr` holds list_cap_in rows of n entries; *list_cap returns the library's list capacity.  What the lists must
 * hold (a superset of nanoflann's radiusSearch(3.0) result, src/multirotor_simulator.cpp:326): every UAV closer than sqrt(3) + skin. */
int mrs_swarm_debug_neighbour_lists(mrs_swarm_t* s, int32_t crash, double rebounce, uint32_t* count, uint32_t* nbr, int32_t list_cap_in, int32_t* list_cap,
                                    double* list_radius);

/* timing helper: average device time (ms) per step-kernel launch of the last mrs_swarm_step_n / mrs_swarm_tick_n call,
 * measured with hipEvents on the swarm's stream.  mode 1: one event pair around the whole region (elapsed / launches,
 * inter-launch gaps included, no perturbation); mode 2: one pair around every launch (perturbs the region); 0: off */
int mrs_swarm_last_step_kernel_ms(mrs_swarm_t* s, double* avg_ms, int32_t* n_launches);
int mrs_swarm_set_profiling(mrs_swarm_t* s, int32_t mode);

/* ---- device-resident callers: commands, observations, resets and crash flags in caller-owned DEVICE memory ----
 * For a controller, policy or reward that lives on the same GPU (a torch module): the calls below batch the host-pointer calls named
 * next to them, but read and write device rows of the swarm's device, so nothing crosses PCIe.  Row k always belongs to UAV first + k;
 * a row holds `stride` elements of `dtype` (FP64, or FP32: a round-to-nearest cast of the FP64 value on the way out, widened exactly
 * on the way in).
 *
 * Stream order: `ext_stream` (a hipStream_t; 0 = the null stream, which is what torch's default stream reports) is always honoured.
 * Each call records an event on ext_stream and makes the swarm's stream wait on it, queues its kernel on the swarm's stream, records a
 * second event there and makes ext_stream wait on that.  So what the caller queued on ext_stream before the call is what the kernel
 * reads, work queued on ext_stream after the call sees the result, and a caching allocator cannot hand an input buffer out again while
 * the kernel still reads it.  The two events belong to the swarm and are reused.  A caller that wants no fence passes the swarm's own
 * stream (mrs_swarm_stream).
 *
 * Host waits: with collisions off none of these calls waits for the device.  With collisions on (lazily evaluated collision ticks,
 * mrs_swarm_tick_n) they wait exactly where their host counterparts do: set_input_device and gather_device enter like
 * mrs_swarm_set_input (the launches queued so far must have run, so a launch that turned into a no-op is replayed before the kernel is
 * queued; a pending collision tick stays pending), get_crashed_device and reset_device like every state call (the pending collision
 * tick is evaluated first: crash mode sets flags there).
 *
 * Every argument is checked on the host before anything is launched: ranges (MRS_ERR_RANGE), mode, dtype, stride >= width, the
 * actuator width against n_motors, non-null pointers, and that every pointer is device memory of the swarm's device (MRS_ERR_ARG).
 * On a sharded swarm gather, commands and crash flags act on the local shard; reset_device returns MRS_ERR_ARG there. */
enum { MRS_DTYPE_F64 = 0, MRS_DTYPE_F32 = 1 };
/* observation groups of mrs_swarm_gather_device, concatenated in bit order */
enum {
  MRS_OBS_POS      = 1 << 0, /* 3: x                                        MultirotorModel::State::x  multirotor_model.hpp:92 */
  MRS_OBS_VEL      = 1 << 1, /* 3: v, world frame                                                 ::v  :93 */
  MRS_OBS_VEL_BODY = 1 << 2, /* 3: R^T v, as mrs_uav_output_t.velocity_body          src/uav_system_ros.cpp:356-360 */
  MRS_OBS_ROT      = 1 << 3, /* 9: R, row-major                                                   ::R  :95 */
  MRS_OBS_QUAT     = 1 << 4, /* 4: x, y, z, w, as mrs_uav_output_t.orientation       src/uav_system_ros.cpp:350 */
  MRS_OBS_OMEGA    = 1 << 5, /* 3: omega                                                      ::omega  :96 */
  MRS_OBS_IMU      = 1 << 6, /* 3: UavSystem::getImuAcceleration                               uav_system.hpp:424 */
  MRS_OBS_RPM      = 1 << 7, /* 8: motor_rpm, 0 past n_motors (as mrs_uav_state_t)          ::motor_rpm  :97 */
  MRS_OBS_ALL      = 0xFF    /* 36 */
};
/* the device a swarm lives on (the device its pointers must belong to) */
int mrs_swarm_device(const mrs_swarm_t* s, int32_t* device_id);
/* elements per row of mrs_swarm_gather_device for `groups` (0 -> 0; unknown bits -> MRS_ERR_ARG); host only, no GPU */
int mrs_swarm_gather_width(uint32_t groups, int32_t* width);
/* UavSystem::setInput(...) x11 (uav_system.hpp:175-248) for UAVs [first, first+count) from device rows: the payload layouts and widths
 * of mrs_swarm_set_input (ACTUATOR: min(stride, MRS_MAX_MOTORS) motors), written to the command columns and the mode by one kernel */
int mrs_swarm_set_input_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, const void* dev_rows, int32_t dtype, int32_t stride,
                               void* ext_stream);
/* UavSystem::getState / getImuAcceleration (uav_system.hpp:386,424) and the odometry / pose fields of mrs_uav_output_t for UAVs
 * [first, first+count): the MRS_OBS_* groups of `groups` into row k, elements [0, width); elements [width, stride) are not touched */
int mrs_swarm_gather_device(mrs_swarm_t* s, int32_t first, int32_t count, uint32_t groups, void* dev_rows, int32_t dtype, int32_t stride,
                            void* ext_stream);
/* UavSystem::hasCrashed (uav_system.hpp:286) of UAVs [first, first+count): dev_out[k] = 1 or 0 */
int mrs_swarm_get_crashed_device(mrs_swarm_t* s, int32_t first, int32_t count, uint8_t* dev_out, void* ext_stream);
/* UavSystem(params, spawn_pos, spawn_heading) again (uav_system.hpp:144-153, what mrs_swarm_construct writes) for each UAV first + k
 * whose dev_mask[k] != 0, on the device: state, IMU, external force and PID columns zero, R = AngleAxis(-heading[k], z), x = pos[k]
 * (count x 3), the initial height = pos[k].z, crash flag cleared, takeoff patch = takeoff_patch_enabled.  dev_heading may be NULL
 * (heading 0).  pos and heading are read for masked rows only.  The one difference from mrs_swarm_construct: the command, the
 * feed-forwards, the input mode, the airframe type and the hold flag are KEPT (the host's mirror of the modes cannot follow a device-side
 * mask without a synchronisation; a loop writes the next command right after the reset anyway).  The next collision tick repeats the
 * neighbour search, as after a host write of positions.  MRS_ERR_ARG on a sharded swarm. */
int mrs_swarm_reset_device(mrs_swarm_t* s, int32_t first, int32_t count, const uint8_t* dev_mask, const void* dev_pos, const void* dev_heading,
                           int32_t dtype, int32_t takeoff_patch_enabled, void* ext_stream);

/* ---- nearest-neighbour observations: the k closest other UAVs within a sensing radius, for swarm policies on the device ----
 * Query set: UAVs [first, first+count).  Candidates: every UAV of the swarm with a finite position, crashed ones included (obstacles);
 * a UAV is never its own neighbour, and a query UAV with a non-finite position gets an empty row.  The neighbours of i are the UAVs
 * j != i with d2 < radius * radius, d2 = ((dx*dx) + dy*dy) + dz*dz, dx = x_j - x_i, all in FP64 without FMA contraction (radius * radius
 * rounded once on the host).  The first k of them by ascending (d2, j) are listed, nearest first; ties in d2 go to the lower index, so
 * the result does not depend on arrival order or grid layout.
 * Output row r belongs to UAV first + r: k slots of mrs_nearest_width(fields, 1) elements each, the MRS_NN_* fields of the slot
 * concatenated in bit order (FP64, or the round-to-nearest FP32 cast); empty slots are 0, their index -1.  Elements [k*width, stride) of
 * a row and [k, index_stride) of an index row are not touched.  dev_index (count x index_stride int32) and dev_count (count int32: the
 * neighbours listed, at most k) may be NULL; dev_rows may be NULL when fields == 0; at least one output must be given.
 * State, stream fence and host waits are those of mrs_swarm_gather_device (the call enters like it: a pending collision tick stays
 * pending).  The call writes no simulation state and leaves the collision pass's tables alone: its scratch is its own (grown on demand,
 * freed by mrs_swarm_destroy, not copied by clone).  Every argument is checked before anything is launched: ranges (MRS_ERR_RANGE),
 * 1 <= k <= MRS_NN_MAX_K, a finite radius > 0, known field bits, stride >= k * width, index_stride >= k, and that every given pointer
 * is device memory of the swarm's device large enough for its rows (MRS_ERR_ARG).  MRS_ERR_ARG on a sharded swarm. */
/* fields of one neighbour slot of mrs_swarm_nearest_device, concatenated in bit order */
enum {
  MRS_NN_REL_POS      = 1 << 0, /* 3: x_j - x_i, world frame */
  MRS_NN_REL_POS_BODY = 1 << 1, /* 3: R_i^T (x_j - x_i), as MRS_OBS_VEL_BODY forms R^T v */
  MRS_NN_REL_VEL      = 1 << 2, /* 3: v_j - v_i, world frame */
  MRS_NN_REL_VEL_BODY = 1 << 3, /* 3: R_i^T (v_j - v_i) */
  MRS_NN_DIST         = 1 << 4, /* 1: sqrt(d2) */
  MRS_NN_ALL          = 0x1F    /* 13 */
};
enum { MRS_NN_MAX_K = 32 };
/* elements per row of mrs_swarm_nearest_device: k * (width of one slot of `fields`) (fields 0 -> 0; unknown bits or k outside
 * [1, MRS_NN_MAX_K] -> MRS_ERR_ARG); host only, no GPU */
int mrs_nearest_width(uint32_t fields, int32_t k, int32_t* width);
int mrs_swarm_nearest_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t k, double radius, uint32_t fields, void* dev_rows, int32_t dtype,
                             int32_t stride, int32_t* dev_index, int32_t index_stride, int32_t* dev_count, void* ext_stream);

/* ---- proximity cost: a per-UAV separation penalty over the k nearest UAVs, added into the cost vector of the cost rollouts ----
 * The search of mrs_swarm_nearest_device followed by a reduction, so that no neighbour row is written and read back.  Neighbours are
 * word for word those of mrs_swarm_nearest_device: query set [first, first+count); candidates every UAV with a finite position, crashed
 * ones included; a UAV is never its own neighbour; equal world labels only, once a label was ever set; d2 = ((dx*dx) + dy*dy) + dz*dz
 * < radius * radius in FP64 without contraction (radius * radius rounded once on the host); order ascending (d2, j).  Let `found` be the
 * number of such neighbours and nf = min(found, k).  Evaluation of UAV first + r:
 *     term = +0.0
 *     for m in [0, nf):                    (nearest first: the slot order of mrs_swarm_nearest_device)
 *       MRS_PROX_HINGE2 : d = sqrt(d2_m) (as MRS_NN_DIST forms it);  g = radius - d;  term = term + (weight * g) * g
 *       MRS_PROX_INVERSE: term = term + weight / (d2_m + eps)
 *       MRS_PROX_COUNT  : term = term + weight
 *     c = accumulate ? dev_cost[r] : +0.0
 *     c = c + term
 *     dev_cost[r] = c
 *     if (dev_found) dev_found[r] = found
 * dev_found is NOT capped by k: a value above k says the term left neighbours out.  Everything is FP64, one rounding per operation, no
 * fused multiply-add, and nothing is special-cased: a query UAV with a non-finite position adds +0.0, coincident UAVs under INVERSE with
 * eps == 0 give what IEEE gives (weight / 0), any weight is legal.  With accumulate == 0 the result does not depend on what dev_cost
 * held (it is not read); elements outside [0, count) are not touched.
 * Entry, stream fence and host waits are those of mrs_swarm_nearest_device: no simulation state is written, the collision pass's
 * tables are left alone, a pending collision tick stays pending; the scratch is that of mrs_swarm_nearest_device.  A horizon cut at its
 * evaluation points reads rollout_tick_cost(accumulate) -> proximity_cost(accumulate) -> rollout_tick_cost(accumulate) -> ..., and the
 * proximity calls between the pieces leave the simulation bit for bit as it was.
 * Every argument is checked before any launch, and a refused call changes nothing: the range MRS_ERR_RANGE; MRS_ERR_ARG for k outside
 * [1, MRS_NN_MAX_K], a radius that is not finite and > 0, an unknown kind, under INVERSE an eps that is NaN, infinite or negative (eps is
 * ignored by the other kinds), a NULL dev_cost, a dev_cost or dev_found that is not device memory of the swarm's device holding `count`
 * elements, and a sharded swarm.  count == 0 is MRS_OK. */
enum { MRS_PROX_HINGE2 = 0, MRS_PROX_INVERSE = 1, MRS_PROX_COUNT = 2 };
int mrs_swarm_proximity_cost_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t k, double radius, int32_t kind, double weight, double eps,
                                    double* dev_cost, int32_t accumulate, int32_t* dev_found /* may be NULL */, void* ext_stream);

/* ---- static obstacles: a set of solids owned by the swarm, observed (nearest_obstacles) and penalised (obstacle_cost), never hit ----
 * Obstacles affect nothing but the two queries below: UAVs fly through them, and the step, the collision pass and every other call
 * behave exactly as without a set.  (Counting penetrations and masking a reset is the caller's business: MRS_PROX_COUNT with the body
 * radius.  A caller who wants UAVs to crash into obstacles asks for it: mrs_swarm_obstacle_contacts_device, "obstacle contacts" below.)
 * Kinds: MRS_OBST_SPHERE centre c, radius h[0]; MRS_OBST_BOX axis-aligned, centre c, half-extents h; MRS_OBST_CYLINDER vertical, centre c,
 * radius h[0], half-height h[2] (+inf: a pillar without ends; h[1] is not used, nor are a sphere's h[1], h[2]).
 * mrs_swarm_set_obstacles replaces the set (count 0 clears it) after validating all of it on the host: c finite; the used h entries
 * finite and >= 0, except a cylinder's h[2], which may be +inf; a known kind; no unknown flag bits; reserved == 0; count in
 * [0, MRS_OBST_MAX]; a non-NULL array when count > 0.  Anything else is MRS_ERR_ARG and changes nothing.  The setter is ordered behind
 * earlier work on the swarm's stream, writes no simulation state, and leaves a pending collision tick pending; it is legal on a sharded
 * swarm (the queries are not).  The set belongs to the swarm: mrs_swarm_clone and mrs_swarm_clone_resized copy it, mrs_swarm_destroy
 * frees it, snapshots and mrs_swarm_copy_uavs do not touch it.
 * mrs_swarm_get_obstacles: *count (may not be NULL) receives the size of the set; the set is copied to `out` when out != NULL, which then
 * needs capacity >= the size (MRS_ERR_ARG otherwise, *count still written).
 * An obstacle applies to UAV i if it carries MRS_OBST_ALL_WORLDS or its `world` equals the UAV's label (mrs_swarm_set_worlds; every label
 * is 0 until a setter says otherwise).
 *
 * Signed distance sd and offset rel (from the UAV to the closest point of the solid; zero inside) of a UAV at p, d = p - c per component.
 * Everything is FP64, one rounding per operation, no fused multiply-add; max(a,b) := a < b ? b : a and min(a,b) := b < a ? b : a,
 * literally (signed zeros follow the comparisons):
 *   SPHERE   rho = sqrt(((dx*dx) + dy*dy) + dz*dz);  sd = rho - r;  t = rho > r ? (r / rho - 1.0) : 0.0;  rel = (t*dx, t*dy, t*dz)
 *   BOX      a_c = |d_c| - h_c;  m_c = max(a_c, 0.0);  sd = sqrt(((m0*m0) + m1*m1) + m2*m2) + min(max(a0, max(a1, a2)), 0.0);
 *            u_c = min(max(d_c, -h_c), h_c);  rel_c = u_c - d_c
 *   CYLINDER rho = sqrt((dx*dx) + dy*dy);  a_r = rho - r;  a_z = |dz| - hz;
 *            sd = sqrt((max(a_r,0.0)*max(a_r,0.0)) + max(a_z,0.0)*max(a_z,0.0)) + min(max(a_r, a_z), 0.0);
 *            t = rho > r ? (r / rho - 1.0) : 0.0;  rel = (t*dx, t*dy, min(max(dz, -hz), hz) - dz)
 * The obstacles of UAV i are those that apply to it with sd < radius; the first k by ascending (sd, obstacle index) are listed, so the
 * result depends on neither traversal order nor grid layout.  A UAV with a non-finite position has no obstacles.
 *
 * mrs_swarm_nearest_obstacles_device: rows, slots (the MRS_ON_* fields concatenated in bit order, k slots of mrs_obstacle_width(fields, 1)
 * elements), empty slots (zeros, index -1), untouched slack ([k*width, stride) of a row, [k, index_stride) of an index row), NULL rules
 * (dev_index and dev_count may be NULL, dev_rows when fields == 0, at least one output), dtype handling (FP32 is the round-to-nearest
 * cast of the FP64 value), stream fence and entry are those of mrs_swarm_nearest_device; dev_index holds obstacle indices, dev_count
 * min(found, k).
 * mrs_swarm_obstacle_cost_device: the evaluation of mrs_swarm_proximity_cost_device with sd_m in place of sqrt(d2_m), nearest first:
 *     term = +0.0;  for m in [0, min(found, k)):
 *       MRS_PROX_HINGE2: g = radius - sd_m;  term = term + (weight * g) * g        (grows the deeper the UAV is inside)
 *       MRS_PROX_COUNT : term = term + weight                                      (MRS_PROX_INVERSE is refused)
 *     c = accumulate ? dev_cost[r] : +0.0;  c = c + term;  dev_cost[r] = c;  if (dev_found) dev_found[r] = found   (NOT capped by k)
 * A horizon cut at its evaluation points reads rollout_tick_cost(accumulate) -> obstacle_cost(accumulate) -> ..., bit for bit.
 * Both calls: a pending collision tick stays pending and the simulation is left bit for bit as it was; an empty set is legal (empty
 * rows, +0.0, found 0); every argument is checked before any launch and a refused call changes nothing: ranges MRS_ERR_RANGE;
 * MRS_ERR_ARG for k outside [1, MRS_OBST_MAX_K], a radius that is not finite and > 0, unknown fields or kind, pointers and strides as in
 * mrs_swarm_nearest_device / mrs_swarm_proximity_cost_device, and a sharded swarm; count == 0 is MRS_OK.
 * The search structure is a uniform grid built on the host when a query first needs it for its radius, cached (one entry) until the
 * radius changes or the set is replaced, and uploaded on the swarm's stream: a cell lists every obstacle whose bounding box, grown by
 * the radius, overlaps it, so a query reads the one cell that contains p and tests every listed obstacle literally.
 * mrs_swarm_obstacle_stats describes the set and the cached grid (zeros where no grid is cached); grid_builds counts builds so far. */
enum { MRS_OBST_SPHERE = 0, MRS_OBST_BOX = 1, MRS_OBST_CYLINDER = 2 };
enum { MRS_OBST_ALL_WORLDS = 1u }; /* flags: seen by UAVs of every world label */
enum { MRS_OBST_MAX = 1 << 20, MRS_OBST_MAX_K = 32 };
typedef struct {
  int32_t  kind, world;
  uint32_t flags, reserved;
  double   c[3], h[3];
} mrs_obstacle_t; /* 64 B */
typedef struct {
  int32_t count;        /* obstacles in the set */
  int32_t dims[3];      /* cells per axis of the cached grid */
  int64_t cells;        /* dims[0] * dims[1] * dims[2] */
  int64_t list_items;   /* entries of all cell lists together */
  int32_t longest_list; /* entries of the longest cell list */
  int32_t reserved;
  int64_t grid_builds;  /* grids built for this swarm so far */
  double  grid_radius;  /* the query radius the cached grid serves (0: none cached) */
  double  cell_edge;    /* edge of a cell of the cached grid */
} mrs_obstacle_stats_t; /* 64 B */
int mrs_swarm_set_obstacles(mrs_swarm_t* s, int32_t count, const mrs_obstacle_t* obstacles);
int mrs_swarm_get_obstacles(const mrs_swarm_t* s, int32_t capacity, mrs_obstacle_t* out, int32_t* count);
int mrs_swarm_obstacle_stats(mrs_swarm_t* s, mrs_obstacle_stats_t* stats);
/* fields of one obstacle slot of mrs_swarm_nearest_obstacles_device, concatenated in bit order */
enum {
  MRS_ON_REL      = 1 << 0, /* 3: rel, world frame */
  MRS_ON_REL_BODY = 1 << 1, /* 3: R_i^T rel, as MRS_NN_REL_POS_BODY forms it */
  MRS_ON_DIST     = 1 << 2, /* 1: sd */
  MRS_ON_ALL      = 7
};
/* elements per row of mrs_swarm_nearest_obstacles_device: k * (width of one slot of `fields`) (fields 0 -> 0; unknown bits or k outside
 * [1, MRS_OBST_MAX_K] -> MRS_ERR_ARG); host only, no GPU */
int mrs_obstacle_width(uint32_t fields, int32_t k, int32_t* width);
int mrs_swarm_nearest_obstacles_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t k, double radius, uint32_t fields, void* dev_rows,
                                       int32_t dtype, int32_t stride, int32_t* dev_index, int32_t index_stride, int32_t* dev_count, void* ext_stream);
int mrs_swarm_obstacle_cost_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t k, double radius, int32_t kind, double weight,
                                   double* dev_cost, int32_t accumulate, int32_t* dev_found /* may be NULL, NOT capped by k */, void* ext_stream);

/* ---- range scans: a pattern of beams per UAV cast against the static obstacles and the ground plane, one range per beam ----
 * The observation of a perception-driven policy: a fixed angular layout with occlusion, which the k-nearest list above is not.  Beams see
 * the obstacle set and the ground plane and nothing else (not other UAVs); they start at the UAV's position.
 * The pattern belongs to the swarm, one for all its UAVs.  mrs_swarm_set_scan_beams replaces it by n_beams rows (bx, by, bz) after
 * validating all of it on the host: n_beams in [0, MRS_SCAN_MAX_BEAMS] (0 clears the pattern); a non-NULL array when n_beams > 0; every
 * row finite with |((bx*bx + by*by) + bz*bz) - 1.0| <= 1e-9 — beams are unit vectors, the kernel never normalises.  Anything else is
 * MRS_ERR_ARG and changes nothing.  Ordering and ownership are those of mrs_swarm_set_obstacles: ordered behind earlier work on the
 * swarm's stream, no simulation state written, a pending collision tick stays pending, legal on a sharded swarm (the scan is not);
 * mrs_swarm_clone and mrs_swarm_clone_resized copy the pattern, mrs_swarm_destroy frees it, snapshots and mrs_swarm_copy_uavs do not
 * touch it.  mrs_swarm_get_scan_beams: *n_beams (may not be NULL) receives the size of the pattern; the rows are copied to `out` when
 * out != NULL, which then needs capacity >= that size in rows (MRS_ERR_ARG otherwise, *n_beams still written).
 *
 * mrs_swarm_range_scan_device: row r of dev_ranges holds the n_beams ranges of UAV first + r, FP64, or FP32 as the round-to-nearest cast
 * of the FP64 value; stride >= n_beams elements, the slack [n_beams, stride) of a row is not touched.  dev_hit (may be NULL; int32 rows of
 * hit_stride >= n_beams, slack untouched) holds per beam the index of the obstacle hit, MRS_SCAN_HIT_NONE (the range is then max_range)
 * or MRS_SCAN_HIT_GROUND.
 * Beam b of a UAV at p with attitude R (row-major) is p + t u, t >= 0, with u = b in the world frame, or under MRS_SCAN_BODY_FRAME
 *     u_c = (R[c][0]*bx + R[c][1]*by) + R[c][2]*bz.
 * Everything is FP64, one rounding per operation, no fused multiply-add; max and min are the comparisons of the static obstacles
 * (max(a,b) := a < b ? b : a, min(a,b) := b < a ? b : a); every comparison below is written so that a NaN misses.
 * Candidates of UAV i, stated without reference to any search structure: obstacle m is a candidate if it applies to i (the world rule of
 * the static obstacles) and, with d = p - c, on every axis a:  |d_a| - hb_a < max_range, where hb is the half-extent of m's bounding box
 * (sphere (r, r, r); box h; cylinder (r, r, hz)).  The gate only cuts hits that could not lie within max_range anyway; it is what makes
 * the result independent of the grid (below).
 * Range t_m of a candidate: the closed solid is entered at t_m >= 0, 0 when p lies in it or on its surface; otherwise a miss.
 *   slab(d, u, h; enter, exit) — one axis of |d + t u| <= h:
 *            u == 0.0:  miss if |d| > h, else no bound (no division, and no 0 * inf ever forms);
 *            else t1 = (-h - d) / u;  t2 = (h - d) / u;  enter = max(enter, min(t1, t2));  exit = min(exit, max(t1, t2))
 *   SPHERE   cc = (((dx*dx) + dy*dy) + dz*dz) - r*r;  cc <= 0.0 -> t = 0.0;
 *            b = ((dx*ux) + dy*uy) + dz*uz;  not b < 0.0 -> miss;  disc = b*b - cc;  not disc >= 0.0 -> miss;
 *            t = cc / (-b + sqrt(disc))                                               (the form without cancellation)
 *   BOX      enter = 0.0, exit = +inf;  slab(dx, ux, h0), slab(dy, uy, h1), slab(dz, uz, h2) in this order;
 *            enter <= exit -> t = enter, else miss
 *   CYLINDER enter = 0.0, exit = +inf;  slab(dz, uz, hz)  (hz = +inf, uz == 0.0 tested first: the pillar);
 *            a = (ux*ux) + uy*uy;  cc = ((dx*dx) + dy*dy) - r*r;
 *            a == 0.0 (a vertical beam):  not cc <= 0.0 -> miss, else no bound;
 *            else b = (dx*ux) + dy*uy;  disc = b*b - a*cc;  not disc >= 0.0 -> miss;  q = -b + sqrt(disc);
 *                 cc <= 0.0:  exit = min(exit, q / a);
 *                 else  not b < 0.0 -> miss;  enter = max(enter, cc / q);  exit = min(exit, q / a);
 *            enter <= exit -> t = enter, else miss
 * Selection: best = max_range, hit = MRS_SCAN_HIT_NONE; for the candidates in ascending obstacle index: t_m < best -> best = t_m,
 * hit = m.  So a candidate hits only with t_m < max_range, strictly; the smallest range wins and among equal ranges the lowest index.
 * Under MRS_SCAN_GROUND the plane z = ground_z of the UAV's airframe type (the value the rangefinder of mrs_swarm_get_outputs reads,
 * whatever ground_enabled says) is considered last:  p_z <= ground_z -> t = 0.0;  else u_z < 0.0 -> t = (p_z - ground_z) / (-u_z);  else
 * miss;  t < best -> best = t, hit = MRS_SCAN_HIT_GROUND (an obstacle at the same range keeps the beam).  A UAV with a non-finite
 * position gets max_range and MRS_SCAN_HIT_NONE on every beam.
 * The search structure is the grid of the static obstacles built for radius = max_range, in a cache entry of the scans' own (one
 * entry, kept until max_range changes or the set is replaced; a loop that alternates obstacle_cost(radius) with range_scan(max_range)
 * builds two grids, not one per call).  The cell that contains p lists every candidate: the gate is the per-axis inequality the grid's
 * coverage proof passes through.  mrs_swarm_obstacle_stats keeps describing the queries' grid; grid_builds counts both.
 * Entry, stream fence and NULL rules are those of mrs_swarm_nearest_obstacles_device: a pending collision tick stays pending and the
 * simulation is left bit for bit as it was; an empty obstacle set is legal.  Every argument is checked before any launch and a refused
 * call changes nothing: the range MRS_ERR_RANGE; MRS_ERR_ARG for no pattern set, a max_range that is not finite and > 0, unknown flag
 * bits, a bad dtype, strides below n_beams, a NULL dev_ranges, a dev_ranges or dev_hit that is not device memory of the swarm's device
 * holding the rows, count * n_beams above 2^39 (one launch), and a sharded swarm; count == 0 is MRS_OK. */
enum { MRS_SCAN_MAX_BEAMS = 4096 };
enum { MRS_SCAN_BODY_FRAME = 1u << 0, MRS_SCAN_GROUND = 1u << 1 }; /* flags of mrs_swarm_range_scan_device */
enum { MRS_SCAN_HIT_NONE = -1, MRS_SCAN_HIT_GROUND = -2 };         /* values of dev_hit besides obstacle indices */
int mrs_swarm_set_scan_beams(mrs_swarm_t* s, int32_t n_beams, const double* dirs /* n_beams x 3 */);
int mrs_swarm_get_scan_beams(const mrs_swarm_t* s, int32_t capacity, double* out, int32_t* n_beams);
int mrs_swarm_range_scan_device(mrs_swarm_t* s, int32_t first, int32_t count, double max_range, uint32_t flags, void* dev_ranges, int32_t dtype,
                                int32_t stride, int32_t* dev_hit /* may be NULL */, int32_t hit_stride, void* ext_stream);

/* ---- range scans that see other UAVs: the scan above, and every other UAV of the observer's world as a closed sphere ----
 * In a swarm, what most often fills a UAV's lidar is another UAV.  mrs_swarm_range_scan_uavs_device is mrs_swarm_range_scan_device (same
 * pattern, same beams, same obstacles, same ground, same rows) with the UAVs considered between the obstacles and the ground; the old call
 * stays what it is.  Arguments, checks, their order and their messages are those of mrs_swarm_range_scan_device (the function name
 * aside): the range, not on a sharded swarm, a pattern set, max_range finite and > 0, flags within MRS_SCAN_BODY_FRAME | MRS_SCAN_GROUND,
 * dtype, stride, dev_hit / hit_stride; then dev_uav (may be NULL, also where dev_hit is given, and given where dev_hit is NULL): int32
 * rows of uav_stride >= n_beams, slack untouched, per beam the index of the UAV hit or -1; one launch holds count * ceil(n_beams / 64)
 * < 2^31 blocks; count == 0 is MRS_OK after the checks; dev_ranges, dev_hit and dev_uav must be device memory of the swarm's device
 * holding their rows.  A refused call changes nothing.
 * What a UAV is to a beam: UAV j is the closed sphere centred at its position p_j with radius rad_j = arm_length + prop_radius of its
 * airframe type (one rounded FP64 addition: the prefix (marm + mprop) of the collision criterion), read from the airframe table, which is
 * brought up to date before the launch.
 * Candidates of observer i, stated without reference to any search structure: every UAV j of the swarm (all n of them, not only those of
 * [first, first + count)) with j != i, world[j] == world[i] (all 0 when no label was ever set) and, on every axis a,
 *     |p_i[a] - p_j[a]| - rad_j < max_range
 * — the gate of the range scans applied to the sphere record {MRS_OBST_SPHERE, c = p_j, h[0] = rad_j}.  A non-finite p_j fails it by
 * itself (every comparison is written so that a NaN misses).  Crashed UAVs are seen like any other.
 * Range t_j of a candidate: the SPHERE lines of the range scans for that record, from p_i along the beam direction u formed as above;
 * 0.0 when p_i lies in or on the sphere, otherwise possibly a miss.
 * Selection per beam: (1) the obstacles exactly as above: best = max_range, hit = MRS_SCAN_HIT_NONE, ascending index, strict <.
 * (2) Among the candidate UAVs the lexicographic minimum of (t_j, j) (a NaN t_j never taken); it takes the beam only if t_j < best,
 * strictly — an obstacle at the same range keeps the beam: best = t_j, hit = MRS_UAVSCAN_HIT_UAV, uav = j.  (3) Under MRS_SCAN_GROUND the
 * plane as above: t < best -> best = t, hit = MRS_SCAN_HIT_GROUND, uav = -1.  dev_uav is -1 wherever hit != MRS_UAVSCAN_HIT_UAV.  An
 * observer with a non-finite position gets max_range, MRS_SCAN_HIT_NONE and -1 on every beam.  The range is FP64, or its
 * round-to-nearest FP32 cast.
 * The search structures are the scans' cached obstacle grid and the hash of mrs_swarm_nearest_device built for radius = max_range +
 * the largest rad of the swarm's airframe table, in the scratch that call uses; the kernel applies j != i, world equality and the gate
 * literally to what the 27 buckets around the observer's cell list, so the result depends on neither.
 * Effect on the simulation: none.  Entry and stream fence are those of mrs_swarm_range_scan_device: a pending collision tick stays
 * pending, the caller's stream is fenced in and out, and a horizon cut at this call is the uncut horizon bit for bit. */
enum { MRS_UAVSCAN_HIT_UAV = -3 }; /* value of dev_hit besides those of the range scans */
int mrs_swarm_range_scan_uavs_device(mrs_swarm_t* s, int32_t first, int32_t count, double max_range, uint32_t flags, void* dev_ranges,
                                     int32_t dtype, int32_t stride, int32_t* dev_hit /* may be NULL */, int32_t hit_stride,
                                     int32_t* dev_uav /* may be NULL */, int32_t uav_stride, void* ext_stream);

/* ---- obstacle contacts: which UAVs touch a static obstacle, reported on the device and, on request, marked crashed ----
 * The queries and scans above observe the obstacles; this call is the one that lets a UAV hit them.  It reports, per UAV, whether its
 * body sphere touches an obstacle, and under MRS_CONTACT_CRASH marks the touching UAVs crashed exactly as UavSystem::crash() /
 * mrs_swarm_crash does (uav_system.hpp:278): the next makeStep zeroes their motors and they fall.  Nothing else about the simulation
 * changes: no rebound force, and without the call (or without the flag) UAVs keep flying through obstacles as before.
 * For UAV i = first + k, everything FP64, one rounding per operation:
 *     rad_i = arm_length + prop_radius   of its airframe type (the sphere of mrs_swarm_range_scan_uavs_device, the prefix of the collision
 *                                        criterion), read from the airframe table, which is brought up to date before the launch
 *     thr_i = rad_i + margin
 *     C_i   = { j : obstacle j applies to i (its world label, or MRS_OBST_ALL_WORLDS) and sd_ij < thr_i }     (strictly)
 * with sd_ij the signed distance of the static obstacles.  C_i is empty when a coordinate of p_i is not finite, and when thr_i is NaN
 * (the comparison misses).  The outputs are dense vectors of `count` elements, each pointer may be NULL:
 *     dev_hit[k]   = |C_i| > 0 ? 1 : 0
 *     dev_count[k] = |C_i|                                        (not capped)
 *     dev_index[k] = the j of the lexicographic minimum of (sd_ij, j) over C_i, or -1     (-0.0 == +0.0: such a tie goes to the lower index)
 *     dev_sd[k]    = that sd_ij, or +inf
 *     dev_cost[k]  = dev_cost[k] + hit_cost   where |C_i| > 0 (one addition); the element is not written elsewhere
 * and under MRS_CONTACT_CRASH the flag word of UAV i gets the crashed bit OR-ed in where |C_i| > 0; the state of a UAV that touches
 * nothing is not written.  The report is geometric: a crashed or held UAV is reported like any other, and marking twice is marking once.
 * Entry.  Without MRS_CONTACT_CRASH no simulation state is written and the call enters like mrs_swarm_obstacle_cost_device: a pending
 * collision tick stays pending, and a horizon cut at the call is the uncut horizon bit for bit.  With it the call enters like
 * mrs_swarm_crash and mrs_swarm_reset_device: a pending collision tick is evaluated first.  Both forms fence the caller's stream in and
 * out like the sibling calls.
 * Refused with MRS_ERR_ARG (MRS_ERR_RANGE for the range), nothing written: unknown flag bits; a margin that is not finite or < 0; a
 * hit_cost that is not finite when dev_cost is given; no output pointer and no MRS_CONTACT_CRASH; an output that is not device memory
 * of the swarm's device holding `count` elements; a sharded swarm; R = fl(rmax + margin) not finite or not > 0, rmax being the largest
 * finite rad of the swarm's airframe table.  count == 0 is MRS_OK after the checks.  An empty obstacle set is legal: nobody touches.
 * The search structure is the grid of the static obstacles built for R, in a cache entry of the contacts' own beside the queries' and
 * the scans' (a loop that alternates obstacle_cost, range_scan and obstacle_contacts builds three grids, not one per call;
 * mrs_swarm_obstacle_stats keeps describing the queries' grid, grid_builds counts all three).  thr_i <= R for every UAV (rounding is
 * monotone), so the one cell that contains p_i lists all of C_i; the kernel tests the world rule and sd < thr_i literally on what the
 * cell lists, so the result depends on neither R, nor unused airframe types, nor the grid.  (An airframe whose rad is not
 * finite is outside that argument.)
 * Tunnelling is the caller's business: the test is a snapshot, not a sweep.  A contact with an obstacle of thickness w is missed only if
 * the UAV travels more than w + 2 thr_i between two calls — at 10 m/s and the default airframe (thr = 0.4 m, margin 0) a call at least
 * every 80 ms sees a wall of zero thickness. */
enum { MRS_CONTACT_CRASH = 1 << 0 }; /* touching UAVs get crashed_, as UavSystem::crash() */
int mrs_swarm_obstacle_contacts_device(mrs_swarm_t* s, int32_t first, int32_t count, double margin, uint32_t flags, uint8_t* dev_hit,
                                       int32_t* dev_index, double* dev_sd, int32_t* dev_count, double* dev_cost, double hit_cost, void* ext_stream);

/* ---- line-of-sight neighbours: the k nearest UAVs that no static obstacle hides from the observer ----
 * mrs_swarm_nearest_device lists the UAV behind a wall exactly like the one in the open.  This call is the neighbour observation of a
 * camera- or UVDAR-based relative localisation: a neighbour is a neighbour only while there is a line of sight to it.  Arguments, rows,
 * slots and fields are those of mrs_swarm_nearest_device, which stays what it is; two more optional outputs count what is seen and what
 * is hidden.
 * Candidates of observer i = first + r, word for word those of mrs_swarm_nearest_device: every UAV j != i of the swarm with a finite
 * position (crashed ones included) and, once a label has been set, world_j == world_i, with
 *     dx = x_j - x_i (per axis);  d2 = ((dx*dx) + dy*dy) + dz*dz;  d2 < radius * radius
 * all in FP64 without FMA contraction, radius * radius rounded once on the host.
 * Sight line of candidate j:
 *     if d2 == 0:  visible, with no test (coincident UAVs see each other, inside a solid too)
 *     else         d = sqrt(d2);  u = (dx / d, dy / d, dz / d)       (three separately rounded divisions)
 *                  hidden  <=>  there is an obstacle o of the set that
 *                                 applies to i        (MRS_OBST_ALL_WORLDS, or o.world == world_i; world_i = 0 without labels),
 *                                 passes the gate     |p_a - c_a| - hb_a < radius on every axis a (hb: the half-extents of o's bounding
 *                                                     box; the gate of the range scans with max_range = radius), and
 *                                 t(o, p_i, u) < d    strictly, t the range at which the beam p_i + t u enters the closed solid o, as
 *                                                     the range scans define it (0 when p_i lies in or on o, +inf when it misses).
 * A NaN never hides (every comparison with it is false).  A target exactly on a surface (t == d) is visible.  An observer inside a solid
 * (t == 0 < d) sees only coincident UAVs.  The target is a point, UAV bodies hide nothing, and the observer's own body is ignored.
 * An obstacle that fails the gate cannot hide anything within the radius up to the rounding of the gate itself; it is part of the
 * contract so that the result does not depend on which obstacles a search structure happens to list.
 * Symmetry is NOT promised bit for bit: "i sees j" uses p_i and u, "j sees i" uses p_j and -u' with u' rounded from the opposite
 * offsets; a sight line that grazes a surface within rounding may be judged differently from its two ends.
 * Selection: the first k VISIBLE candidates by ascending (d2, j) — not the k nearest filtered afterwards: a hidden candidate takes no slot.
 * Outputs.  Row r, its k slots, the MRS_NN_* fields, empty slots (zeros, index -1), the untouched slack of rows and index rows and the
 * FP32 rows (the cast of the FP64 value) are exactly those of mrs_swarm_nearest_device.  dev_count[r] = min(visible, k);
 * dev_visible[r] = the number of visible candidates and dev_hidden[r] = the number of hidden ones, neither capped by k (int32[count],
 * each may be NULL).  An observer with a non-finite position gets an empty row and zeros.  dev_rows may be NULL when fields == 0; at
 * least one of dev_rows (with fields), dev_index, dev_count, dev_visible, dev_hidden must be given.
 * Obstacle sets.  An empty set, or none ever given, is legal: rows, index and count are then bit for bit those of
 * mrs_swarm_nearest_device, and hidden is 0.
 * Entry.  The call enters like mrs_swarm_nearest_device (a pending collision tick stays pending), fences the caller's stream in and out
 * and writes no simulation state.  Its scratch is that of mrs_swarm_nearest_device plus a cached obstacle grid of its own, keyed by
 * radius (counted in mrs_obstacle_stats_t::grid_builds, dropped by mrs_swarm_set_obstacles, not copied by clone); neither the grid nor
 * the hash can change a result bit.
 * Refusals, in this order, before anything is launched — a refused call changes no output byte and no state: the range (MRS_ERR_RANGE);
 * then MRS_ERR_ARG for a sharded swarm; unknown field bits; k outside [1, MRS_NN_MAX_K]; a radius that is not finite and > 0; no output
 * at all; with fields: an unknown dtype, stride < k * width; with dev_index: index_stride < k; then (count == 0 is MRS_OK here) dev_rows,
 * dev_index, dev_count, dev_visible, dev_hidden, in this order, that is not device memory of the swarm's device large enough for its
 * rows. */
int mrs_swarm_nearest_visible_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t k, double radius, uint32_t fields, void* dev_rows,
                                     int32_t dtype, int32_t stride, int32_t* dev_index, int32_t index_stride, int32_t* dev_count,
                                     int32_t* dev_visible, int32_t* dev_hidden, void* ext_stream);

/* ---- collision worlds: several scenes in one swarm that do not see each other (per-sample horizons of a sampling-based planner) ----
 * A world is a 32-bit label per UAV, 0 for every UAV until a setter says otherwise.  Two UAVs interact through the collision pass
 * (mrs_swarm_handle_collisions, mrs_swarm_tick_n, the tick rollouts), or appear in each other's rows of mrs_swarm_nearest_device, only
 * if their labels are equal: the neighbour set of i is { j : world[j] == world[i], j != i, d2(i,j) < 3.0 }, forces are summed in
 * ascending partner index, and the neighbour lists (and their capacity) hold same-world partners only.  A swarm whose UAVs carry W
 * distinct labels behaves, world by world, as W separate swarms that each hold the UAVs of one label in ascending index order and
 * receive the same calls — UAVs of different worlds may share coordinates (a forked scene: mrs_swarm_load_device with an index).
 * Labels are compared for equality and nothing else: every int32_t value is legal, there is no order.  Nothing else about a UAV follows
 * its label: its step, its commands, its ground plane and its slot index are what they were.
 * The label belongs to the slot, like the hold flag: mrs_swarm_construct, mrs_swarm_set_state*, mrs_swarm_load_device,
 * mrs_swarm_reset_device and mrs_swarm_copy_uavs (the destination's labels stay) leave it alone, a snapshot record does not hold it;
 * mrs_swarm_clone and mrs_swarm_clone_resized copy it (UAVs past the original's: 0).
 * Each call enters like a state call (a pending collision tick is evaluated first, under the old labels); a setter makes the next
 * collision tick repeat the neighbour search.  set_worlds_device honours ext_stream and checks its pointer like the other
 * device-resident calls.  Errors: ranges MRS_ERR_RANGE; a null pointer, for _device a pointer that is not memory of the swarm's device
 * holding `count` labels, or a setter on a sharded swarm MRS_ERR_ARG; count == 0 is MRS_OK; a refused call changes nothing.  Sharded
 * swarms have one world: mrs_swarm_comm_init* and mrs_swarm_handle_collisions_gathered return MRS_ERR_ARG on a swarm that holds a
 * label other than 0.  get_worlds returns zeros when no label was ever set, on a sharded swarm (its own UAVs) too. */
int mrs_swarm_set_worlds(mrs_swarm_t* s, int32_t first, int32_t count, const int32_t* worlds);
int mrs_swarm_get_worlds(mrs_swarm_t* s, int32_t first, int32_t count, int32_t* out);
int mrs_swarm_set_worlds_device(mrs_swarm_t* s, int32_t first, int32_t count, const int32_t* dev_worlds, void* ext_stream);

/* ---- state snapshots: the whole per-UAV simulation state into caller-owned device records and back (rewind, recorded resets, forks) ----
 * One record holds everything a step reads of a UAV besides its command, feed-forwards and mode, bit for bit.  The 60 doubles are the
 * state columns in their order (MultirotorModel::State x, v, v_prev, R row-major, omega, motor_rpm — all MRS_MAX_MOTORS columns as
 * stored —, the IMU acceleration, the latched external force, _initial_pos_(2), and the 24 PID words in the order of
 * mrs_swarm_get_pid).  v_prev is the value mrs_swarm_get_states returns (v unless setState split it).  `flags` holds the crash flag,
 * the mutated takeoff patch and whether v_prev differs from v; `airframe` is the swarm's parameter-set (type) index of the UAV;
 * `magic` is MRS_SNAP_MAGIC in every record save wrote.  496 B: an array of records keeps every row 16-B aligned. */
enum { MRS_SNAP_CRASHED = 1, MRS_SNAP_TAKEOFF = 2, MRS_SNAP_VPREV_SPLIT = 4 };
#define MRS_SNAP_MAGIC 0x50414E53u /* "SNAP" */
typedef struct {
  double   x[3], v[3], v_prev[3], R[9], omega[3];
  double   motor_rpm[MRS_MAX_MOTORS];
  double   imu_acceleration[3], external_force[3];
  double   initial_z;
  double   pid[24];
  uint32_t flags;    /* MRS_SNAP_* */
  uint32_t airframe; /* parameter-set (type) index */
  uint32_t magic;    /* MRS_SNAP_MAGIC */
  uint32_t _reserved;
} mrs_uav_snapshot_t;
/* save: the records of UAVs [first, first+count) into dev_records[0 .. count-1].  Enters like every state call: a pending collision
 * tick is evaluated first, so a record holds the latched collision force and crash flags handleCollisions would have left. */
int mrs_swarm_save_device(mrs_swarm_t* s, int32_t first, int32_t count, mrs_uav_snapshot_t* dev_records, void* ext_stream);
/* load: UAV first + k <- dev_records[k] (dev_index NULL; n_records >= count), or <- dev_records[dev_index[k]] (one record may go to many
 * UAVs).  Writes the state columns and the CRASHED / TAKEOFF / VPREV_SPLIT flags; keeps the command, the feed-forwards, the mode, the
 * airframe and the hold flag (as mrs_swarm_reset_device), so the host's mirrors stay valid.  A row is skipped and dev_status[k] (NULL,
 * or count bytes) says why: 0 loaded, 1 index -1, 2 the record's airframe is not the UAV's, 3 index outside [0, n_records), 4 no
 * MRS_SNAP_MAGIC (zeroed or never-written memory).  The next collision tick repeats the neighbour search, and the external force
 * acts (as after mrs_swarm_copy_uavs).
 * Both calls: stream fence and host waits of mrs_swarm_reset_device.  Every argument is checked before anything is launched: the range
 * (MRS_ERR_RANGE), and MRS_ERR_ARG for null, host or other-device pointers, rows past their allocation, records not 16-B aligned,
 * n_records < count without an index, and a sharded swarm. */
enum { MRS_SNAP_LOADED = 0, MRS_SNAP_SKIPPED = 1, MRS_SNAP_BAD_AIRFRAME = 2, MRS_SNAP_BAD_INDEX = 3, MRS_SNAP_BAD_MAGIC = 4 };
int mrs_swarm_load_device(mrs_swarm_t* s, int32_t first, int32_t count, const mrs_uav_snapshot_t* dev_records, int64_t n_records,
                          const int32_t* dev_index, uint8_t* dev_status, void* ext_stream);

/* ---- device-resident rollouts: per-step commands in, observations out (sampling-based planners: MPPI, CEM, random shooting) ----
 * Equals, bit for bit in LITERAL arithmetic, the loop
 *   for t in [0, n_steps):
 *     mrs_swarm_set_input_device(s, first, count, mode, row block t of dev_cmd, dtype, cmd_stride, ext_stream);
 *     mrs_swarm_step_n(s, dt, 1, 1);
 *     if (groups) mrs_swarm_gather_device(s, first, count, groups, row block t of dev_obs, dtype, obs_stride, ext_stream);
 * run as launches of fused steps that read each step's command row and write each step's observation row in the step kernel.
 * Command row (t, k), the setInput payload of UAV first + k before step t, starts at element ((size_t)t * count + k) * cmd_stride of
 * dev_cmd, with the layout and width of mrs_swarm_set_input_device (ACTUATOR: min(cmd_stride, MRS_MAX_MOTORS) motors, checked against
 * n_motors).  Observation row (t, k), the MRS_OBS_* groups of UAV first + k after step t, starts at element ((size_t)t * count + k) *
 * obs_stride of dev_obs: the layout and the bits of mrs_swarm_gather_device.  One dtype serves both (FP32 commands are widened
 * exactly, FP32 observations are the round-to-nearest cast); elements past a row's width are not touched.
 * Every UAV of the swarm is stepped, as mrs_swarm_step_n steps it; UAVs outside the range keep their own commands and modes.  A UAV on
 * hold is not stepped, but its command columns are written and its rows hold its unchanged state.  Afterwards the command columns of the
 * range hold row block n_steps - 1 and its mode is `mode`.  The call enters like a state call (a pending collision tick is evaluated
 * first and its force acts on the first step); collisions are not evaluated inside the rollout.  Stream order: ONE fence per call, that of
 * the other device-resident calls.  Every argument is checked before anything is launched, and a refused call changes nothing: the range
 * (MRS_ERR_RANGE), and MRS_ERR_ARG for the mode, the dtype, n_steps < 1, a dt that is not finite and > 0, cmd_stride below the command
 * width, unknown group bits, obs_stride below the gather width, dev_obs NULL with groups != 0, pointers that are not device memory of the
 * swarm's device or too small for all their rows, and a sharded swarm. */
int mrs_swarm_rollout_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_steps, const void* dev_cmd,
                             int32_t dtype, int32_t cmd_stride, uint32_t groups, void* dev_obs, int32_t obs_stride, void* ext_stream);

/* ---- control-rate rollouts: a command row block held for cmd_every steps, an observation row block every obs_every steps ----
 * The simulator steps at 1 kHz, what commands it at 50-100 Hz: UavSystem::setInput latches (uav_system.hpp:175-248), so a command stays
 * in force over the makeStep calls (:304-380) until the next setInput, and getState (:386) is asked for at the caller's own rate.
 * Equals, bit for bit in LITERAL arithmetic, the loop
 *   for t in [0, n_steps):
 *     if (t % cmd_every == 0)
 *       mrs_swarm_set_input_device(s, first, count, mode, row block t / cmd_every of dev_cmd, dtype, cmd_stride, ext_stream);
 *     mrs_swarm_step_n(s, dt, 1, 1);
 *     if (groups && (t + 1) % obs_every == 0)
 *       mrs_swarm_gather_device(s, first, count, groups, row block (t + 1) / obs_every - 1 of dev_obs, dtype, obs_stride, ext_stream);
 * dev_cmd holds n_steps / cmd_every row blocks and dev_obs n_steps / obs_every row blocks of `count` rows each: row (j, k) starts at
 * element ((size_t)j * count + k) * stride, as in mrs_swarm_rollout_device.  The two rates are independent of each other; each must be
 * >= 1 and divide n_steps (MRS_ERR_ARG).  obs_every == n_steps is the terminal-cost case: one row block per call.  Inside a command
 * block nothing is read from dev_cmd, and nothing is written to dev_obs except at the end of an observation block.
 * Everything else is the contract of mrs_swarm_rollout_device, which is this call with cmd_every = obs_every = 1: every UAV of the swarm
 * is stepped; a UAV on hold is not stepped, its command columns are written and its rows hold its unchanged state; afterwards the
 * command columns of the range hold the LAST row block and its mode is `mode`; the call enters like a state call; collisions are not
 * evaluated inside; ONE stream fence per call; every argument is checked before anything is launched and a refused call changes
 * nothing; refused on a sharded swarm.  The pointer checks use the decimated sizes: a dev_obs of exactly n_steps / obs_every row blocks
 * is accepted, one row short is refused. */
int mrs_swarm_rollout_rate_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_steps, int32_t cmd_every,
                                  int32_t obs_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride, uint32_t groups, void* dev_obs,
                                  int32_t obs_stride, void* ext_stream);

/* ---- device-resident external forces: applyForce from device rows, and a force row block every force_every steps of a rollout ----
 * UavSystem::applyForce (uav_system.hpp:293-298) latches external_force_ (multirotor_model.hpp:292-295), which enters v_dot at :346: the
 * simulator's one disturbance channel (gusts, pushes).  mrs_swarm_apply_force_device is mrs_swarm_apply_force with device rows: row k,
 * the force on UAV first + k in world frame and newtons, has component c at element k * stride + c of dev_force (FP64, or FP32 widened
 * exactly).  The force stays latched until the next applyForce or the next evaluated collision tick (with handleCollisions enabled that
 * tick sets every UAV's force, src/multirotor_simulator.cpp:357).  The call enters like the host call (a pending collision tick is
 * evaluated first: it writes the same columns) and is fenced like the other device-resident calls.  Checked before anything is
 * launched: the range (MRS_ERR_RANGE), and MRS_ERR_ARG for the dtype, stride < 3, a NULL pointer, a pointer that is not device memory of
 * the swarm's device or too small for its rows, and a sharded swarm.  count == 0 is MRS_OK. */
int mrs_swarm_apply_force_device(mrs_swarm_t* s, int32_t first, int32_t count, const void* dev_force, int32_t dtype, int32_t stride, void* ext_stream);
/* mrs_swarm_rollout_rate_device under a force schedule.  Equals, bit for bit in LITERAL arithmetic, the loop
 *   for t in [0, n_steps):
 *     if (t % cmd_every == 0)
 *       mrs_swarm_set_input_device(s, first, count, mode, row block t / cmd_every of dev_cmd, dtype, cmd_stride, ext_stream);
 *     if (t % force_every == 0)
 *       mrs_swarm_apply_force_device(s, first, count, row block t / force_every of dev_force, dtype, force_stride, ext_stream);
 *     mrs_swarm_step_n(s, dt, 1, 1);
 *     if (groups && (t + 1) % obs_every == 0)
 *       mrs_swarm_gather_device(s, first, count, groups, row block (t + 1) / obs_every - 1 of dev_obs, dtype, obs_stride, ext_stream);
 * dev_force holds n_steps / force_every row blocks of `count` rows; row (j, k) starts at element ((size_t)j * count + k) * force_stride.
 * One dtype serves commands, forces and observations.  force_every must be >= 1 and divide n_steps (force_every == n_steps: one force for
 * the whole call); the three rates are independent, and inside a force block nothing is read from dev_force.  UAVs outside the range keep
 * their own commands, modes and forces.  A UAV on hold is not stepped; its command and force columns are written with the last row
 * blocks that start in the call.  Crashed UAVs take their force rows and the force acts on them as in the reference.  Afterwards the
 * force columns of the range hold the LAST force block (mrs_swarm_get_external_force returns it).  A pending collision tick is evaluated
 * first; force block 0 then replaces that tick's force for the range, as the loop's first mrs_swarm_apply_force_device would.
 * Everything else is the contract of mrs_swarm_rollout_rate_device, and so are the refusals, plus, as MRS_ERR_ARG: force_every < 1 or not
 * dividing n_steps, force_stride < 3, and a dev_force that is NULL, not device memory or one row short of its n_steps / force_every
 * blocks (exactly that many are accepted). */
int mrs_swarm_rollout_force_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_steps, int32_t cmd_every,
                                   int32_t obs_every, int32_t force_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride,
                                   const void* dev_force, int32_t force_stride, uint32_t groups, void* dev_obs, int32_t obs_stride, void* ext_stream);

/* ---- cost rollouts: a per-UAV quadratic cost summed inside the rollout (the number a sampling-based planner wants per sample) ----
 * mrs_swarm_rollout_rate_device that, where it would write an observation row, compares the row with a target row and adds the weighted
 * squared distance to one FP64 number per UAV.  Stands for the loop
 *   for t in [0, n_steps):
 *     if (t % cmd_every == 0)
 *       mrs_swarm_set_input_device(s, first, count, mode, row block t / cmd_every of dev_cmd, dtype, cmd_stride, ext_stream);
 *     mrs_swarm_step_n(s, dt, 1, 1);
 *     if ((t + 1) % cost_every == 0)
 *       rows[(t + 1) / cost_every - 1] = mrs_swarm_gather_device(s, first, count, groups, ..., MRS_DTYPE_F64, ...);
 * followed, with E = n_steps / cost_every evaluations and w = the gather width of `groups`, by
 *   c = accumulate ? dev_cost[k] : +0.0
 *   for j in [0, E):
 *     term = +0.0
 *     for col in [0, w):                         (ascending, no column skipped)
 *       d    = rows[j][k][col] - target[j][k or 0][col]
 *       term = term + (weight[j or 0][col] * d) * d
 *     c = c + term
 *   dev_cost[k] = c
 * for every UAV first + k of the range.  All of it is FP64, one rounding per operation and no fused multiply-add, in both arithmetic
 * flavours; targets and weights have the commands' dtype (FP32 is widened exactly); dev_cost is always FP64; the residual is taken on
 * the FP64 values of the row, not on a row rounded to FP32.  Nothing is special-cased: a non-finite target, a zero weight against a
 * non-finite residual and a negative weight give what the lines above give, and the zeros of the MRS_OBS_RPM group past n_motors take
 * part like any other column.
 * Target row (j, k) starts at element ((size_t)j * count + k) * target_stride of dev_target; target_stride == 0: all UAVs share ONE row
 * per evaluation and row j starts at element j * w (a dense [E, w] array).  Weight row j starts at element j * weight_stride of
 * dev_weight; weight_stride == 0: one row of w elements serves every evaluation.  cost_every == n_steps is a terminal cost,
 * cost_every == 1 a running cost; a heavier last weight row gives both.  Inside an evaluation block nothing is read from dev_target or
 * dev_weight and dev_cost is not touched; no observation row is written at all.
 * A UAV on hold is not stepped and adds one term of its unchanged state per evaluation; crashed UAVs are evaluated like any other;
 * UAVs outside the range are stepped and own no element of dev_cost.  The result does not depend on how the call is cut into launches,
 * and two calls over the halves of a horizon, the second with accumulate != 0, give the bits of one call over the whole.  Commands, the
 * mode, the final state and everything else are the contract of mrs_swarm_rollout_rate_device (ONE stream fence per call; the call
 * enters like a state call; refused on a sharded swarm), and so are its refusals, plus, as MRS_ERR_ARG with nothing changed:
 * groups == 0, a NULL dev_target, dev_weight or dev_cost, cost_every < 1 or not dividing n_steps, a target_stride or weight_stride that
 * is neither 0 nor at least w, and pointers that are not device memory of the swarm's device or too small for their rows (dev_cost:
 * count doubles). */
int mrs_swarm_rollout_cost_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_steps, int32_t cmd_every,
                                  int32_t cost_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride, uint32_t groups,
                                  const void* dev_target, int32_t target_stride, /* 0: one shared row per evaluation ([E, w]) */
                                  const void* dev_weight, int32_t weight_stride, /* 0: one weight row for every evaluation */
                                  double* dev_cost, int32_t accumulate, void* ext_stream);

/* ---- feedback rollouts: closed-loop linear state feedback inside the rollout (the samples are controllers, not command sequences) ----
 * mrs_swarm_rollout_cost_device whose command rows are NOMINAL commands: the command written at the start of a command block is
 * cmd_row + G (ref_row - obs_row), formed in the step kernel from the state it holds.  W_o = the gather width of fb_groups (at least
 * one group), W_c = the command width of `mode` as the rollouts define it (MRS_ACTUATOR_CMD: the motors of the row, i.e. cmd_stride,
 * at most MRS_MAX_MOTORS); B = n_steps / cmd_every command blocks.  At the top of step t, when t % cmd_every == 0, with b = t / cmd_every,
 * for UAV first + k:
 *   o[0 .. W_o) = the FP64 observation row of fb_groups that mrs_swarm_gather_device(MRS_DTYPE_F64) would return at this moment (the
 *                 state BEFORE the step)
 *   for j ascending:  e[j] = ref[b][k][j] - o[j]
 *   for each c < W_c: acc = cmd[b][k][c];  for j ascending: acc = acc + (G[b][k][c][j] * e[j]);  u[c] = acc
 *   u -> the command columns, as mrs_swarm_set_input_device(mode, u) stores a row
 * Every operation is FP64 with one rounding and no fused multiply-add, in both arithmetic flavours; FP32 inputs are widened exactly.
 * No column is skipped and nothing is special-cased: a zero gain times a non-finite residual is what IEEE makes of it, and the zeros
 * of the MRS_OBS_RPM group past n_motors take part.  A NaN setpoint or observation is its residual with its own sign and payload (the
 * setpoint's if both are NaN), as a host subtraction propagates it, so that the loop run with host arithmetic writes the same command
 * bits for a UAV whose state is NaN.  Inside a command block the command stays as written: the feedback is sampled at
 * the command rate, like a real control loop.  The call stands for the loop
 *   mrs_swarm_gather_device(fb_groups, MRS_DTYPE_F64) -> the lines above -> mrs_swarm_set_input_device(mode, u) -> cmd_every steps
 * with the evaluations of mrs_swarm_rollout_cost_device (cost_every, cost_groups, dev_target, dev_weight, dev_cost, accumulate) beside
 * it, and gives that loop's bits.  cost_groups == 0 with dev_target, dev_weight and dev_cost NULL is a pure closed-loop run whose
 * result is the swarm's state.  A UAV on hold is not stepped; its command is still formed (from its unchanged state) and written and
 * its cost evaluated; crashed UAVs get what the loop gives them.  The feedback has no memory: a horizon cut into two calls, the second
 * with accumulate != 0, gives the bits of one call.
 * Layouts (one dtype serves commands, gains, setpoints, targets and weights; dev_cost is FP64):
 *   dev_cmd, dev_target, dev_weight   as mrs_swarm_rollout_cost_device
 *   dev_ref      setpoint rows, as the cost targets: row (b, k) at element ((size_t)b * count + k) * ref_stride; ref_stride == 0: all
 *                UAVs share ONE dense row of W_o elements per block ([ref_blocks, W_o])
 *   dev_gain     gain_per_uav == 0: dense row-major [gain_blocks, W_c, W_o], one matrix for all UAVs;
 *                gain_per_uav == 1: dense [gain_blocks, W_c, W_o, count], UAV-MINOR: G[b][k][c][j] at element
 *                ((b * W_c + c) * W_o + j) * count + k.  A UAV's gain is W_c * W_o elements (4 x 18 doubles: 576 B, more than the 492 B
 *                a step moves); with one matrix per UAV contiguous every load of a 64-lane wave would touch 64 cache lines, UAV-minor
 *                makes each of the W_c * W_o loads one coalesced 512-B request
 *   gain_blocks, ref_blocks   B (a block per command block) or 1 (one block serves the whole call)
 * Everything else (the step, the mode, the stream fence, launch cutting, refusal on a sharded swarm, the argument checks before any
 * launch) is the contract of mrs_swarm_rollout_cost_device, and so are its refusals, plus, as MRS_ERR_ARG with nothing changed: a mode
 * without a payload, fb_groups without a group or with unknown bits, a NULL dev_gain or dev_ref, gain_per_uav other than 0 or 1,
 * gain_blocks or ref_blocks that are neither 1 nor B, a ref_stride that is neither 0 nor at least W_o, cost_groups == 0 with a cost
 * pointer, and pointers that are not device memory of the swarm's device or too small for their rows. */
int mrs_swarm_rollout_feedback_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_steps, int32_t cmd_every,
                                      int32_t cost_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride, uint32_t fb_groups,
                                      const void* dev_gain, int32_t gain_per_uav, /* 0: [Bg, W_c, W_o] | 1: [Bg, W_c, W_o, count] */
                                      int32_t gain_blocks,                        /* 1 or B */
                                      const void* dev_ref, int32_t ref_stride,    /* 0: one shared row per block ([Bg, W_o]) */
                                      int32_t ref_blocks,                         /* 1 or B */
                                      uint32_t cost_groups, const void* dev_target, int32_t target_stride, const void* dev_weight,
                                      int32_t weight_stride, double* dev_cost, int32_t accumulate, void* ext_stream);

/* ---- tick rollouts: timerMain over n_ticks ticks in one call — makeStep of every UAV, then handleCollisions — with device rows ----
 * MultirotorSimulator::timerMain (src/multirotor_simulator.cpp:211-217) is makeStep for every UAV, then handleCollisions (:295-359).  A
 * swarm policy or a multi-agent planner needs the contacts, the rebounce forces and the crash flags inside its horizon.  Equals, bit for
 * bit in LITERAL arithmetic, the loop
 *   for t in [0, n_ticks):
 *     if (t % cmd_every == 0)
 *       mrs_swarm_set_input_device(s, first, count, mode, row block t / cmd_every of dev_cmd, dtype, cmd_stride, ext_stream);
 *     mrs_swarm_step(s, dt);             evaluates the collision tick pending from tick t - 1 (fused with the step when the lists allow it)
 *     if ((t + 1) % obs_every == 0) {    row block j = (t + 1) / obs_every - 1
 *       if (groups) mrs_swarm_gather_device(s, first, count, groups, row block j of dev_obs, dtype, obs_stride, ext_stream);
 *       if (dev_crashed) mrs_swarm_get_crashed_device(s, first, count, dev_crashed + j * count, ext_stream);
 *     }
 *     mrs_swarm_handle_collisions(s, 1, crash, rebounce);    stays pending: the next step, of this call or a later one, evaluates it
 * dev_cmd and dev_obs are the row blocks of mrs_swarm_rollout_rate_device.  dev_crashed (may be NULL) holds n_ticks / obs_every dense
 * blocks of `count` bytes: block j is UavSystem::hasCrashed of the range at the instant observation block j is taken — after makeStep of
 * the tick and before that tick's handleCollisions, where the reference's publishers see the swarm — so it holds every collision up to
 * the previous tick.  groups and dev_crashed are independent: either may be 0 / NULL.  handleCollisions is always enabled here (there is
 * no argument that switches it off: without collisions mrs_swarm_rollout_rate_device is the call); crash != 0 is the crash mode, else the
 * elastic one with `rebounce`.
 * The call enters like a state call, except that a collision tick pending at entry is evaluated by the first launch of the call; the
 * last tick's collision stays pending as after mrs_swarm_tick_n.  The call waits for its own launches before it returns (a replay after
 * stale neighbour lists writes into the caller's rows, which need only live until the call returns): ONE host wait per call, where the
 * loop above has one or more per tick.  ONE stream fence per call.  A UAV on hold takes part in the collisions and is not iterated; it
 * gets its command rows, and observation and crash rows of its unchanged state (its crash flag included, if the evaluation set it).
 * Crashed UAVs and UAVs outside the range are treated as in mrs_swarm_rollout_rate_device.  Every argument is checked before anything is
 * launched and a refused call changes nothing: the refusals of mrs_swarm_rollout_rate_device (a sharded swarm among them), plus, as
 * MRS_ERR_ARG, a dev_crashed that is not device memory of the swarm's device or shorter than n_ticks / obs_every * count bytes, and a
 * rebounce that is not finite. */
int mrs_swarm_rollout_tick_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_ticks, int32_t cmd_every,
                                  int32_t obs_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride, uint32_t groups, void* dev_obs,
                                  int32_t obs_stride, uint8_t* dev_crashed, int32_t crash, double rebounce, void* ext_stream);

/* ---- cost tick rollouts: a per-UAV cost with a crash penalty, summed inside a tick rollout ----
 * mrs_swarm_rollout_tick_device that returns one FP64 number per UAV instead of row blocks: the horizon cost of a swarm policy or a
 * multi-agent planner with the contacts of timerMain in it (src/multirotor_simulator.cpp:211-217, handleCollisions :295-359), and with the
 * crash flag, the one thing a collision-aware horizon produces that the state rows do not show, as a cost.  Stands for the loop of
 * mrs_swarm_rollout_tick_device with obs_every = cost_every, FP64 rows of `groups` (MRS_DTYPE_F64) and crash rows,
 *   for t in [0, n_ticks):
 *     if (t % cmd_every == 0)
 *       mrs_swarm_set_input_device(s, first, count, mode, row block t / cmd_every of dev_cmd, dtype, cmd_stride, ext_stream);
 *     mrs_swarm_step(s, dt);              evaluates the collision tick pending from tick t - 1
 *     if ((t + 1) % cost_every == 0) {    j = (t + 1) / cost_every - 1
 *       if (groups) rows[j] = mrs_swarm_gather_device(s, first, count, groups, ..., MRS_DTYPE_F64, ...);
 *       crashed[j] = mrs_swarm_get_crashed_device(s, first, count, ...);
 *     }
 *     mrs_swarm_handle_collisions(s, 1, crash, rebounce);    stays pending
 * followed, with E = n_ticks / cost_every evaluations and w = the gather width of `groups`, for every UAV first + k by
 *   c = accumulate ? dev_cost[k] : +0.0
 *   for j in [0, E):
 *     if (groups) {
 *       term = +0.0
 *       for col in [0, w):                         (ascending, no column skipped)
 *         d    = rows[j][k][col] - target[j][k or 0][col]
 *         term = term + (weight[j or 0][col] * d) * d
 *       c = c + term
 *     }
 *     if (crashed[j][k]) c = c + crash_cost
 *   dev_cost[k] = c
 * All of it is FP64, one rounding per operation and no fused multiply-add, in both arithmetic flavours; targets and weights have the
 * commands' dtype (FP32 is widened exactly); nothing is special-cased.  The term and the crash cost are two separately rounded
 * additions, in that order, and the crash add is performed whenever the byte is set, whatever crash_cost is (0, negative, non-finite).
 * crashed[j][k] is UavSystem::hasCrashed where the tick rollout takes its crash rows: after the tick's makeStep, before that tick's
 * handleCollisions.  It is a level, not an edge: a UAV that crashed early pays at every later evaluation; a crash caused by the last
 * tick's collision pass stays pending with that pass, is not charged by this call, and is charged by the next horizon (accumulate != 0
 * chains the two).  Target and weight layouts, target_stride == 0 and weight_stride == 0 are those of mrs_swarm_rollout_cost_device.
 * groups == 0 with dev_target and dev_weight NULL is the crash cost alone.  No observation row and no crash byte is written.
 * Everything else is the contract of mrs_swarm_rollout_tick_device: the entry (a collision tick pending at entry is evaluated by the
 * first launch), the last tick's collision staying pending, ONE host wait and ONE stream fence per call, UAVs on hold (they take part in
 * the collisions, are not iterated, get their command rows, and add one term of their unchanged state per evaluation plus the crash cost
 * if their flag is set), crashed UAVs, UAVs outside the range (they own no element of dev_cost), and the refusal on a sharded swarm.
 * Every argument is checked before anything is launched and a refused call changes nothing: the refusals of
 * mrs_swarm_rollout_tick_device and of mrs_swarm_rollout_cost_device, except that groups == 0 is refused only when a dev_target or
 * dev_weight comes with it; groups != 0 with a NULL dev_target or dev_weight, a dev_cost that is NULL or shorter than count doubles,
 * cost_every < 1 or not dividing n_ticks, and a rebounce that is not finite are refused. */
int mrs_swarm_rollout_tick_cost_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_ticks,
                                       int32_t cmd_every, int32_t cost_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride,
                                       uint32_t groups, const void* dev_target, int32_t target_stride, const void* dev_weight,
                                       int32_t weight_stride, double crash_cost, double* dev_cost, int32_t accumulate, int32_t crash,
                                       double rebounce, void* ext_stream);

/* ---- feedback tick rollouts: closed-loop linear state feedback inside a tick rollout (controllers as samples, contacts in the horizon) ----
 * mrs_swarm_rollout_tick_cost_device whose command rows are NOMINAL commands, as mrs_swarm_rollout_feedback_device's are: linear-policy
 * search for a swarm, tube-MPPI around a nominal plan in a crowded airspace, one law over many initial states with crash penalties — with
 * the contacts of timerMain in the horizon (src/multirotor_simulator.cpp:211-217, handleCollisions :295-359).  With B = n_ticks / cmd_every
 * command blocks, W_o the gather width of fb_groups and W_c the command width of `mode`, the call stands for the loop
 *   for t in [0, n_ticks):
 *     if (t % cmd_every == 0) {           b = t / cmd_every
 *       o = mrs_swarm_gather_device(s, first, count, fb_groups, ..., MRS_DTYPE_F64, ...);    the state BEFORE the step; a collision tick
 *                                                                                            pending from tick t - 1 stays pending
 *       for every UAV first + k: u[k] = the law of mrs_swarm_rollout_feedback_device on
 *                                       (cmd[b][k], G[gain_blocks == 1 ? 0 : b][k or shared], ref[ref_blocks == 1 ? 0 : b][k or shared], o[k])
 *       mrs_swarm_set_input_device(s, first, count, mode, u, MRS_DTYPE_F64, W_c, ext_stream);
 *     }
 *     mrs_swarm_step(s, dt);              evaluates the collision tick pending from tick t - 1
 *     if ((t + 1) % cost_every == 0 && dev_cost)
 *       the evaluation of mrs_swarm_rollout_tick_cost_device: the term of cost_groups if cost_groups != 0, then the crash add
 *     mrs_swarm_handle_collisions(s, 1, crash, rebounce);    stays pending
 * The law is the feedback rollout's, word for word: FP64 with one rounding per operation and no fused multiply-add in both arithmetic
 * flavours, columns ascending and none skipped, FP32 inputs widened exactly, a NaN setpoint or observation being its residual with its
 * own bits (the setpoint's if both are NaN), and the layouts of dev_gain (gain_per_uav == 0: [gain_blocks, W_c, W_o]; 1: [gain_blocks,
 * W_c, W_o, count], UAV-minor) and dev_ref (ref_stride == 0: one shared dense row per block).  The row the law reads does not depend on
 * whether the pending collision tick has been evaluated: the evaluation writes the external force and the crash flag, and no observation
 * group reads either.  The evaluation is the cost tick rollout's, word for word: two separately rounded additions, the term first, the
 * crash add performed whenever the flag is set whatever crash_cost is, the flag a level and not an edge, cost_groups == 0 with dev_target
 * and dev_weight NULL the crash cost alone.  dev_cost == NULL with cost_groups == 0 and dev_target and dev_weight NULL is a pure
 * closed-loop run with no evaluation at all, whose result is the swarm's state: cost_every is still checked, crash_cost is ignored.
 * Everything else is the contract of mrs_swarm_rollout_tick_device: the entry (a collision tick pending at entry is evaluated by the
 * first launch), the last tick's collision staying pending, ONE host wait and ONE stream fence per call, crashed UAVs, UAVs outside the
 * range (stepped with their own commands, no element of dev_cost), and the refusal on a sharded swarm.  A UAV on hold is not iterated
 * and takes part in the collisions; its command is still formed (from its unchanged state) and written, and its cost evaluated.  The
 * feedback has no memory: a horizon cut into two calls, the second with accumulate != 0, gives the bits of one call.
 * Every argument is checked before anything is launched and a refused call changes nothing: the refusals of
 * mrs_swarm_rollout_feedback_device and of mrs_swarm_rollout_tick_cost_device together, except that cost_groups == 0 is refused only when
 * a dev_target or dev_weight comes with it, and cost_groups != 0 needs all of dev_target, dev_weight and dev_cost. */
int mrs_swarm_rollout_tick_feedback_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_ticks,
                                           int32_t cmd_every, int32_t cost_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride,
                                           uint32_t fb_groups, const void* dev_gain, int32_t gain_per_uav, int32_t gain_blocks,
                                           const void* dev_ref, int32_t ref_stride, int32_t ref_blocks, uint32_t cost_groups,
                                           const void* dev_target, int32_t target_stride, const void* dev_weight, int32_t weight_stride,
                                           double crash_cost, double* dev_cost, int32_t accumulate, int32_t crash, double rebounce,
                                           void* ext_stream);

#ifdef __cplusplus
}
#endif
#endif /* MRS_SWARM_H */
