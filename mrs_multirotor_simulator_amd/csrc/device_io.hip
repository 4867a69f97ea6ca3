// device_io.hip — per-UAV I/O between the SoA state and caller-owned DEVICE rows, for callers whose controller, policy or reward
// lives on the same GPU (a torch module): commands in, observations out, masked resets, crash flags, with no host copy on the way.
// One lane per UAV; the state side is the coalesced field-major columns of swarm_layout.h, the caller side one row of `stride`
// elements per UAV (FP64 or FP32).  The host entry points at the end validate every argument before anything is launched and fence
// the caller's stream against the swarm's (include/mrs_swarm.h, "device-resident callers").
#include "host_internal.h"
#include "obs_row.h"

namespace {

// Eigen::AngleAxisd(angle, UnitZ).toRotationMatrix() (Eigen/src/Geometry/AngleAxis.h), row-major out: the host's angle_axis_z
// (host_api.hip) with the device's sin / cos
__device__ __forceinline__ void angle_axis_z_dev(double angle, double R[9]) {
  const double ax[3] = {0, 0, 1};
  const double s = sin(angle), c = cos(angle);
  const double sa[3] = {s * ax[0], s * ax[1], s * ax[2]};
  const double ca[3] = {(1.0 - c) * ax[0], (1.0 - c) * ax[1], (1.0 - c) * ax[2]};
  double       tmp;
  tmp  = ca[0] * ax[1];
  R[1] = tmp - sa[2];
  R[3] = tmp + sa[2];
  tmp  = ca[0] * ax[2];
  R[2] = tmp + sa[1];
  R[6] = tmp - sa[1];
  tmp  = ca[1] * ax[2];
  R[5] = tmp - sa[0];
  R[7] = tmp + sa[0];
  R[0] = ca[0] * ax[0] + c;
  R[4] = ca[1] * ax[1] + c;
  R[8] = ca[2] * ax[2] + c;
}

// what an observation row reads of UAV i: its state columns
struct ColumnObs {
  const SwarmDev& sw;
  size_t          np;
  int             i;
  __device__ double col(int f) const { return sw.S[(size_t)f * np + i]; }
  __device__ double x(int c) const { return col(F_X + c); }
  __device__ double v(int c) const { return col(F_V + c); }
  __device__ double R(int c) const { return col(F_R + c); }
  __device__ double omega(int c) const { return col(F_W + c); }
  __device__ double imu(int c) const { return col(F_IMU + c); }
  __device__ double rpm(int m) const { return col(F_RPM + m); }
  __device__ int    n_motors() const { return sw.T[sw.F[i] >> FLAG_TYPE_SHIFT].n_motors; }
};

// observation groups of UAVs [first, first + count) into rows of `stride` elements (obs_row.h).  Direct per-lane stores, as
// k_pack_poses (LDS staging measured no better there).
template <typename T>
__global__ void __launch_bounds__(256) k_gather_rows(SwarmDev sw, int first, int count, uint32_t groups, T* rows, int stride) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const ColumnObs src{sw, (size_t)sw.npad, first + k};
  mrs_obs_row(src, groups, rows + (size_t)k * (size_t)stride);
}

// setInput payload rows (FP64 or FP32, device-resident) into the command columns F_CMD + j, and the mode bits of the flag word: what
// mrs_swarm_set_input's column uploads + flag update do, in one launch (k_unpack_rows with another source)
template <typename T>
__global__ void __launch_bounds__(256) k_scatter_cmd(SwarmDev sw, const T* rows, int stride, int width, int first, int count, uint32_t mode_bits) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const int    i  = first + k;
  const size_t np = (size_t)sw.npad;
  const T*     r  = rows + (size_t)k * (size_t)stride;
  for (int j = 0; j < width; j++) sw.S[(size_t)(F_CMD + j) * np + i] = (double)r[j];
  sw.F[i] = (sw.F[i] & ~FLAG_MODE_MASK) | mode_bits;
}

// applyForce rows (FP64 or FP32, device-resident, world frame, N) into the external-force columns: what mrs_swarm_apply_force's three
// column uploads do, in one launch
template <typename T>
__global__ void __launch_bounds__(256) k_scatter_force(SwarmDev sw, const T* rows, int stride, int first, int count) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const int    i  = first + k;
  const size_t np = (size_t)sw.npad;
  const T*     r  = rows + (size_t)k * (size_t)stride;
  const double f[3] = {(double)r[0], (double)r[1], (double)r[2]};
#pragma unroll
  for (int c = 0; c < 3; c++) sw.S[(size_t)(F_FEXT + c) * np + i] = f[c];
}

// mrs_swarm_construct(params of the UAV's own type, pos, heading) for the UAVs whose mask byte is set, without the host: state,
// IMU, external force and PID columns zero, R = AngleAxis(-heading, z), x = pos, _initial_pos_ z = pos z; crashed and v_prev-split
// cleared, takeoff patch as given.  Commands, feed-forwards, the mode / feed-forward / type bits and the hold flag are kept.
template <typename T>
__global__ void __launch_bounds__(256) k_reset_masked(SwarmDev sw, int first, int count, const uint8_t* mask, const T* pos, const T* heading,
                                                      uint32_t takeoff) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count || !mask[k]) return;
  const int    i  = first + k;
  const size_t np = (size_t)sw.npad;
#define ST(f) sw.S[(size_t)(f) * np + i]
  double x[3], R[9];
#pragma unroll
  for (int c = 0; c < 3; c++) x[c] = (double)pos[(size_t)k * 3 + c];
  angle_axis_z_dev(-(heading ? (double)heading[k] : 0.0), R);
#pragma unroll
  for (int c = 0; c < 3; c++) ST(F_X + c) = x[c];
#pragma unroll
  for (int f = F_V; f < F_R; f++) ST(f) = 0.0;  // v, v_prev
#pragma unroll
  for (int c = 0; c < 9; c++) ST(F_R + c) = R[c];
#pragma unroll
  for (int f = F_W; f < F_INITZ; f++) ST(f) = 0.0;  // omega, motor rpm, IMU, external force
  ST(F_INITZ) = x[2];
#pragma unroll
  for (int f = F_PID; f < F_CMD; f++) ST(f) = 0.0;
#undef ST
  sw.F[i] = (sw.F[i] & ~(FLAG_CRASHED | FLAG_VPREV_SPLIT | FLAG_TAKEOFF)) | takeoff;
}

// UavSystem::hasCrashed of UAVs [first, first + count) as bytes
__global__ void __launch_bounds__(256) k_crashed_u8(const uint32_t* F, int first, int count, uint8_t* out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  out[k] = (F[first + k] & FLAG_CRASHED) ? 1 : 0;
}

// the crash add of a cost tick or feedback tick rollout's evaluation (mrs_swarm_rollout_tick_cost_device,
// mrs_swarm_rollout_tick_feedback_device) for a tick without the fused form: one FP64 addition per crashed UAV of the range, behind the
// term the cost or feedback rollout kernels added, performed whatever crash_cost is
__global__ void __launch_bounds__(256) k_crash_cost(const uint32_t* F, int first, int count, double* cost, double crash_cost) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  if (F[first + k] & FLAG_CRASHED) cost[k] = cost[k] + crash_cost;
}

inline dim3 grid_of(int count) { return dim3((unsigned)((count + 255) / 256)); }

// payload elements of a command row of `mode`: the widths of mrs_swarm_set_input (ACTUATOR: the row's stride, at most MRS_MAX_MOTORS)
int command_width(int mode, int stride) {
  switch (mode) {
    case MRS_INPUT_UNKNOWN: return 0;
    case MRS_ACTUATOR_CMD: return stride < MRS_MAX_MOTORS ? stride : MRS_MAX_MOTORS;
    case MRS_ATTITUDE_CMD: return 10;
    case MRS_TILT_HDG_RATE_CMD: return 5;
    default: return 4;
  }
}

// an ACTUATOR payload of `width` motors must cover every motor of UAVs [first, first + count)
bool actuator_width_ok(const mrs_swarm* s, int first, int count, int width) {
  if (width >= MRS_MAX_MOTORS) return true;
  for (int k = 0; k < count; k++)
    if (s->keys[s->uav_type[(size_t)first + k]].mp.n_motors > width) return false;
  return true;
}

}  // namespace

// ---- host side (shared with nearest.hip through host_internal.h) ----
namespace mrs_host {

size_t dtype_bytes(int dtype) { return dtype == MRS_DTYPE_F32 ? sizeof(float) : sizeof(double); }

int check_dtype(int dtype) {
  if (dtype != MRS_DTYPE_F64 && dtype != MRS_DTYPE_F32) return fail(MRS_ERR_ARG, "dtype must be MRS_DTYPE_F64 or MRS_DTYPE_F32");
  return MRS_OK;
}

// `p` must be device memory of the swarm's device holding at least `bytes` bytes from p on (the end is checked against the allocation
// that holds p where the runtime can tell)
int check_device_ptr(const mrs_swarm* s, const void* p, size_t bytes, const char* what) {
  if (!p) return fail(MRS_ERR_ARG, std::string(what) + ": null pointer");
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof a);
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // (not sticky: a later launch must not report it)
    return fail(MRS_ERR_ARG, std::string(what) + ": not a pointer the HIP runtime knows (host memory?)");
  }
  if (a.type != hipMemoryTypeDevice) return fail(MRS_ERR_ARG, std::string(what) + ": not device memory");
  if (a.device != s->device)
    return fail(MRS_ERR_ARG, std::string(what) + ": memory of device " + std::to_string(a.device) + ", the swarm lives on device " + std::to_string(s->device));
  hipDeviceptr_t base = nullptr;
  size_t         size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) == hipSuccess) {
    if ((const char*)p + bytes > (const char*)base + size) return fail(MRS_ERR_ARG, std::string(what) + ": the rows extend past the end of their allocation");
  } else {
    (void)hipGetLastError();
  }
  return MRS_OK;
}

// bytes spanned by `count` rows of `stride` elements of which the first `width` are used
size_t rows_bytes(int count, int stride, int width, int dtype) {
  return ((size_t)(count - 1) * (size_t)stride + (size_t)width) * dtype_bytes(dtype);
}
// ... and by such rows of int32 indices or counts (one per row: stride = width = 1)
size_t index_rows_bytes(int count, int stride, int width) { return ((size_t)(count - 1) * (size_t)stride + (size_t)width) * sizeof(int32_t); }

// the stream fence of every call: the swarm's stream waits for what the caller queued on `ext` so far ...
int fence_in(mrs_swarm* s, hipStream_t ext) {
  if (ext == s->stream) return MRS_OK;
  HIPCHK(s->ev_dio_in.create(hipEventDisableTiming));
  HIPCHK(s->ev_dio_out.create(hipEventDisableTiming));
  HIPCHK(hipEventRecord(s->ev_dio_in, ext));
  HIPCHK(hipStreamWaitEvent(s->stream, s->ev_dio_in, 0));
  return MRS_OK;
}
// ... and `ext` waits for the kernel of the call
int fence_out(mrs_swarm* s, hipStream_t ext) {
  if (ext == s->stream) return MRS_OK;
  HIPCHK(hipEventRecord(s->ev_dio_out, s->stream));
  HIPCHK(hipStreamWaitEvent(ext, s->ev_dio_out, 0));
  return MRS_OK;
}

int launch_crashed_u8(mrs_swarm* s, int first, int count, uint8_t* dev_out) {
  hipLaunchKernelGGL(k_crashed_u8, grid_of(count), dim3(256), 0, s->stream, s->dF, first, count, dev_out);
  HIPCHK(hipGetLastError());
  return MRS_OK;
}

int launch_crash_cost(mrs_swarm* s, int first, int count, double* dev_cost, double crash_cost) {
  hipLaunchKernelGGL(k_crash_cost, grid_of(count), dim3(256), 0, s->stream, s->dF, first, count, dev_cost, crash_cost);
  HIPCHK(hipGetLastError());
  return MRS_OK;
}

}  // namespace mrs_host

extern "C" {

int mrs_swarm_device(const mrs_swarm_t* s, int32_t* device_id) {
  MRS_LOCK(s);
  if (!s || !device_id) return fail(MRS_ERR_ARG, "null argument");
  *device_id = s->device;
  return MRS_OK;
}

int mrs_swarm_gather_width(uint32_t groups, int32_t* width) {
  if (!width) return fail(MRS_ERR_ARG, "null width");
  if (groups & ~(uint32_t)MRS_OBS_ALL) return fail(MRS_ERR_ARG, "unknown observation group bits");
  int w = 0;
  for (int b = 0; b < 8; b++)
    if (groups & (1u << b)) w += kObsWidth[b];
  *width = w;
  return MRS_OK;
}

int mrs_swarm_set_input_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, const void* dev_rows, int32_t dtype, int32_t stride,
                               void* ext_stream) {
  MRS_ENTER_COMMANDS(s);
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (mode < MRS_INPUT_UNKNOWN || mode > MRS_POSITION_CMD) return fail(MRS_ERR_ARG, "bad input mode");
  if ((rc = check_dtype(dtype))) return rc;
  if (count == 0) return MRS_OK;
  const int width = command_width(mode, stride);  // the payload widths of mrs_swarm_set_input
  if (width > 0) {
    if (stride < width || width < 1) return fail(MRS_ERR_ARG, "stride too small for this mode");
    if ((rc = check_device_ptr(s, dev_rows, rows_bytes(count, stride, width, dtype), "dev_rows"))) return rc;
  }
  if (mode == MRS_ACTUATOR_CMD && !actuator_width_ok(s, first, count, width)) return fail(MRS_ERR_ARG, "actuator payload narrower than n_motors");
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  if ((rc = fence_in(s, ext))) return rc;
  const uint32_t mode_bits = (uint32_t)mode << FLAG_MODE_SHIFT;
  if (dtype == MRS_DTYPE_F32)
    hipLaunchKernelGGL(k_scatter_cmd<float>, grid_of(count), dim3(256), 0, s->stream, s->view(), static_cast<const float*>(dev_rows), stride, width,
                       first, count, mode_bits);
  else
    hipLaunchKernelGGL(k_scatter_cmd<double>, grid_of(count), dim3(256), 0, s->stream, s->view(), static_cast<const double*>(dev_rows), stride,
                       width, first, count, mode_bits);
  HIPCHK(hipGetLastError());
  if ((rc = fence_out(s, ext))) return rc;
  // host mirror of the modes (kernel variant): a loop that keeps its mode finds nothing to change
  const uint8_t* m    = s->uav_mode.data() + first;
  unsigned       diff = 0;
  for (int k = 0; k < count; k++) diff |= (unsigned)(m[k] ^ (uint8_t)mode);
  if (diff) track_mode(s, first, count, mode);
  return MRS_OK;
}

int mrs_swarm_gather_device(mrs_swarm_t* s, int32_t first, int32_t count, uint32_t groups, void* dev_rows, int32_t dtype, int32_t stride,
                            void* ext_stream) {
  MRS_ENTER_COMMANDS(s);
  int rc = check_range(s, first, count);
  if (rc) return rc;
  int32_t width = 0;
  if ((rc = mrs_swarm_gather_width(groups, &width))) return rc;
  if (width == 0) return fail(MRS_ERR_ARG, "no observation group selected");
  if ((rc = check_dtype(dtype))) return rc;
  if (stride < width) return fail(MRS_ERR_ARG, "stride smaller than the width of the selected groups");
  if (count == 0) return MRS_OK;
  if ((rc = check_device_ptr(s, dev_rows, rows_bytes(count, stride, width, dtype), "dev_rows"))) return rc;
  HIPCHK(hipSetDevice(s->device));
  if ((groups & MRS_OBS_RPM) && (rc = upload_types(s, s->table_dt > 0 ? s->table_dt : 0.001))) return rc;  // (n_motors of the type table)
  hipStream_t ext = (hipStream_t)ext_stream;
  if ((rc = fence_in(s, ext))) return rc;
  if (dtype == MRS_DTYPE_F32)
    hipLaunchKernelGGL(k_gather_rows<float>, grid_of(count), dim3(256), 0, s->stream, s->view(), first, count, groups, static_cast<float*>(dev_rows), stride);
  else
    hipLaunchKernelGGL(k_gather_rows<double>, grid_of(count), dim3(256), 0, s->stream, s->view(), first, count, groups, static_cast<double*>(dev_rows),
                       stride);
  HIPCHK(hipGetLastError());
  return fence_out(s, ext);
}

int mrs_swarm_get_crashed_device(mrs_swarm_t* s, int32_t first, int32_t count, uint8_t* dev_out, void* ext_stream) {
  MRS_ENTER(s);
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (count == 0) return MRS_OK;
  if ((rc = check_device_ptr(s, dev_out, (size_t)count, "dev_out"))) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  if ((rc = fence_in(s, ext))) return rc;
  hipLaunchKernelGGL(k_crashed_u8, grid_of(count), dim3(256), 0, s->stream, s->dF, first, count, dev_out);
  HIPCHK(hipGetLastError());
  return fence_out(s, ext);
}

int mrs_swarm_reset_device(mrs_swarm_t* s, int32_t first, int32_t count, const uint8_t* dev_mask, const void* dev_pos, const void* dev_heading,
                           int32_t dtype, int32_t takeoff_patch_enabled, void* ext_stream) {
  MRS_ENTER(s);
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, "mrs_swarm_reset_device: not on a sharded swarm");
  if ((rc = check_dtype(dtype))) return rc;
  if (count == 0) return MRS_OK;
  if ((rc = check_device_ptr(s, dev_mask, (size_t)count, "dev_mask"))) return rc;
  if ((rc = check_device_ptr(s, dev_pos, rows_bytes(count, 3, 3, dtype), "dev_pos"))) return rc;
  if (dev_heading && (rc = check_device_ptr(s, dev_heading, rows_bytes(count, 1, 1, dtype), "dev_heading"))) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  if ((rc = fence_in(s, ext))) return rc;
  const uint32_t takeoff = takeoff_patch_enabled ? FLAG_TAKEOFF : 0u;
  if (dtype == MRS_DTYPE_F32)
    hipLaunchKernelGGL(k_reset_masked<float>, grid_of(count), dim3(256), 0, s->stream, s->view(), first, count, dev_mask,
                       static_cast<const float*>(dev_pos), static_cast<const float*>(dev_heading), takeoff);
  else
    hipLaunchKernelGGL(k_reset_masked<double>, grid_of(count), dim3(256), 0, s->stream, s->view(), first, count, dev_mask,
                       static_cast<const double*>(dev_pos), static_cast<const double*>(dev_heading), takeoff);
  HIPCHK(hipGetLastError());
  s->nbr_dirty = true;  // positions changed under the neighbour lists (what put_column notes for a host write of F_X)
  return fence_out(s, ext);
}

int mrs_swarm_apply_force_device(mrs_swarm_t* s, int32_t first, int32_t count, const void* dev_force, int32_t dtype, int32_t stride, void* ext_stream) {
  MRS_ENTER(s);  // (a pending collision tick writes the same columns: it is evaluated first)
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, "mrs_swarm_apply_force_device: not on a sharded swarm");
  if ((rc = check_dtype(dtype))) return rc;
  if (stride < 3) return fail(MRS_ERR_ARG, "stride smaller than the three force components");
  if (count == 0) return MRS_OK;
  if ((rc = check_device_ptr(s, dev_force, rows_bytes(count, stride, 3, dtype), "dev_force"))) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  if ((rc = fence_in(s, ext))) return rc;
  if (dtype == MRS_DTYPE_F32)
    hipLaunchKernelGGL(k_scatter_force<float>, grid_of(count), dim3(256), 0, s->stream, s->view(), static_cast<const float*>(dev_force), stride, first,
                       count);
  else
    hipLaunchKernelGGL(k_scatter_force<double>, grid_of(count), dim3(256), 0, s->stream, s->view(), static_cast<const double*>(dev_force), stride, first,
                       count);
  HIPCHK(hipGetLastError());
  s->fext_active = true;
  return fence_out(s, ext);
}

// Every argument of the rollout entry points as one record; a call leaves what it does not have at zero.  `kind` is the entry point:
// it decides which of the optional parts are checked and which kernel family runs.
enum RolloutKind { ROLLOUT_ROWS, ROLLOUT_FORCE, ROLLOUT_COST, ROLLOUT_FEEDBACK, ROLLOUT_TICK, ROLLOUT_TICK_COST, ROLLOUT_TICK_FEEDBACK };
struct RolloutArgs {
  const char* who;
  RolloutKind kind;
  int32_t     first, count, mode;
  double      dt;
  int32_t     n_steps, cmd_every, obs_every;  // (n_ticks of a tick rollout; cost_every of a cost, feedback, cost tick or feedback tick rollout)
  const void* dev_cmd;
  int32_t     dtype, cmd_stride;
  uint32_t    groups;  // of the observation rows, or of the cost (a feedback rollout's may be 0: no cost; a cost tick rollout's: crash cost only)
  void*       dev_obs;
  int32_t     obs_stride;
  void*       ext_stream;
  // mrs_swarm_rollout_force_device
  int32_t     force_every;
  const void* dev_force;
  int32_t     force_stride;
  // mrs_swarm_rollout_cost_device, mrs_swarm_rollout_feedback_device
  const void* target;
  int32_t     target_stride;
  const void* weight;
  int32_t     weight_stride;
  double*     cost;
  int32_t     accumulate;
  // mrs_swarm_rollout_feedback_device, mrs_swarm_rollout_tick_feedback_device
  uint32_t    fb_groups;
  const void* gain;
  int32_t     gain_per_uav, gain_blocks;
  const void* ref;
  int32_t     ref_stride, ref_blocks;
  // mrs_swarm_rollout_tick_device, mrs_swarm_rollout_tick_cost_device and mrs_swarm_rollout_tick_feedback_device (which have no dev_crashed)
  uint8_t*    dev_crashed;
  int32_t     crash;
  double      rebounce;
  double      crash_cost;  // (the two costed tick rollouts)
};
// what the checks work out on their way
struct RolloutWidths {
  int     cmd;      // payload elements of a command row
  int32_t obs, fb;  // elements of a row of `groups` and of `fb_groups`
  bool    costed;   // the call evaluates a cost (a feedback rollout without cost groups is a pure closed-loop run)
};

// The argument checks of every rollout entry point, in the order in which a call with several faults reports them.  `steps` and `every`
// are the nouns of the messages: n_steps or n_ticks, obs_every or cost_every.  Nothing is launched and nothing is changed here.
static int check_rollout_args(mrs_swarm_t* s, const RolloutArgs& a, const std::string& steps, const std::string& every, RolloutWidths& w) {
  // tf: a feedback tick rollout has the feedback rollout's parts (fb) and the cost tick rollout's evaluation (tc)
  const bool tf = a.kind == ROLLOUT_TICK_FEEDBACK;
  const bool forced = a.kind == ROLLOUT_FORCE, fb = tf || a.kind == ROLLOUT_FEEDBACK, tc = tf || a.kind == ROLLOUT_TICK_COST;
  const bool cost   = fb || tc || a.kind == ROLLOUT_COST;
  int        rc     = check_range(s, a.first, a.count);
  if (rc) return rc;
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, std::string(a.who) + ": not on a sharded swarm");
  if (a.mode < MRS_INPUT_UNKNOWN || a.mode > MRS_POSITION_CMD) return fail(MRS_ERR_ARG, "bad input mode");
  if ((rc = check_dtype(a.dtype))) return rc;
  if (a.n_steps < 1) return fail(MRS_ERR_ARG, steps + " must be at least 1");
  if (a.cmd_every < 1 || a.n_steps % a.cmd_every != 0) return fail(MRS_ERR_ARG, "cmd_every must be at least 1 and divide " + steps);
  if (a.obs_every < 1 || a.n_steps % a.obs_every != 0) return fail(MRS_ERR_ARG, every + " must be at least 1 and divide " + steps);
  if (forced && (a.force_every < 1 || a.n_steps % a.force_every != 0)) return fail(MRS_ERR_ARG, "force_every must be at least 1 and divide " + steps);
  if (forced && a.force_stride < 3) return fail(MRS_ERR_ARG, "force_stride smaller than the three force components");
  if (forced && !a.dev_force) return fail(MRS_ERR_ARG, "dev_force: null pointer");
  if (!(a.dt > 0) || !std::isfinite(a.dt)) return fail(MRS_ERR_ARG, "dt must be finite and > 0");
  if (!std::isfinite(a.rebounce)) return fail(MRS_ERR_ARG, "rebounce must be finite");
  w.cmd = command_width(a.mode, a.cmd_stride);
  if (w.cmd > 0 && (a.cmd_stride < w.cmd || w.cmd < 1)) return fail(MRS_ERR_ARG, "cmd_stride too small for this mode");
  w.obs = w.fb = 0;
  if ((rc = mrs_swarm_gather_width(a.groups, &w.obs))) return rc;
  if (!cost && a.groups != 0u && a.obs_stride < w.obs) return fail(MRS_ERR_ARG, "obs_stride smaller than the width of the selected groups");
  // (no cost groups: a feedback rollout evaluates nothing; a feedback tick rollout with a dev_cost evaluates the crash cost alone)
  w.costed = cost && !(fb && a.groups == 0u && !(tf && a.cost));
  if (fb) {
    if (w.cmd < 1) return fail(MRS_ERR_ARG, "a feedback rollout needs a mode with a payload");
    if ((rc = mrs_swarm_gather_width(a.fb_groups, &w.fb))) return rc;
    if (w.fb < 1) return fail(MRS_ERR_ARG, "no feedback group selected: fb_groups must select at least one observation group");
    if (!a.gain) return fail(MRS_ERR_ARG, "dev_gain: null pointer");
    if (!a.ref) return fail(MRS_ERR_ARG, "dev_ref: null pointer");
    if (a.gain_per_uav != 0 && a.gain_per_uav != 1) return fail(MRS_ERR_ARG, "gain_per_uav must be 0 (shared gains) or 1");
    if (a.gain_blocks != 1 && a.gain_blocks != a.n_steps / a.cmd_every) return fail(MRS_ERR_ARG, "gain_blocks must be 1 or the number of command blocks");
    if (a.ref_blocks != 1 && a.ref_blocks != a.n_steps / a.cmd_every) return fail(MRS_ERR_ARG, "ref_blocks must be 1 or the number of command blocks");
    if (a.ref_stride != 0 && a.ref_stride < w.fb)
      return fail(MRS_ERR_ARG, "ref_stride must be 0 (shared rows) or at least the width of the feedback groups");
    if (!w.costed && (a.target || a.weight || a.cost)) return fail(MRS_ERR_ARG, "cost_groups == 0 takes no dev_target, dev_weight or dev_cost");
  }
  if (w.costed) {
    if (tc && a.groups == 0u) {  // the crash cost alone
      if (a.target || a.weight) return fail(MRS_ERR_ARG, "groups == 0 (the crash cost alone) takes no dev_target or dev_weight");
    } else {
      if (a.groups == 0u) return fail(MRS_ERR_ARG, "no observation group selected: a cost needs columns");
      if (!a.target) return fail(MRS_ERR_ARG, "dev_target: null pointer");
      if (!a.weight) return fail(MRS_ERR_ARG, "dev_weight: null pointer");
    }
    if (!a.cost) return fail(MRS_ERR_ARG, "dev_cost: null pointer");
    if (a.target_stride != 0 && a.target_stride < w.obs)
      return fail(MRS_ERR_ARG, "target_stride must be 0 (shared rows) or at least the width of the selected groups");
    if (a.weight_stride != 0 && a.weight_stride < w.obs)
      return fail(MRS_ERR_ARG, "weight_stride must be 0 (one row) or at least the width of the selected groups");
  }
  if (a.count <= 0) return MRS_OK;
  // rows of the n_steps / cmd_every and n_steps / obs_every row blocks; 64-bit: blocks x count x stride can pass 2^31 elements
  const size_t elem = dtype_bytes(a.dtype), count = (size_t)a.count, width = (size_t)w.cmd;
  const size_t cmd_rows = (size_t)(a.n_steps / a.cmd_every) * count, obs_rows = (size_t)(a.n_steps / a.obs_every) * count;
  if (w.cmd > 0 && (rc = check_device_ptr(s, a.dev_cmd, ((cmd_rows - 1) * (size_t)a.cmd_stride + width) * elem, "dev_cmd"))) return rc;
  if (!cost && a.groups != 0u && (rc = check_device_ptr(s, a.dev_obs, ((obs_rows - 1) * (size_t)a.obs_stride + (size_t)w.obs) * elem, "dev_obs")))
    return rc;
  if (a.dev_crashed && (rc = check_device_ptr(s, a.dev_crashed, obs_rows, "dev_crashed"))) return rc;
  if (fb) {  // 64-bit: blocks x payload x row width x count can pass 2^31 elements
    const size_t gains = (size_t)a.gain_blocks * width * (size_t)w.fb * (a.gain_per_uav ? count : (size_t)1);
    const size_t refs  = a.ref_stride ? ((size_t)a.ref_blocks * count - 1) * (size_t)a.ref_stride + (size_t)w.fb : (size_t)a.ref_blocks * (size_t)w.fb;
    if ((rc = check_device_ptr(s, a.gain, gains * elem, "dev_gain"))) return rc;
    if ((rc = check_device_ptr(s, a.ref, refs * elem, "dev_ref"))) return rc;
  }
  if (w.costed) {  // (obs_rows: one target row per evaluation and UAV, unless the rows are shared)
    const size_t evals = (size_t)(a.n_steps / a.obs_every), ow = (size_t)w.obs;
    const size_t tgt   = a.target_stride ? (obs_rows - 1) * (size_t)a.target_stride + ow : evals * ow;
    const size_t wt    = a.weight_stride ? (evals - 1) * (size_t)a.weight_stride + ow : ow;
    if (a.groups != 0u && (rc = check_device_ptr(s, a.target, tgt * elem, "dev_target"))) return rc;
    if (a.groups != 0u && (rc = check_device_ptr(s, a.weight, wt * elem, "dev_weight"))) return rc;
    if ((rc = check_device_ptr(s, a.cost, count * sizeof(double), "dev_cost"))) return rc;
  }
  if (forced) {
    const size_t force_rows = (size_t)(a.n_steps / a.force_every) * count;
    if ((rc = check_device_ptr(s, a.dev_force, ((force_rows - 1) * (size_t)a.force_stride + 3u) * elem, "dev_force"))) return rc;
  }
  if (a.mode == MRS_ACTUATOR_CMD && !actuator_width_ok(s, a.first, a.count, w.cmd)) return fail(MRS_ERR_ARG, "actuator payload narrower than n_motors");
  return MRS_OK;
}

// the host's mirror of the modes: the launchers pick the cascade or the model-only kernels as mrs_swarm_step_n would after the first
// mrs_swarm_set_input_device of the loop the call stands for
static void rollout_track_mode(mrs_swarm_t* s, const RolloutArgs& a) {
  const uint8_t* m    = s->uav_mode.data() + a.first;
  unsigned       diff = 0;
  for (int k = 0; k < a.count; k++) diff |= (unsigned)(m[k] ^ (uint8_t)a.mode);
  if (diff) track_mode(s, a.first, a.count, a.mode);
}

// the rollout entry points but the tick rollout, under the caller's lock (MRS_ENTER's settle after the argument checks: a refused call
// launches nothing)
static int rollout_locked(mrs_swarm_t* s, const RolloutArgs& a) {
  const bool    fb = a.kind == ROLLOUT_FEEDBACK, cost = fb || a.kind == ROLLOUT_COST;
  RolloutWidths w;
  int           rc = check_rollout_args(s, a, "n_steps", cost ? "cost_every" : "obs_every", w);
  if (rc) return rc;
  if (s->n == 0) return MRS_OK;
  if ((rc = settle(s))) return rc;  // MRS_ENTER: a pending collision tick is evaluated first, its force acts on the first step
  HIPCHK(hipSetDevice(s->device));
  if ((rc = upload_types(s, a.dt))) return rc;
  rollout_track_mode(s, a);
  hipStream_t ext = (hipStream_t)a.ext_stream;
  if ((rc = fence_in(s, ext))) return rc;
  s->collide_since_step = false;
  s->p_valid            = false;  // (plain steps do not refresh the position records)
  const int      variant = s->n_cascade > 0 ? 0 : 1;  // 0 all input modes | 1 model only
  const bool     fast = s->arith == MRS_ARITH_FAST, f32 = a.dtype == MRS_DTYPE_F32;
  const uint32_t cmd_word = ((uint32_t)w.cmd | (f32 ? 32u : 0u)) << 24, mode_bits = (uint32_t)a.mode << FLAG_MODE_SHIFT;
  const int      first = a.first, count = a.count, n_steps = a.n_steps, cmd_every = a.cmd_every, obs_every = a.obs_every;
  void* const    obs = a.groups != 0u ? a.dev_obs : nullptr;
  // (each descriptor: row block 0 and the call's width, dtype and groups; the launcher sets each launch's schedule and first blocks)
  if (w.costed && count > 0 && !a.accumulate) HIPCHK(hipMemsetAsync(a.cost, 0, (size_t)count * sizeof(double), s->stream));  // (+0.0)
  const uint64_t tgt_blk = a.target_stride ? (uint64_t)count * (uint64_t)a.target_stride : (uint64_t)w.obs;
  if (fb) {  // the command is formed in the kernel: the feedback kernels of rollout_cost_device.inc, whatever the rates are
    RolloutFeedbackDev r{};
    r.cmd = a.dev_cmd, r.gain = a.gain, r.ref = a.ref;
    r.first = first, r.count = count, r.cmd_stride = a.cmd_stride;
    r.cmd_sched = cmd_word, r.mode_bits = mode_bits;
    if (w.costed) {
      r.target = a.target, r.weight = a.weight, r.cost = a.cost;
      r.cost_sched = count > 0 ? a.groups << 24 : 0u;
      r.tgt_row = a.target_stride, r.wt_row = a.weight_stride, r.tgt_blk = tgt_blk;
    }
    const uint64_t per = a.gain_per_uav ? (uint64_t)count : 1u;
    r.gain_col = (uint32_t)per, r.gain_lane = a.gain_per_uav ? 1 : 0;
    r.gain_blk = a.gain_blocks == 1 ? 0u : (uint64_t)w.cmd * (uint64_t)w.fb * per;
    r.ref_row  = a.ref_stride;
    r.ref_blk  = a.ref_blocks == 1 ? 0u : a.ref_stride ? (uint64_t)count * (uint64_t)a.ref_stride : (uint64_t)w.fb;
    r.fb_word  = a.fb_groups | (uint32_t)w.fb << 8;
    HIPCHK((fast ? mrs_launch_rollout_feedback_fast : mrs_launch_rollout_feedback_literal)(s->view(), r, a.dt, n_steps, cmd_every, obs_every, variant, s->stream));
  } else if (cost) {  // evaluations in place of observation rows: the cost kernels of rollout_cost_device.inc, whatever the rates are
    RolloutCostDev r{};
    r.cmd = a.dev_cmd, r.target = a.target, r.weight = a.weight, r.cost = a.cost;
    r.first = first, r.count = count, r.cmd_stride = a.cmd_stride;
    r.cmd_sched = cmd_word, r.mode_bits = mode_bits;
    r.cost_sched = count > 0 ? a.groups << 24 : 0u;
    r.tgt_row = a.target_stride, r.wt_row = a.weight_stride, r.tgt_blk = tgt_blk;
    HIPCHK((fast ? mrs_launch_rollout_cost_fast : mrs_launch_rollout_cost_literal)(s->view(), r, a.dt, n_steps, cmd_every, obs_every, variant, s->stream));
  } else if (a.kind == ROLLOUT_FORCE) {  // a third schedule: the force kernels of rollout_rate_device.inc, whatever the rates are
    if (count > 0) s->fext_active = true;  // (the loop's first mrs_swarm_apply_force_device: from here on the steps read the F_FEXT columns)
    RolloutForceDev r{};
    r.cmd = a.dev_cmd, r.obs = obs, r.force = count > 0 ? a.dev_force : nullptr;
    r.first = first, r.count = count;
    r.cmd_stride = a.cmd_stride, r.obs_stride = a.obs_stride, r.force_stride = a.force_stride;
    r.cmd_sched = cmd_word, r.obs_sched = a.groups << 24, r.mode_bits = mode_bits;
    HIPCHK((fast ? mrs_launch_rollout_force_fast : mrs_launch_rollout_force_literal)(s->view(), r, a.dt, n_steps, cmd_every, obs_every, a.force_every, variant,
                                                                                     s->stream));
  } else if (cmd_every == 1 && obs_every == 1) {  // a row before and after every step: the kernels of rollout_device.inc
    const RolloutDev r{a.dev_cmd, obs, first, count, a.cmd_stride, w.cmd, a.obs_stride, 0, mode_bits, a.groups, f32 ? 1 : 0};
    HIPCHK((fast ? mrs_launch_rollout_fast : mrs_launch_rollout_literal)(s->view(), r, a.dt, n_steps, variant, s->stream));
  } else {  // the rate kernels of rollout_rate_device.inc
    RolloutRateDev r{};
    r.cmd = a.dev_cmd, r.obs = obs;
    r.first = first, r.count = count;
    r.cmd_stride = a.cmd_stride, r.obs_stride = a.obs_stride;
    r.cmd_sched = cmd_word, r.obs_sched = a.groups << 24, r.mode_bits = mode_bits;
    HIPCHK((fast ? mrs_launch_rollout_rate_fast : mrs_launch_rollout_rate_literal)(s->view(), r, a.dt, n_steps, cmd_every, obs_every, variant, s->stream));
  }
  return fence_out(s, ext);
}

int mrs_swarm_rollout_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_steps, const void* dev_cmd,
                             int32_t dtype, int32_t cmd_stride, uint32_t groups, void* dev_obs, int32_t obs_stride, void* ext_stream) {
  MRS_LOCK(s);
  return rollout_locked(s, RolloutArgs{"mrs_swarm_rollout_device", ROLLOUT_ROWS, first, count, mode, dt, n_steps, 1, 1, dev_cmd, dtype, cmd_stride, groups,
                                       dev_obs, obs_stride, ext_stream});
}

int mrs_swarm_rollout_rate_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_steps, int32_t cmd_every,
                                  int32_t obs_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride, uint32_t groups, void* dev_obs,
                                  int32_t obs_stride, void* ext_stream) {
  MRS_LOCK(s);
  return rollout_locked(s, RolloutArgs{"mrs_swarm_rollout_rate_device", ROLLOUT_ROWS, first, count, mode, dt, n_steps, cmd_every, obs_every, dev_cmd, dtype,
                                       cmd_stride, groups, dev_obs, obs_stride, ext_stream});
}

int mrs_swarm_rollout_force_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_steps, int32_t cmd_every,
                                   int32_t obs_every, int32_t force_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride,
                                   const void* dev_force, int32_t force_stride, uint32_t groups, void* dev_obs, int32_t obs_stride, void* ext_stream) {
  MRS_LOCK(s);
  RolloutArgs a{"mrs_swarm_rollout_force_device", ROLLOUT_FORCE, first, count, mode, dt, n_steps, cmd_every, obs_every, dev_cmd, dtype, cmd_stride, groups,
                dev_obs, obs_stride, ext_stream};
  a.force_every = force_every, a.dev_force = dev_force, a.force_stride = force_stride;
  return rollout_locked(s, a);
}

int mrs_swarm_rollout_cost_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_steps, int32_t cmd_every,
                                  int32_t cost_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride, uint32_t groups,
                                  const void* dev_target, int32_t target_stride, const void* dev_weight, int32_t weight_stride, double* dev_cost,
                                  int32_t accumulate, void* ext_stream) {
  MRS_LOCK(s);
  RolloutArgs a{"mrs_swarm_rollout_cost_device", ROLLOUT_COST, first, count, mode, dt, n_steps, cmd_every, cost_every, dev_cmd, dtype, cmd_stride, groups,
                nullptr, 0, ext_stream};
  a.target = dev_target, a.target_stride = target_stride, a.weight = dev_weight, a.weight_stride = weight_stride;
  a.cost = dev_cost, a.accumulate = accumulate;
  return rollout_locked(s, a);
}

int mrs_swarm_rollout_feedback_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_steps, int32_t cmd_every,
                                      int32_t cost_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride, uint32_t fb_groups,
                                      const void* dev_gain, int32_t gain_per_uav, int32_t gain_blocks, const void* dev_ref, int32_t ref_stride,
                                      int32_t ref_blocks, uint32_t cost_groups, const void* dev_target, int32_t target_stride,
                                      const void* dev_weight, int32_t weight_stride, double* dev_cost, int32_t accumulate, void* ext_stream) {
  MRS_LOCK(s);
  RolloutArgs a{"mrs_swarm_rollout_feedback_device", ROLLOUT_FEEDBACK, first, count, mode, dt, n_steps, cmd_every, cost_every, dev_cmd, dtype, cmd_stride,
                cost_groups, nullptr, 0, ext_stream};
  a.target = dev_target, a.target_stride = target_stride, a.weight = dev_weight, a.weight_stride = weight_stride;
  a.cost = dev_cost, a.accumulate = accumulate;
  a.fb_groups = fb_groups, a.gain = dev_gain, a.gain_per_uav = gain_per_uav, a.gain_blocks = gain_blocks;
  a.ref = dev_ref, a.ref_stride = ref_stride, a.ref_blocks = ref_blocks;
  return rollout_locked(s, a);
}

// The tick rollouts are timerMain over n_ticks ticks with what each tick carries of the caller's memory (mrs_swarm::TickLoad): every
// tick is step_one (tick_single.hip) with that tick's pointers, then the tick's handleCollisions stays pending as after
// mrs_swarm_tick_n.  The launches of the call carry their descriptors through the stall / replay log, and the call drains the log
// before it returns.

// what every tick of the call carries alike: the descriptor of the call's kind without a pointer
static mrs_swarm::TickLoad tick_load(const RolloutArgs& a, const RolloutWidths& w) {
  mrs_swarm::TickLoad p;
  const uint32_t cmd_word = (uint32_t)w.cmd | (a.dtype == MRS_DTYPE_F32 ? 32u : 0u), mode_bits = (uint32_t)a.mode << FLAG_MODE_SHIFT;
  if (a.kind == ROLLOUT_TICK) {
    p.kind = mrs_swarm::TickLoad::ROWS;
    RolloutTickDev& r = p.row = RolloutTickDev{};
    r.first = a.first, r.count = a.count;
    r.cmd_stride = a.cmd_stride, r.obs_stride = a.obs_stride;
    r.cmd_word = cmd_word, r.groups = a.groups, r.mode_bits = mode_bits;
  } else if (a.kind == ROLLOUT_TICK_COST) {
    p.kind = mrs_swarm::TickLoad::COST;
    RolloutTickCostDev& c = p.cost = RolloutTickCostDev{};
    c.first = a.first, c.count = a.count;
    c.cmd_stride = a.cmd_stride;
    c.tgt_row = a.target_stride, c.wt_row = a.weight_stride, c.width = w.obs;
    c.cmd_word = cmd_word, c.groups = a.groups, c.mode_bits = mode_bits;
    c.crash_cost = a.crash_cost;
  } else {
    p.kind = mrs_swarm::TickLoad::FEEDBACK;
    RolloutTickFeedbackDev& f = p.fb = RolloutTickFeedbackDev{};
    f.first = a.first, f.count = a.count;
    f.cmd_stride = a.cmd_stride;
    f.ref_row = a.ref_stride, f.tgt_row = a.target_stride;
    f.gain_lane = a.gain_per_uav ? 1 : 0, f.gain_col = a.gain_per_uav ? (uint32_t)a.count : 1u;
    f.fb_word  = a.fb_groups | (uint32_t)w.fb << 8;
    f.cmd_word = cmd_word, f.groups = a.groups, f.mode_bits = mode_bits;
    f.crash_cost = a.crash_cost;
  }
  return p;
}

// block `blk` of a call's blocks, which lie `per_blk` elements of `elem` bytes apart (none: null)
static const void* tick_block(const void* base, long long blk, size_t per_blk, size_t elem) {
  return blk >= 0 ? static_cast<const char*>(base) + (size_t)blk * per_blk * elem : nullptr;
}
// The pointers of tick t: the blocks that start at it (commands; gains and setpoints, of which one block may serve every command
// block) and the blocks that end with it (observation and crash rows; the evaluation).  An empty range has none.
static void tick_pointers(mrs_swarm::TickLoad& p, const RolloutArgs& a, const RolloutWidths& w, int t) {
  const size_t    elem = dtype_bytes(a.dtype), count = (size_t)a.count;
  const long long b    = a.count > 0 && w.cmd > 0 ? mrs_tick_block_start(t, a.cmd_every, a.n_steps / a.cmd_every) : -1;
  const long long j    = a.count > 0 && (w.costed || a.kind == ROLLOUT_TICK) ? mrs_tick_block_end(t, a.obs_every, a.n_steps / a.obs_every) : -1;
  const void*     cmd  = tick_block(a.dev_cmd, b, count * (size_t)a.cmd_stride, elem);
  // the evaluation that ends with a tick of a costed tick rollout: the caller's vector, and with cost groups the evaluation's target
  // rows (a row per UAV, or one dense row for all) and weight row
  auto evaluation = [&](auto& d) {
    const long long rows    = a.groups != 0u ? j : -1;
    const size_t    tgt_blk = a.target_stride ? count * (size_t)a.target_stride : (size_t)w.obs;
    d.cost   = j >= 0 ? a.cost : nullptr;
    d.target = tick_block(a.target, rows, tgt_blk, elem);
    d.weight = tick_block(a.weight, rows, (size_t)a.weight_stride, elem);
  };
  switch (p.kind) {
    case mrs_swarm::TickLoad::ROWS:
      p.row.cmd     = cmd;
      p.row.obs     = a.groups != 0u ? const_cast<void*>(tick_block(a.dev_obs, j, count * (size_t)a.obs_stride, elem)) : nullptr;
      p.row.crashed = a.dev_crashed && j >= 0 ? a.dev_crashed + (size_t)j * count : nullptr;
      break;
    case mrs_swarm::TickLoad::COST:
      p.cost.cmd = cmd;
      evaluation(p.cost);
      break;
    case mrs_swarm::TickLoad::FEEDBACK: {
      const size_t per      = a.gain_per_uav ? count : (size_t)1;
      const size_t gain_blk = a.gain_blocks == 1 ? 0u : (size_t)w.cmd * (size_t)w.fb * per;
      const size_t ref_blk  = a.ref_blocks == 1 ? 0u : a.ref_stride ? count * (size_t)a.ref_stride : (size_t)w.fb;
      p.fb.cmd  = cmd;
      p.fb.gain = tick_block(a.gain, b, gain_blk, elem);
      p.fb.ref  = tick_block(a.ref, b, ref_blk, elem);
      evaluation(p.fb);
      break;
    }
    case mrs_swarm::TickLoad::NONE: break;
  }
}

// the three tick rollout entry points, under the caller's lock
static int rollout_tick_locked(mrs_swarm_t* s, const RolloutArgs& a) {
  RolloutWidths w;
  int           rc = check_rollout_args(s, a, "n_ticks", a.kind == ROLLOUT_TICK ? "obs_every" : "cost_every", w);
  if (rc) return rc;
  if (s->n == 0) return MRS_OK;
  HIPCHK(hipSetDevice(s->device));
  // like a command call: launches queued by earlier calls must have run before the mode mirror (which picks the kernel variant of a
  // replay) changes; a collision tick pending at entry stays pending — the first launch of this call evaluates it
  if (!s->log.empty() && (rc = drain(s))) return rc;
  if ((rc = upload_types(s, a.dt))) return rc;
  rollout_track_mode(s, a);
  hipStream_t ext = (hipStream_t)a.ext_stream;
  if ((rc = fence_in(s, ext))) return rc;
  if ((rc = begin_profile(s))) return rc;
  // dev_cost is zeroed once on the swarm's stream, behind the entry fence and in front of the first launch, unless the call
  // accumulates; the memset is not part of the launch log, so a replay after a stall does not repeat it, and the replayed launches add
  // what their no-ops did not.  (A feedback tick rollout without a dev_cost evaluates nothing: a pure closed-loop run.)
  if (w.costed && a.count > 0 && !a.accumulate) HIPCHK(hipMemsetAsync(a.cost, 0, (size_t)a.count * sizeof(double), s->stream));  // (+0.0)
  mrs_swarm::TickLoad p = tick_load(a, w);
  for (int t = 0; t < a.n_steps; t++) {
    tick_pointers(p, a, w, t);
    if ((rc = step_one(s, a.dt, &p))) return rc;
    if ((rc = mrs_swarm_handle_collisions(s, 1, a.crash, a.rebounce))) return rc;
  }
  // nothing of this call stays in the log: a replay after a stall writes into the caller's rows, reads the caller's rows and gains and
  // adds to the caller's vector, which are only guaranteed to live until the call returns (one host wait per call); the last tick's
  // collision stays pending
  if ((rc = drain(s))) return rc;
  if ((rc = finish_profile(s))) return rc;
  return fence_out(s, ext);
}

int mrs_swarm_rollout_tick_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_ticks, int32_t cmd_every,
                                  int32_t obs_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride, uint32_t groups, void* dev_obs,
                                  int32_t obs_stride, uint8_t* dev_crashed, int32_t crash, double rebounce, void* ext_stream) {
  MRS_LOCK(s);
  RolloutArgs a{"mrs_swarm_rollout_tick_device", ROLLOUT_TICK, first, count, mode, dt, n_ticks, cmd_every, obs_every, dev_cmd, dtype, cmd_stride, groups,
                dev_obs, obs_stride, ext_stream};
  a.dev_crashed = dev_crashed, a.crash = crash, a.rebounce = rebounce;
  return rollout_tick_locked(s, a);
}

// mrs_swarm_rollout_tick_device whose ticks carry an evaluation in place of row blocks
int mrs_swarm_rollout_tick_cost_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_ticks, int32_t cmd_every,
                                       int32_t cost_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride, uint32_t groups,
                                       const void* dev_target, int32_t target_stride, const void* dev_weight, int32_t weight_stride,
                                       double crash_cost, double* dev_cost, int32_t accumulate, int32_t crash, double rebounce, void* ext_stream) {
  MRS_LOCK(s);
  RolloutArgs a{"mrs_swarm_rollout_tick_cost_device", ROLLOUT_TICK_COST, first, count, mode, dt, n_ticks, cmd_every, cost_every, dev_cmd, dtype, cmd_stride,
                groups, nullptr, 0, ext_stream};
  a.target = dev_target, a.target_stride = target_stride, a.weight = dev_weight, a.weight_stride = weight_stride;
  a.cost = dev_cost, a.accumulate = accumulate;
  a.crash = crash, a.rebounce = rebounce, a.crash_cost = crash_cost;
  return rollout_tick_locked(s, a);
}

// mrs_swarm_rollout_tick_cost_device whose command rows are nominal commands: every tick at which a command block starts carries that
// block's nominal commands, gains and setpoints, and the launch forms the command from the state before the step
int mrs_swarm_rollout_tick_feedback_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t mode, double dt, int32_t n_ticks, int32_t cmd_every,
                                           int32_t cost_every, const void* dev_cmd, int32_t dtype, int32_t cmd_stride, uint32_t fb_groups,
                                           const void* dev_gain, int32_t gain_per_uav, int32_t gain_blocks, const void* dev_ref, int32_t ref_stride,
                                           int32_t ref_blocks, uint32_t cost_groups, const void* dev_target, int32_t target_stride,
                                           const void* dev_weight, int32_t weight_stride, double crash_cost, double* dev_cost, int32_t accumulate,
                                           int32_t crash, double rebounce, void* ext_stream) {
  MRS_LOCK(s);
  RolloutArgs a{"mrs_swarm_rollout_tick_feedback_device", ROLLOUT_TICK_FEEDBACK, first, count, mode, dt, n_ticks, cmd_every, cost_every, dev_cmd, dtype,
                cmd_stride, cost_groups, nullptr, 0, ext_stream};
  a.target = dev_target, a.target_stride = target_stride, a.weight = dev_weight, a.weight_stride = weight_stride;
  a.cost = dev_cost, a.accumulate = accumulate;
  a.fb_groups = fb_groups, a.gain = dev_gain, a.gain_per_uav = gain_per_uav, a.gain_blocks = gain_blocks;
  a.ref = dev_ref, a.ref_stride = ref_stride, a.ref_blocks = ref_blocks;
  a.crash = crash, a.rebounce = rebounce, a.crash_cost = crash_cost;
  return rollout_tick_locked(s, a);
}

}  // extern "C"
