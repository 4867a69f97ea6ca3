// range_scan.hip — range scans (include/mrs_swarm.h, "range scans"): the beam pattern a swarm owns, and the device-resident scan that
// casts every beam of every UAV against the static obstacles and, if asked, the ground plane.  One lane per (UAV, beam), beams fastest, so
// a row's stores are coalesced and the lanes of one UAV walk the same cell list and load the same 64-B obstacle records (they stay in
// cache).  A lane reads the ONE grid cell that contains its UAV (obstacle_grid.h, built for radius = max_range: it lists every candidate
// of the contract's gate), tests every listed obstacle literally (world rule, gate, ray) and keeps (t, index) in two registers: no list,
// no LDS, no atomics.  The gate is recomputed by every lane (DESIGN §7c says why).  The pure functions are those of range_scan_math.h;
// beam set-up, obstacle pass (over mrs_obst::walk_cell), ground pass, stores, argument checks and argument fill are those of
// range_scan_common.h, which range_scan_uavs.hip calls too: this unit keeps the beam pattern, the lane mapping and the entry point.
// Nothing here writes simulation state; the scan enters like mrs_swarm_nearest_obstacles_device (a pending collision tick stays pending).
#include "range_scan_common.h"

struct ScanBeams {
  std::vector<double> host;  // n_beams x 3 unit vectors as given (get_scan_beams, clone)
  DevBuf<double>      dev;
};

namespace {

constexpr int RS_BLOCK = 256;

struct ScanArgs {
  ScanCommon      c;
  const uint32_t* wlab;   // null: every UAV is in world 0
  int64_t         lanes;  // count * n_beams
};

template <typename T>
__global__ void __launch_bounds__(RS_BLOCK) k_range_scan(ScanArgs a) {
  const int64_t lane = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (lane >= a.lanes) return;
  const int r = (int)(lane / a.c.n_beams), b = (int)(lane - (int64_t)r * a.c.n_beams);
  const int i = a.c.first + r;
  double    p[3], u[3];
  scan_beam(a.c, i, b, p, u);
  double best = a.c.max_range;
  int    idx  = MRS_SCAN_HIT_NONE;
  if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
    if (a.c.v.m > 0) scan_obstacles(a.c, p, u, a.wlab ? a.wlab[i] : 0u, &best, &idx);
    (void)scan_ground(a.c, i, p, u, &best, &idx);
  }
  scan_store<T>(a.c, r, b, best, idx);
}

const char* bad_beam(const double* d) {
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(d[c])) return "not finite";
  const double e = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) - 1.0;
  return std::fabs(e) <= 1e-9 ? nullptr : "not a unit vector (|b|^2 differs from 1 by more than 1e-9)";
}

// replaces the pattern of s by n validated beams: host copy, device copy behind everything queued on the swarm's stream
int adopt_beams(mrs_swarm* s, const double* dirs, int32_t n) {
  if (!s->scan) s->scan = new ScanBeams;
  ScanBeams* sb = s->scan;
  HIPCHK(hipStreamSynchronize(s->stream));  // (a scan of the old pattern may still be running)
  std::vector<double> fresh(dirs, dirs + (size_t)n * 3);
  if (n > 0) {
    HIPCHK(sb->dev.reserve((size_t)n * 3));
    HIPCHK(hipMemcpyAsync(sb->dev, fresh.data(), sizeof(double) * (size_t)n * 3, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
  }
  sb->host.swap(fresh);
  return MRS_OK;
}

}  // namespace

extern "C" void mrs_scan_beams_free(ScanBeams* b) { delete b; }

namespace mrs_host {
// the pattern of src into dst (mrs_swarm_clone*); dst is idle
int scan_beams_copy(mrs_swarm* dst, const mrs_swarm* src) {
  if (!src->scan || src->scan->host.empty()) return MRS_OK;
  return adopt_beams(dst, src->scan->host.data(), (int32_t)(src->scan->host.size() / 3));
}
// for range_scan_common.h and the scans that see other UAVs (range_scan_uavs.hip): the pattern's size (asked before the checks: a null
// swarm has none) and device copy
int32_t       scan_beam_count(const mrs_swarm* s) { return s && s->scan ? (int32_t)(s->scan->host.size() / 3) : 0; }
const double* scan_beams_dev(const mrs_swarm* s) { return s->scan ? s->scan->dev.get() : nullptr; }
}  // namespace mrs_host

extern "C" {

int mrs_swarm_set_scan_beams(mrs_swarm_t* s, int32_t n_beams, const double* dirs) {
  MRS_ENTER_COMMANDS(s);  // (no simulation state is written: a pending collision tick stays pending)
  if (!s) return fail(MRS_ERR_ARG, "null swarm");
  if (n_beams < 0 || n_beams > MRS_SCAN_MAX_BEAMS) return fail(MRS_ERR_ARG, "n_beams must be in [0, MRS_SCAN_MAX_BEAMS]");
  if (n_beams > 0 && !dirs) return fail(MRS_ERR_ARG, "null dirs");
  for (int32_t b = 0; b < n_beams; b++)
    if (const char* why = bad_beam(dirs + 3 * (size_t)b)) return fail(MRS_ERR_ARG, "beam " + std::to_string(b) + ": " + why);
  HIPCHK(hipSetDevice(s->device));
  return adopt_beams(s, dirs, n_beams);
}

int mrs_swarm_get_scan_beams(const mrs_swarm_t* s, int32_t capacity, double* out, int32_t* n_beams) {
  MRS_LOCK(s);
  if (!s || !n_beams) return fail(MRS_ERR_ARG, "null argument");
  const size_t n = s->scan ? s->scan->host.size() / 3 : 0;
  *n_beams = (int32_t)n;
  if (!out) return MRS_OK;
  if (capacity < (int32_t)n) return fail(MRS_ERR_ARG, "capacity smaller than the pattern");
  if (n) memcpy(out, s->scan->host.data(), sizeof(double) * 3 * n);
  return MRS_OK;
}

int mrs_swarm_range_scan_device(mrs_swarm_t* s, int32_t first, int32_t count, double max_range, uint32_t flags, void* dev_ranges, int32_t dtype,
                                int32_t stride, int32_t* dev_hit, int32_t hit_stride, void* ext_stream) {
  MRS_ENTER_COMMANDS(s);
  const int32_t  nb = scan_beam_count(s);
  const ScanRows rows{dev_ranges, dtype, stride, dev_hit, hit_stride, nullptr, 0};
  int            rc = check_scan(s, "mrs_swarm_range_scan_device", nb, first, count, max_range, flags, rows, ((int64_t)count * nb + RS_BLOCK - 1) / RS_BLOCK,
                                 "count * n_beams exceeds one launch (2^31 blocks of 256 beams)");
  if (rc || count == 0) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  // the ground plane is read from the airframe table, as the rangefinder of outputs.hip reads it: current before the launch
  if ((flags & MRS_SCAN_GROUND) && (rc = upload_types(s, s->table_dt > 0 ? s->table_dt : 0.001))) return rc;
  if ((rc = scan_grid(s, max_range))) return rc;
  if ((rc = fence_in(s, ext))) return rc;
  const ScanArgs a{scan_common(s, first, nb, max_range, flags, rows), s->dWorld, (int64_t)count * nb};
  const dim3     grid((unsigned)((a.lanes + RS_BLOCK - 1) / RS_BLOCK));
  if (dtype == MRS_DTYPE_F32)
    hipLaunchKernelGGL(k_range_scan<float>, grid, dim3(RS_BLOCK), 0, s->stream, a);
  else
    hipLaunchKernelGGL(k_range_scan<double>, grid, dim3(RS_BLOCK), 0, s->stream, a);
  HIPCHK(hipGetLastError());
  return fence_out(s, ext);
}

}  // extern "C"
