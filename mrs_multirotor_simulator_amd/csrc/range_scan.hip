// range_scan.hip — range scans (include/mrs_swarm.h, "range scans"): the beam pattern a swarm owns, and the device-resident scan that
// casts every beam of every UAV against the static obstacles and, if asked, the ground plane.  One lane per (UAV, beam), beams fastest, so
// a row's stores are coalesced and the lanes of one UAV walk the same cell list and load the same 64-B obstacle records (they stay in
// cache).  A lane reads the ONE grid cell that contains its UAV (obstacle_grid.h, built for radius = max_range: it lists every candidate
// of the contract's gate), tests every listed obstacle literally (world rule, gate, ray) and keeps (t, index) in two registers: no list,
// no LDS, no atomics.  The gate is recomputed by every lane (DESIGN §7c says why).  The pure functions are those of range_scan_math.h.
// Nothing here writes simulation state; the scan enters like mrs_swarm_nearest_obstacles_device (a pending collision tick stays pending).
#include "host_internal.h"
#include "obstacle_set.h"
#include "pose_math.h"
#include "range_scan_math.h"

struct ScanBeams {
  std::vector<double> host;  // n_beams x 3 unit vectors as given (get_scan_beams, clone)
  DevBuf<double>      dev;
};

namespace {

constexpr int RS_BLOCK = 256;

struct ScanArgs {
  const double*         S;
  const uint32_t*       F;
  const TypeParams*     T;
  const uint32_t*       wlab;  // null: every UAV is in world 0
  int32_t               npad, first, n_beams;
  uint32_t              flags;
  int64_t               lanes;  // count * n_beams
  const double*         beams;
  double                max_range;
  mrs_obst::Grid        g;
  const int32_t *       start, *items;
  const mrs_obstacle_t* obst;
  int32_t               m, n_items;
  void*                 ranges;
  int32_t*              hit;
  int32_t               stride, hit_stride;
};

template <typename T>
__global__ void __launch_bounds__(RS_BLOCK) k_range_scan(ScanArgs a) {
  const int64_t lane = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (lane >= a.lanes) return;
  const int    r  = (int)(lane / a.n_beams), b = (int)(lane - (int64_t)r * a.n_beams);
  const int    i  = a.first + r;
  const size_t np = (size_t)a.npad;
  double       p[3], u[3];
  p[0] = a.S[(size_t)F_X * np + i];
  p[1] = a.S[(size_t)(F_X + 1) * np + i];
  p[2] = a.S[(size_t)(F_X + 2) * np + i];
  const double bm[3] = {a.beams[3 * b], a.beams[3 * b + 1], a.beams[3 * b + 2]};
  if (a.flags & MRS_SCAN_BODY_FRAME) {  // u = R b: row c of R times b, as body_velocity forms a column of its argument times a vector
    double Rt[9];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int k = 0; k < 3; k++) Rt[3 * k + c] = a.S[(size_t)(F_R + 3 * c + k) * np + i];
    u[0] = body_velocity(Rt, bm, 0), u[1] = body_velocity(Rt, bm, 1), u[2] = body_velocity(Rt, bm, 2);
  } else {
    u[0] = bm[0], u[1] = bm[1], u[2] = bm[2];
  }
  double best = a.max_range;
  int    idx  = MRS_SCAN_HIT_NONE;
  if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
    if (a.m > 0) {
      const uint32_t myw = a.wlab ? a.wlab[i] : 0u;
      const int64_t  q   = mrs_obst::cell_of(a.g, p[0], p[1], p[2]);  // (inside the grid by the clamp of cell_coord)
      const int      beg = max(a.start[q], 0), end = min(a.start[q + 1], a.n_items);
      for (int s = beg; s < end; s++) {  // obstacle indices ascend within a cell: a strict < keeps the lowest index among equal ranges
        const int j = a.items[s];
        if ((unsigned)j >= (unsigned)a.m) continue;
        const mrs_obstacle_t o = a.obst[j];
        if (!(o.flags & (uint32_t)MRS_OBST_ALL_WORLDS) && (uint32_t)o.world != myw) continue;  // another world's obstacle
        if (!mrs_scan::gate(o, p, a.max_range)) continue;
        const double t = mrs_scan::ray(o, p, u);
        if (t < best) {
          best = t;
          idx  = j;
        }
      }
    }
    if (a.flags & MRS_SCAN_GROUND) {
      const double t = mrs_scan::ground(p[2], u[2], a.T[a.F[i] >> FLAG_TYPE_SHIFT].ground_z);
      if (t < best) {
        best = t;
        idx  = MRS_SCAN_HIT_GROUND;
      }
    }
  }
  static_cast<T*>(a.ranges)[(size_t)r * (size_t)a.stride + (size_t)b] = (T)best;
  if (a.hit) a.hit[(size_t)r * (size_t)a.hit_stride + (size_t)b] = idx;
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

// The scans' grid for max_range: built and uploaded on the swarm's stream when the cached one serves another range or another set.
// Called after every argument check and before the entry fence (the upload reads nothing of the caller's).
int ensure_scan_grid(mrs_swarm* s, double max_range) {
  if (!s->obst) s->obst = new ObstacleSet;
  ObstacleSet*       o = s->obst;
  ObstacleGridCache& c = o->scan;
  if (c.ok && c.grid.radius == max_range) return MRS_OK;
  mrs_obst::Built b = mrs_obst::build(o->host.data(), (int32_t)o->host.size(), max_range);
  HIPCHK(hipStreamSynchronize(s->stream));  // (a scan may still read the cached grid, and its host vectors may still be uploading)
  c.ok = false;
  HIPCHK(c.d_start.reserve(b.start.size()));
  HIPCHK(c.d_items.reserve(std::max<size_t>(b.items.size(), 1)));
  c.grid = std::move(b);
  HIPCHK(hipMemcpyAsync(c.d_start, c.grid.start.data(), sizeof(int32_t) * c.grid.start.size(), hipMemcpyHostToDevice, s->stream));
  if (!c.grid.items.empty())
    HIPCHK(hipMemcpyAsync(c.d_items, c.grid.items.data(), sizeof(int32_t) * c.grid.items.size(), hipMemcpyHostToDevice, s->stream));
  c.ok = true;
  o->builds++;
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
// for the scans that see other UAVs (range_scan_uavs.hip): the pattern's size and device copy, and the scans' cached obstacle grid
int32_t       scan_beam_count(const mrs_swarm* s) { return s->scan ? (int32_t)(s->scan->host.size() / 3) : 0; }
const double* scan_beams_dev(const mrs_swarm* s) { return s->scan ? s->scan->dev.get() : nullptr; }
int           scan_grid(mrs_swarm* s, double max_range) { return ensure_scan_grid(s, max_range); }
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
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, "mrs_swarm_range_scan_device: not on a sharded swarm");
  const int32_t nb = s->scan ? (int32_t)(s->scan->host.size() / 3) : 0;
  if (nb == 0) return fail(MRS_ERR_ARG, "no beam pattern set (mrs_swarm_set_scan_beams)");
  if (!(max_range > 0.0) || !std::isfinite(max_range)) return fail(MRS_ERR_ARG, "max_range must be finite and > 0");
  if (flags & ~(uint32_t)(MRS_SCAN_BODY_FRAME | MRS_SCAN_GROUND)) return fail(MRS_ERR_ARG, "unknown scan flag bits");
  if ((rc = check_dtype(dtype))) return rc;
  if (stride < nb) return fail(MRS_ERR_ARG, "stride smaller than n_beams");
  if (dev_hit && hit_stride < nb) return fail(MRS_ERR_ARG, "hit_stride smaller than n_beams");
  if (!dev_ranges) return fail(MRS_ERR_ARG, "dev_ranges: null pointer");
  if (((int64_t)count * nb + RS_BLOCK - 1) / RS_BLOCK > 0x7FFFFFFFll) return fail(MRS_ERR_ARG, "count * n_beams exceeds one launch (2^31 blocks of 256 beams)");
  if (count == 0) return MRS_OK;
  if ((rc = check_device_ptr(s, dev_ranges, rows_bytes(count, stride, nb, dtype), "dev_ranges"))) return rc;
  if (dev_hit && (rc = check_device_ptr(s, dev_hit, ((size_t)(count - 1) * (size_t)hit_stride + (size_t)nb) * sizeof(int32_t), "dev_hit"))) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  // the ground plane is read from the airframe table, as the rangefinder of outputs.hip reads it: current before the launch
  if ((flags & MRS_SCAN_GROUND) && (rc = upload_types(s, s->table_dt > 0 ? s->table_dt : 0.001))) return rc;
  if ((rc = ensure_scan_grid(s, max_range))) return rc;
  if ((rc = fence_in(s, ext))) return rc;
  const ObstacleSet* o = s->obst;
  ScanArgs           a;
  memset(&a, 0, sizeof a);
  a.S          = s->dS;
  a.F          = s->dF;
  a.T          = s->dT;
  a.wlab       = s->dWorld;
  a.npad       = s->npad;
  a.first      = first;
  a.n_beams    = nb;
  a.flags      = flags;
  a.lanes      = (int64_t)count * nb;
  a.beams      = s->scan->dev;
  a.max_range  = max_range;
  a.g          = o->scan.grid.g;
  a.start      = o->scan.d_start;
  a.items      = o->scan.d_items;
  a.obst       = o->dev;
  a.m          = (int32_t)o->host.size();
  a.n_items    = (int32_t)o->scan.grid.items.size();
  a.ranges     = dev_ranges;
  a.hit        = dev_hit;
  a.stride     = stride;
  a.hit_stride = hit_stride;
  const dim3 grid((unsigned)((a.lanes + RS_BLOCK - 1) / RS_BLOCK));
  if (dtype == MRS_DTYPE_F32)
    hipLaunchKernelGGL(k_range_scan<float>, grid, dim3(RS_BLOCK), 0, s->stream, a);
  else
    hipLaunchKernelGGL(k_range_scan<double>, grid, dim3(RS_BLOCK), 0, s->stream, a);
  HIPCHK(hipGetLastError());
  return fence_out(s, ext);
}

}  // extern "C"
