// obstacles.hip — static obstacles (include/mrs_swarm.h, "static obstacles"): the set a swarm owns, and the two device-resident queries
// against it — the k nearest obstacles of each UAV as observation rows (k_obst_rows) and a per-UAV penalty over them added into the FP64
// cost vector of the cost rollouts (k_obst_cost).  Both are one search: a lane per query UAV reads the ONE grid cell that contains its
// position (obstacle_grid.h: inflated binning, built on the host, cached per radius), tests every obstacle listed there literally
// (world rule, sd < radius) and keeps the first KC by (sd, obstacle index) in a register list.  A wave's lanes sit in unrelated cells, so
// the walk diverges; the lists are short (a cell's neighbourhood) and the 64-B obstacle records stay in cache.
// The steps of the walk are those of mrs_obst::walk_cell (obstacle_grid.h), which both range scans call, over the same GridView;
// obst_search keeps them as a loop of its own because the callable form measured slower here ("One cell walk ...").
// This unit also owns the set and ensure(), the one routine that makes a cached grid current, for the queries' entry and, through
// mrs_host::scan_grid, mrs_host::contact_grid and mrs_host::sight_grid, for the scans', the contacts' and the sight lines'.
// The sorted insertion stays here, a text of its own beside nearest.hip's nn_probe: it orders by (sd, obstacle index) over a list this
// kernel keeps, nn_probe by (d2, UAV index) inside a probe loop whose measured schedule a shared template would disturb — that unit
// stays as it is.
// Nothing here writes simulation state; the calls enter like mrs_swarm_nearest_device (a pending collision tick stays pending).
#include <type_traits>

#include "host_internal.h"
#include "obstacle_grid.h"
#include "obstacle_set.h"
#include "pose_math.h"

namespace {

constexpr int OB_BLOCK     = 256;
constexpr int kOnWidth[3]  = {3, 3, 1};

struct ObstArgs {
  const double*         S;
  const uint32_t*       wlab;  // null: every UAV is in world 0
  int32_t               n, npad, first, count, k;
  double                radius;
  mrs_obst::GridView    v;
  // rows of k_obst_rows
  void*    rows;
  int32_t  stride, width;  // width: elements of one slot
  uint32_t fields;
  int32_t* index;
  int32_t  index_stride;
  int32_t* counts;
};
struct ObstCost {
  double   weight;
  double*  cost;
  int32_t* found;  // may be null
  int32_t  kind, accumulate;
};

// (sd, j) orders before (e, m)
__device__ __forceinline__ bool ob_before(double sd, int j, double e, int m) { return sd < e || (sd == e && j < m); }

// One query UAV at p with world label myw: every obstacle of p's cell tested literally, the first KC by (sd, index) left in (ld, lj)
// (unused slots: (inf, INT_MAX)).  Returns the number of obstacles with sd < radius that apply, uncapped.
template <int KC>
__device__ __forceinline__ int obst_search(const ObstArgs& a, const double p[3], uint32_t myw, double (&ld)[KC], int (&lj)[KC]) {
#pragma unroll
  for (int m = 0; m < KC; m++) {
    ld[m] = __builtin_inf();
    lj[m] = 0x7FFFFFFF;
  }
  int found = 0;
  if (a.v.m > 0 && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
    const mrs_obst::GridView& v   = a.v;
    const int64_t             q   = mrs_obst::cell_of(v.g, p[0], p[1], p[2]);  // (inside the grid by the clamp of cell_coord)
    const int                 beg = max(v.start[q], 0), end = min(v.start[q + 1], v.n_items);
    for (int s = beg; s < end; s++) {  // (the steps of mrs_obst::walk_cell, see the head of the file)
      const int j = v.items[s];
      if ((unsigned)j >= (unsigned)v.m) continue;
      const mrs_obstacle_t o = v.obst[j];
      if (!(o.flags & (uint32_t)MRS_OBST_ALL_WORLDS) && (uint32_t)o.world != myw) continue;  // another world's obstacle
      double       rel[3];
      const double sd = mrs_obst::eval(o, p, rel);
      if (!(sd < a.radius)) continue;
      found++;
      if (!ob_before(sd, j, ld[KC - 1], lj[KC - 1])) continue;
      // insertion into the sorted list, from the back (every slot decided from the old values of its own and the one before)
#pragma unroll
      for (int m = KC - 1; m > 0; m--) {
        const bool before_prev = ob_before(sd, j, ld[m - 1], lj[m - 1]);
        const bool before_cur  = ob_before(sd, j, ld[m], lj[m]);
        ld[m] = before_prev ? ld[m - 1] : (before_cur ? sd : ld[m]);
        lj[m] = before_prev ? lj[m - 1] : (before_cur ? j : lj[m]);
      }
      if (ob_before(sd, j, ld[0], lj[0])) {
        ld[0] = sd;
        lj[0] = j;
      }
    }
  }
  return found;
}

// position and world label of query row q
__device__ __forceinline__ int obst_query(const ObstArgs& a, int q, double p[3], uint32_t* myw) {
  const int    i  = a.first + q;
  const size_t np = (size_t)a.npad;
  p[0] = a.S[(size_t)F_X * np + i];
  p[1] = a.S[(size_t)(F_X + 1) * np + i];
  p[2] = a.S[(size_t)(F_X + 2) * np + i];
  *myw = a.wlab ? a.wlab[i] : 0u;
  return i;
}

template <typename T>
__device__ __forceinline__ void put3(T* o, double a, double b, double c) {
  o[0] = (T)a;
  o[1] = (T)b;
  o[2] = (T)c;
}

// slot of obstacle j at signed distance sd from a UAV at p with attitude R, or an empty slot (zeros)
template <typename T>
__device__ __forceinline__ void write_slot(T* o, const ObstArgs& a, bool valid, int j, double sd, const double p[3], const double R[9]) {
  if (!valid) {
    for (int e = 0; e < a.width; e++) o[e] = (T)0;
    return;
  }
  const uint32_t f = a.fields;
  double         rel[3];
  if (f & (MRS_ON_REL | MRS_ON_REL_BODY)) (void)mrs_obst::eval(a.v.obst[j], p, rel);
  if (f & MRS_ON_REL) {
    put3(o, rel[0], rel[1], rel[2]);
    o += 3;
  }
  if (f & MRS_ON_REL_BODY) {
    put3(o, body_velocity(R, rel, 0), body_velocity(R, rel, 1), body_velocity(R, rel, 2));
    o += 3;
  }
  if (f & MRS_ON_DIST) o[0] = (T)sd;
}

// KC: list length (>= k)
template <int KC, typename T>
__global__ void __launch_bounds__(OB_BLOCK) k_obst_rows(ObstArgs a) {
  const int q = blockIdx.x * OB_BLOCK + threadIdx.x;
  if (q >= a.count) return;
  double    p[3];
  uint32_t  myw;
  const int i = obst_query(a, q, p, &myw);
  double    ld[KC];
  int       lj[KC];
  const int found = obst_search<KC>(a, p, myw, ld, lj);
  const int nf    = found < a.k ? found : a.k;
  if (a.counts) a.counts[q] = nf;
  if (a.index) {
    int32_t* o = a.index + (size_t)q * (size_t)a.index_stride;
#pragma unroll
    for (int m = 0; m < KC; m++)
      if (m < a.k) o[m] = m < nf ? lj[m] : -1;
  }
  if (!a.fields) return;
  double R[9];
  if (a.fields & MRS_ON_REL_BODY) {
#pragma unroll
    for (int c = 0; c < 9; c++) R[c] = a.S[(size_t)(F_R + c) * (size_t)a.npad + i];
  }
  T* o = static_cast<T*>(a.rows) + (size_t)q * (size_t)a.stride;
#pragma unroll
  for (int m = 0; m < KC; m++)
    if (m < a.k) write_slot(o + (size_t)m * (size_t)a.width, a, m < nf, lj[m], ld[m], p, R);
}

// term = +0.0, then one separately rounded addition per listed obstacle, nearest first; steps past nf are predicated off and the list is
// indexed statically, so it stays in registers.  `kind` is the same in every lane.
template <int KC>
__global__ void __launch_bounds__(OB_BLOCK) k_obst_cost(ObstArgs a, ObstCost c) {
  const int q = blockIdx.x * OB_BLOCK + threadIdx.x;
  if (q >= a.count) return;
  double   p[3];
  uint32_t myw;
  (void)obst_query(a, q, p, &myw);
  double    ld[KC];
  int       lj[KC];
  const int found = obst_search<KC>(a, p, myw, ld, lj);
  const int nf    = found < a.k ? found : a.k;
  double    term  = 0.0;
  if (c.kind == MRS_PROX_HINGE2) {
#pragma unroll
    for (int m = 0; m < KC; m++) {
      const double g = a.radius - ld[m];
      const double t = term + (c.weight * g) * g;
      term           = m < nf ? t : term;
    }
  } else {
#pragma unroll
    for (int m = 0; m < KC; m++) term = m < nf ? term + c.weight : term;
  }
  double v = 0.0;
  if (c.accumulate) v = c.cost[q];
  c.cost[q] = v + term;
  if (c.found) c.found[q] = found;
}

inline dim3 grid_of(int count) { return dim3((unsigned)((count + OB_BLOCK - 1) / OB_BLOCK)); }

// the list length of the kernels that serve k: launch(integral_constant<int, 8 / 16 / 32>)
template <class Launch>
void for_list_length(int k, Launch&& launch) {
  if (k <= 8)
    launch(std::integral_constant<int, 8>{});
  else if (k <= 16)
    launch(std::integral_constant<int, 16>{});
  else
    launch(std::integral_constant<int, 32>{});
}
template <typename T>
void launch_rows(const ObstArgs& a, hipStream_t st) {
  for_list_length(a.k, [&](auto kc) { hipLaunchKernelGGL((k_obst_rows<decltype(kc)::value, T>), grid_of(a.count), dim3(OB_BLOCK), 0, st, a); });
}
void launch_cost(const ObstArgs& a, const ObstCost& c, hipStream_t st) {
  for_list_length(a.k, [&](auto kc) { hipLaunchKernelGGL((k_obst_cost<decltype(kc)::value>), grid_of(a.count), dim3(OB_BLOCK), 0, st, a, c); });
}

ObstacleSet* set_of(mrs_swarm* s) {
  if (!s->obst) s->obst = new ObstacleSet;
  return s->obst;
}

// replaces the set of s by `count` validated obstacles: host copy, device copy behind everything queued on the swarm's stream
int adopt(mrs_swarm* s, const mrs_obstacle_t* obstacles, int32_t count) {
  ObstacleSet* o = set_of(s);
  HIPCHK(hipStreamSynchronize(s->stream));  // (a query of the old set may still be running)
  std::vector<mrs_obstacle_t> fresh(obstacles, obstacles + count);
  if (count > 0) {
    HIPCHK(o->dev.reserve((size_t)count));
    HIPCHK(hipMemcpyAsync(o->dev, fresh.data(), sizeof(mrs_obstacle_t) * (size_t)count, hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
  }
  o->host.swap(fresh);
  o->query.ok = o->scan.ok = o->contact.ok = o->sight.ok = false;  // (every cached grid served the old set)
  return MRS_OK;
}

// Makes the cache entry c of s's set current for `radius`: built and uploaded on the swarm's stream when the cached grid serves another
// radius or another set.  Called after every argument check and before the entry fence (the upload reads nothing of the caller's).
int ensure(mrs_swarm* s, ObstacleGridCache& c, double radius) {
  ObstacleSet* o = s->obst;
  if (c.ok && c.grid.radius == radius) return MRS_OK;
  mrs_obst::Built b = mrs_obst::build(o->host.data(), (int32_t)o->host.size(), radius);
  HIPCHK(hipStreamSynchronize(s->stream));  // (a kernel may still read the cached grid, and its host vectors may still be uploading)
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

// the queries' grid made current for `radius`, and the search part of `a`
int query_args(mrs_swarm* s, int32_t first, int32_t count, int32_t k, double radius, ObstArgs* out) {
  ObstacleSet* o  = set_of(s);
  int          rc = ensure(s, o->query, radius);
  if (rc) return rc;
  ObstArgs a;
  memset(&a, 0, sizeof a);
  a.S      = s->dS;
  a.wlab   = s->dWorld;
  a.n      = s->n;
  a.npad   = s->npad;
  a.first  = first;
  a.count  = count;
  a.k      = k;
  a.radius = radius;
  a.v      = grid_view(*o, o->query);
  *out     = a;
  return MRS_OK;
}

int check_query(const mrs_swarm* s, int32_t first, int32_t count, int32_t k, double radius, const char* what) {
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, std::string(what) + ": not on a sharded swarm");
  if (k < 1 || k > MRS_OBST_MAX_K) return fail(MRS_ERR_ARG, "k must be in [1, MRS_OBST_MAX_K]");
  if (!(radius > 0.0) || !std::isfinite(radius)) return fail(MRS_ERR_ARG, "radius must be finite and > 0");
  return MRS_OK;
}

}  // namespace

extern "C" void mrs_obstacles_free(ObstacleSet* o) { delete o; }

namespace mrs_host {
// the set of src into dst (mrs_swarm_clone*); dst is idle
int obstacles_copy(mrs_swarm* dst, const mrs_swarm* src) {
  if (!src->obst || src->obst->host.empty()) return MRS_OK;
  return adopt(dst, src->obst->host.data(), (int32_t)src->obst->host.size());
}
// the scans' entry (s->obst->scan) made current for max_range, for the kernels of the two scan units
int scan_grid(mrs_swarm* s, double max_range) { return ensure(s, set_of(s)->scan, max_range); }
// the contacts' entry (s->obst->contact) made current for R, for the kernel of obstacle_contact.hip
int contact_grid(mrs_swarm* s, double R) { return ensure(s, set_of(s)->contact, R); }
// the sight lines' entry (s->obst->sight) made current for radius, for the kernel of nearest_visible.hip
int sight_grid(mrs_swarm* s, double radius) { return ensure(s, set_of(s)->sight, radius); }
}  // namespace mrs_host

extern "C" {

int mrs_swarm_set_obstacles(mrs_swarm_t* s, int32_t count, const mrs_obstacle_t* obstacles) {
  MRS_ENTER_COMMANDS(s);  // (no simulation state is written: a pending collision tick stays pending)
  if (!s) return fail(MRS_ERR_ARG, "null swarm");
  if (count < 0 || count > MRS_OBST_MAX) return fail(MRS_ERR_ARG, "count must be in [0, MRS_OBST_MAX]");
  if (count > 0 && !obstacles) return fail(MRS_ERR_ARG, "null obstacles");
  for (int32_t j = 0; j < count; j++)
    if (const char* why = mrs_obst::invalid(obstacles[j])) return fail(MRS_ERR_ARG, "obstacle " + std::to_string(j) + ": " + why);
  HIPCHK(hipSetDevice(s->device));
  return adopt(s, obstacles, count);
}

int mrs_swarm_get_obstacles(const mrs_swarm_t* s, int32_t capacity, mrs_obstacle_t* out, int32_t* count) {
  MRS_LOCK(s);
  if (!s || !count) return fail(MRS_ERR_ARG, "null argument");
  const size_t m = s->obst ? s->obst->host.size() : 0;
  *count = (int32_t)m;
  if (!out) return MRS_OK;
  if (capacity < (int32_t)m) return fail(MRS_ERR_ARG, "capacity smaller than the set");
  if (m) memcpy(out, s->obst->host.data(), sizeof(mrs_obstacle_t) * m);
  return MRS_OK;
}

int mrs_swarm_obstacle_stats(mrs_swarm_t* s, mrs_obstacle_stats_t* st) {
  MRS_LOCK(s);
  if (!s || !st) return fail(MRS_ERR_ARG, "null argument");
  memset(st, 0, sizeof *st);
  const ObstacleSet* o = s->obst;
  if (!o) return MRS_OK;
  st->count       = (int32_t)o->host.size();
  st->grid_builds = o->builds;
  if (!o->query.ok) return MRS_OK;
  const mrs_obst::Built& b = o->query.grid;  // (the queries' entry: the scans' is not reported)
  for (int a = 0; a < 3; a++) st->dims[a] = b.g.dim[a];
  st->cells        = b.cells();
  st->list_items   = (int64_t)b.items.size();
  st->longest_list = b.longest;
  st->grid_radius  = b.radius;
  st->cell_edge    = b.edge;
  return MRS_OK;
}

int mrs_obstacle_width(uint32_t fields, int32_t k, int32_t* width) {
  if (!width) return fail(MRS_ERR_ARG, "null width");
  if (fields & ~(uint32_t)MRS_ON_ALL) return fail(MRS_ERR_ARG, "unknown obstacle field bits");
  if (k < 1 || k > MRS_OBST_MAX_K) return fail(MRS_ERR_ARG, "k must be in [1, MRS_OBST_MAX_K]");
  int w = 0;
  for (int b = 0; b < 3; b++)
    if (fields & (1u << b)) w += kOnWidth[b];
  *width = k * w;
  return MRS_OK;
}

int mrs_swarm_nearest_obstacles_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t k, double radius, uint32_t fields, void* dev_rows,
                                       int32_t dtype, int32_t stride, int32_t* dev_index, int32_t index_stride, int32_t* dev_count, void* ext_stream) {
  MRS_ENTER_COMMANDS(s);
  int rc = check_query(s, first, count, k, radius, "mrs_swarm_nearest_obstacles_device");
  if (rc) return rc;
  int32_t width = 0;
  if ((rc = mrs_obstacle_width(fields, k, &width))) return rc;
  if (!dev_index && !dev_count && !(fields && dev_rows)) return fail(MRS_ERR_ARG, "no output given (dev_rows with fields, dev_index or dev_count)");
  if (fields) {
    if ((rc = check_dtype(dtype))) return rc;
    if (stride < width) return fail(MRS_ERR_ARG, "stride smaller than k * the width of the selected fields");
  }
  if (dev_index && index_stride < k) return fail(MRS_ERR_ARG, "index_stride smaller than k");
  if (count == 0) return MRS_OK;
  if (fields && (rc = check_device_ptr(s, dev_rows, rows_bytes(count, stride, width, dtype), "dev_rows"))) return rc;
  if (dev_index && (rc = check_device_ptr(s, dev_index, index_rows_bytes(count, index_stride, k), "dev_index")))
    return rc;
  if (dev_count && (rc = check_device_ptr(s, dev_count, index_rows_bytes(count, 1, 1), "dev_count"))) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  ObstArgs    a;
  if ((rc = query_args(s, first, count, k, radius, &a))) return rc;
  if ((rc = fence_in(s, ext))) return rc;
  a.fields       = dev_rows ? fields : 0u;
  a.rows         = dev_rows;
  a.stride       = stride;
  a.width        = fields ? width / k : 0;
  a.index        = dev_index;
  a.index_stride = index_stride;
  a.counts       = dev_count;
  if (dtype == MRS_DTYPE_F32)
    launch_rows<float>(a, s->stream);
  else
    launch_rows<double>(a, s->stream);
  HIPCHK(hipGetLastError());
  return fence_out(s, ext);
}

int mrs_swarm_obstacle_cost_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t k, double radius, int32_t kind, double weight,
                                   double* dev_cost, int32_t accumulate, int32_t* dev_found, void* ext_stream) {
  MRS_ENTER_COMMANDS(s);
  int rc = check_query(s, first, count, k, radius, "mrs_swarm_obstacle_cost_device");
  if (rc) return rc;
  if (kind == MRS_PROX_INVERSE) return fail(MRS_ERR_ARG, "MRS_PROX_INVERSE is not an obstacle cost kind");
  if (kind != MRS_PROX_HINGE2 && kind != MRS_PROX_COUNT) return fail(MRS_ERR_ARG, "unknown obstacle cost kind");
  if (!dev_cost) return fail(MRS_ERR_ARG, "dev_cost: null pointer");
  if (count == 0) return MRS_OK;
  if ((rc = check_device_ptr(s, dev_cost, (size_t)count * sizeof(double), "dev_cost"))) return rc;
  if (dev_found && (rc = check_device_ptr(s, dev_found, index_rows_bytes(count, 1, 1), "dev_found"))) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  ObstArgs    a;
  if ((rc = query_args(s, first, count, k, radius, &a))) return rc;
  if ((rc = fence_in(s, ext))) return rc;
  ObstCost c;
  c.weight     = weight;
  c.cost       = dev_cost;
  c.found      = dev_found;
  c.kind       = kind;
  c.accumulate = accumulate ? 1 : 0;
  launch_cost(a, c, s->stream);
  HIPCHK(hipGetLastError());
  return fence_out(s, ext);
}

}  // extern "C"
