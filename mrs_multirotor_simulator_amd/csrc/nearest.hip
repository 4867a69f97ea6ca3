// nearest.hip — k-nearest-neighbour observations for device-resident callers (include/mrs_swarm.h, "nearest-neighbour observations"):
// for each query UAV i, the k UAVs j != i with the smallest (d2, j), d2 = ((dx*dx) + dy*dy) + dz*dz < radius^2, and per listed neighbour
// the relative position / velocity (world or body frame) and the distance, written into caller-owned device rows.
//
// Not the collision pass's hash (collide.hip): its cells, table entries and quantised in-cell coordinates are built for one fixed radius,
// and its tables and neighbour lists are state of the fused step.  This unit has its own scratch and four kernels per call:
//   bin     one lane per UAV: cell = floor(x / edge) with edge = radius (1 + 1e-6), clamped to +-2^30; bucket = hash(cell) & (T-1),
//           T = a power of two >= 2n; atomicAdd on the bucket count, the returned value is the UAV's rank in its bucket.  UAVs with a
//           non-finite position go to the extra bucket T, which no query probes.
//   scan    the T + 1 counts into bucket starts: exclusive scan of 2048-entry chunks (one block each), then one block scans the chunk
//           totals; the scatter and the query add the two levels on the fly.
//   scatter each UAV's compact record (position, index: 32 B) into slot start[bucket] + rank: every bucket is a contiguous range.
//   query   one lane per query UAV: the 27 cells around its own, their buckets deduplicated (two cells can hash to one bucket, which
//           must not be read twice), every record of those ranges tested literally; a per-lane top-KC list in registers by (d2, j);
//           then the k slots of the row, relative quantities from the state columns of i and the listed j.
// Collision worlds (mrs_swarm_set_worlds): once a label has been set, the world-aware instantiations of bin, scatter and query run instead
// (the same templates with the label column as one more argument).  A mixed image of the label enters the bucket hash on the bin side and the probe side alike (the
// copies of a forked scene spread over the table instead of sharing every bucket), the sorted record carries the label in its spare
// word, and a candidate enters the top-k list only after its label has been compared with the query UAV's exactly.
// The proximity cost (mrs_swarm_proximity_cost_device) is the same build and the same search with a reduction instead of the row: k_nn_proximity.
// Lanes walk either the query range in index order or the sorted records (all n slots, those outside the range return at once): the
// second reads neighbouring cells across a wave (MRS_NN_ORDER).  The result depends on neither: it is defined by (d2, j).
#include <stdlib.h>
#include <string.h>

#include "host_internal.h"
#include "nn_hash.h"
#include "nn_slot.h"
#include "pose_math.h"

namespace {

// the record, the cell coordinate, the bucket hash and the bucket starts: nn_hash.h (range_scan_uavs.hip probes the same hash);
// the argument block NnArgs and the slot text put3 / write_slot: nn_slot.h (nearest_visible.hip writes the same rows)
using namespace mrs_nn;

constexpr int    NN_BLOCK   = 256;
constexpr int    SCAN_PER   = 8;                      // counts per lane of the chunk scan
constexpr int    SCAN_CH    = NN_BLOCK * SCAN_PER;    // 2048 counts per chunk (1 << SCAN_LOG)
static_assert(SCAN_CH == 1 << SCAN_LOG, "bucket_begin adds the chunk total of bucket b >> SCAN_LOG");
constexpr int    kNnWidth[5] = {3, 3, 3, 3, 1};

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// bucket and rank of every UAV (bucket tmask + 1: non-finite position)
// (W: empty, or the label column, const uint32_t*)
template <class... W>
__global__ void __launch_bounds__(NN_BLOCK) k_nn_bin(const double* S, int n, int npad, double inv_edge, uint32_t tmask, int32_t* cnt, int32_t* rank,
                                                     int32_t* bkt, W... labels) {
  constexpr bool WORLDS = sizeof...(W) != 0;
  const int i = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const size_t np = (size_t)npad;
  const double x = S[(size_t)F_X * np + i], y = S[(size_t)(F_X + 1) * np + i], z = S[(size_t)(F_X + 2) * np + i];
  uint32_t wm = 0u;
  if constexpr (WORLDS) wm = world_mix(world_labels(labels...)[i]);
  const uint32_t b = finite3(x, y, z) ? bucket_of_x<WORLDS>(cell_coord(x, inv_edge), cell_coord(y, inv_edge), cell_coord(z, inv_edge), tmask, wm) : tmask + 1;
  rank[i] = atomicAdd(&cnt[b], 1);
  bkt[i]  = (int32_t)b;
}
// exclusive scan of the 256 lane values of a block; returns the block total in every lane
__device__ __forceinline__ int block_exclusive_scan(int v, int* excl) {
  __shared__ int wsum[NN_BLOCK / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < NN_BLOCK / 64; w++) {
    const int t = wsum[w];
    before += w < wave ? t : 0;
    total += t;
  }
  __syncthreads();  // (wsum is reused by the next call)
  *excl = before + inc - v;
  return total;
}

// chunk b: start[] = exclusive scan of cnt[] within the chunk, bsum[b] = the chunk's total
__global__ void __launch_bounds__(NN_BLOCK) k_nn_scan_chunks(const int32_t* cnt, int32_t* start, int32_t* bsum) {
  const size_t base = (size_t)blockIdx.x * SCAN_CH + (size_t)threadIdx.x * SCAN_PER;
  const int4   a = *reinterpret_cast<const int4*>(cnt + base);
  const int4   b = *reinterpret_cast<const int4*>(cnt + base + 4);
  const int    v[SCAN_PER] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  int          sum = 0;
#pragma unroll
  for (int e = 0; e < SCAN_PER; e++) sum += v[e];
  int       excl;
  const int total = block_exclusive_scan(sum, &excl);
  int       o[SCAN_PER];
#pragma unroll
  for (int e = 0; e < SCAN_PER; e++) {
    o[e] = excl;
    excl += v[e];
  }
  *reinterpret_cast<int4*>(start + base)     = make_int4(o[0], o[1], o[2], o[3]);
  *reinterpret_cast<int4*>(start + base + 4) = make_int4(o[4], o[5], o[6], o[7]);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: the chunk totals into their exclusive prefix, in place, 256 at a time
__global__ void __launch_bounds__(NN_BLOCK) k_nn_scan_top(int32_t* bsum, int nchunks) {
  int carry = 0;
  for (int base = 0; base < nchunks; base += NN_BLOCK) {
    const int c = base + (int)threadIdx.x;
    const int v = c < nchunks ? bsum[c] : 0;
    int       excl;
    const int total = block_exclusive_scan(v, &excl);
    if (c < nchunks) bsum[c] = carry + excl;
    carry += total;
  }
}

template <class... W>
__global__ void __launch_bounds__(NN_BLOCK) k_nn_scatter(const double* S, int n, int npad, const int32_t* rank, const int32_t* bkt,
                                                         const int32_t* start, const int32_t* bsum, NnRec* rec, W... labels) {
  constexpr bool WORLDS = sizeof...(W) != 0;
  const int i = blockIdx.x * NN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const size_t np = (size_t)npad;
  NnRec r;
  r.x   = S[(size_t)F_X * np + i];
  r.y   = S[(size_t)(F_X + 1) * np + i];
  r.z   = S[(size_t)(F_X + 2) * np + i];
  r.idx = i;
  r.pad = 0;
  if constexpr (WORLDS) r.pad = (int32_t)world_labels(labels...)[i];
  const int slot = bucket_begin(start, bsum, (uint32_t)bkt[i]) + rank[i];
  if ((unsigned)slot < (unsigned)n) rec[slot] = r;  // (always: the slots are a permutation of [0, n))
}
// (d2, j) orders before (e2, m)
__device__ __forceinline__ bool nn_before(double d2, int j, double e2, int m) { return d2 < e2 || (d2 == e2 && j < m); }

// The search of k_nn_query once more, for k_nn_proximity.  k_nn_query keeps its own text: with this function inlined into it, hipcc
// schedules it differently and nearest(NN_DIST, FP64) at 100 000 UAVs measured about 1 % slower than the parent's build, so the loop has
// two definitions that must stay equal; tests/test_proximity_cost_gpu.py and tests/test_nearest_gpu.py hold both to the same numpy search.
// One query UAV i at (xi, yi, zi): the 27 deduplicated probes, every record of their buckets tested literally, the first KC
// neighbours by (d2, j) left in (ld, lj) (unused slots: (inf, INT_MAX)).  Returns the number of neighbours, uncapped.  WORLDS: only UAVs
// that carry the query UAV's label myw are candidates (the records carry the labels).
template <int KC, bool WORLDS>
__device__ __forceinline__ int nn_probe(const NnArgs& a, int i, double xi, double yi, double zi, int32_t myw, double (&ld)[KC], int (&lj)[KC]) {
  uint32_t wm = 0u;
  if constexpr (WORLDS) wm = world_mix((uint32_t)myw);
#pragma unroll
  for (int m = 0; m < KC; m++) {
    ld[m] = __builtin_inf();
    lj[m] = 0x7FFFFFFF;
  }
  int found = 0;
  if (finite3(xi, yi, zi)) {
    const int cx = cell_coord(xi, a.inv_edge), cy = cell_coord(yi, a.inv_edge), cz = cell_coord(zi, a.inv_edge);
    // the 27 buckets; bit p of `dup`: probe p hits a bucket an earlier probe reads already
    uint32_t bk[27];
#pragma unroll
    for (int p = 0; p < 27; p++) bk[p] = bucket_of_x<WORLDS>(cx + p % 3 - 1, cy + (p / 3) % 3 - 1, cz + p / 9 - 1, a.tmask, wm);
    uint32_t dup = 0;
#pragma unroll
    for (int p = 1; p < 27; p++) {
      bool d = false;
#pragma unroll
      for (int o = 0; o < p; o++) d = d || bk[o] == bk[p];
      dup |= d ? 1u << p : 0u;
    }
    for (int p = 0; p < 27; p++) {
      if (dup & (1u << p)) continue;
      const uint32_t b   = bucket_of_x<WORLDS>(cx + p % 3 - 1, cy + (p / 3) % 3 - 1, cz + p / 9 - 1, a.tmask, wm);
      const int      beg = bucket_begin(a.start, a.bsum, b), end = min(beg + a.cnt[b], a.n);
      for (int s = beg; s < end; s++) {
        const NnRec  r  = a.rec[s];
        const double dx = r.x - xi, dy = r.y - yi, dz = r.z - zi;
        const double d2 = ((dx * dx) + dy * dy) + dz * dz;
        const int    j  = r.idx;
        if (!(d2 < a.rr) || j == i || (unsigned)j >= (unsigned)a.n) continue;
        if (WORLDS && r.pad != myw) continue;  // another world: never a neighbour, however close
        found++;
        if (!nn_before(d2, j, ld[KC - 1], lj[KC - 1])) continue;
        // insertion into the sorted list, from the back (every slot decided from the old values of its own and the one before)
#pragma unroll
        for (int m = KC - 1; m > 0; m--) {
          const bool before_prev = nn_before(d2, j, ld[m - 1], lj[m - 1]);
          const bool before_cur  = nn_before(d2, j, ld[m], lj[m]);
          ld[m] = before_prev ? ld[m - 1] : (before_cur ? d2 : ld[m]);
          lj[m] = before_prev ? lj[m - 1] : (before_cur ? j : lj[m]);
        }
        if (nn_before(d2, j, ld[0], lj[0])) {
          ld[0] = d2;
          lj[0] = j;
        }
      }
    }
  }
  return found;
}

// KC: list length (>= k); SORTED: lanes walk the sorted records instead of the query range; WORLDS: only UAVs that carry the query
// UAV's label are candidates (wlab = the label column; the records carry the labels too)
template <int KC, typename T, bool SORTED, class... W>
__global__ void __launch_bounds__(NN_BLOCK) k_nn_query(NnArgs a, W... labels) {
  constexpr bool  WORLDS = sizeof...(W) != 0;
  const uint32_t* wlab   = world_labels(labels...);
  const int    q  = blockIdx.x * NN_BLOCK + threadIdx.x;
  const size_t np = (size_t)a.npad;
  int          i;
  double       xi, yi, zi;
  int32_t      myw = 0;  // (the query UAV's label; unused without labels)
  if (SORTED) {
    if (q >= a.n) return;
    const NnRec r = a.rec[q];
    i             = r.idx;
    if (i < a.first || i >= a.first + a.count) return;
    xi = r.x;
    yi = r.y;
    zi = r.z;
    if constexpr (WORLDS) myw = r.pad;
  } else {
    if (q >= a.count) return;
    i  = a.first + q;
    xi = a.S[(size_t)F_X * np + i];
    yi = a.S[(size_t)(F_X + 1) * np + i];
    zi = a.S[(size_t)(F_X + 2) * np + i];
    if constexpr (WORLDS) myw = (int32_t)wlab[i];
  }
  const int row = i - a.first;
  uint32_t  wm  = 0u;
  if constexpr (WORLDS) wm = world_mix((uint32_t)myw);

  double ld[KC];
  int    lj[KC];
#pragma unroll
  for (int m = 0; m < KC; m++) {
    ld[m] = __builtin_inf();
    lj[m] = 0x7FFFFFFF;
  }
  int found = 0;
  if (finite3(xi, yi, zi)) {
    const int cx = cell_coord(xi, a.inv_edge), cy = cell_coord(yi, a.inv_edge), cz = cell_coord(zi, a.inv_edge);
    // the 27 buckets; bit p of `dup`: probe p hits a bucket an earlier probe reads already
    uint32_t bk[27];
#pragma unroll
    for (int p = 0; p < 27; p++) bk[p] = bucket_of_x<WORLDS>(cx + p % 3 - 1, cy + (p / 3) % 3 - 1, cz + p / 9 - 1, a.tmask, wm);
    uint32_t dup = 0;
#pragma unroll
    for (int p = 1; p < 27; p++) {
      bool d = false;
#pragma unroll
      for (int o = 0; o < p; o++) d = d || bk[o] == bk[p];
      dup |= d ? 1u << p : 0u;
    }
    for (int p = 0; p < 27; p++) {
      if (dup & (1u << p)) continue;
      const uint32_t b   = bucket_of_x<WORLDS>(cx + p % 3 - 1, cy + (p / 3) % 3 - 1, cz + p / 9 - 1, a.tmask, wm);
      const int      beg = bucket_begin(a.start, a.bsum, b), end = min(beg + a.cnt[b], a.n);
      for (int s = beg; s < end; s++) {
        const NnRec  r  = a.rec[s];
        const double dx = r.x - xi, dy = r.y - yi, dz = r.z - zi;
        const double d2 = ((dx * dx) + dy * dy) + dz * dz;
        const int    j  = r.idx;
        if (!(d2 < a.rr) || j == i || (unsigned)j >= (unsigned)a.n) continue;
        if (WORLDS && r.pad != myw) continue;  // another world: never a neighbour, however close
        found++;
        if (!nn_before(d2, j, ld[KC - 1], lj[KC - 1])) continue;
        // insertion into the sorted list, from the back (every slot decided from the old values of its own and the one before)
#pragma unroll
        for (int m = KC - 1; m > 0; m--) {
          const bool before_prev = nn_before(d2, j, ld[m - 1], lj[m - 1]);
          const bool before_cur  = nn_before(d2, j, ld[m], lj[m]);
          ld[m] = before_prev ? ld[m - 1] : (before_cur ? d2 : ld[m]);
          lj[m] = before_prev ? lj[m - 1] : (before_cur ? j : lj[m]);
        }
        if (nn_before(d2, j, ld[0], lj[0])) {
          ld[0] = d2;
          lj[0] = j;
        }
      }
    }
  }
  const int nf = found < a.k ? found : a.k;
  if (a.counts) a.counts[row] = nf;
  if (a.index) {
    int32_t* o = a.index + (size_t)row * (size_t)a.index_stride;
#pragma unroll
    for (int m = 0; m < KC; m++)
      if (m < a.k) o[m] = m < nf ? lj[m] : -1;
  }
  if (!a.fields) return;
  const uint32_t f    = a.fields;
  const bool     body = f & (MRS_NN_REL_POS_BODY | MRS_NN_REL_VEL_BODY);
  const bool     vel  = f & (MRS_NN_REL_VEL | MRS_NN_REL_VEL_BODY);
  double         R[9], vi[3];
  if (body) {
#pragma unroll
    for (int c = 0; c < 9; c++) R[c] = a.S[(size_t)(F_R + c) * np + i];
  }
  if (vel) {
#pragma unroll
    for (int c = 0; c < 3; c++) vi[c] = a.S[(size_t)(F_V + c) * np + i];
  }
  const double xs[3] = {xi, yi, zi};
  T*           o     = static_cast<T*>(a.rows) + (size_t)row * (size_t)a.stride;
#pragma unroll
  for (int m = 0; m < KC; m++)
    if (m < a.k) write_slot(o + (size_t)m * (size_t)a.width, a, m < nf, lj[m], ld[m], xs, vi, R);
}
inline dim3 grid_of(int count) { return dim3((unsigned)((count + NN_BLOCK - 1) / NN_BLOCK)); }

template <int KC, typename T>
void launch_query(const NnArgs& a, bool sorted, hipStream_t st, const uint32_t* wlab) {
  if (wlab) {
    if (sorted)
      hipLaunchKernelGGL((k_nn_query<KC, T, true, const uint32_t*>), grid_of(a.n), dim3(NN_BLOCK), 0, st, a, wlab);
    else
      hipLaunchKernelGGL((k_nn_query<KC, T, false, const uint32_t*>), grid_of(a.count), dim3(NN_BLOCK), 0, st, a, wlab);
    return;
  }
  if (sorted)
    hipLaunchKernelGGL((k_nn_query<KC, T, true>), grid_of(a.n), dim3(NN_BLOCK), 0, st, a);
  else
    hipLaunchKernelGGL((k_nn_query<KC, T, false>), grid_of(a.count), dim3(NN_BLOCK), 0, st, a);
}

template <typename T>
void launch_query_k(const NnArgs& a, bool sorted, hipStream_t st, const uint32_t* wlab) {
  if (a.k <= 8)
    launch_query<8, T>(a, sorted, st, wlab);
  else if (a.k <= 16)
    launch_query<16, T>(a, sorted, st, wlab);
  else
    launch_query<32, T>(a, sorted, st, wlab);
}

// ---- proximity cost (mrs_swarm_proximity_cost_device): the search of k_nn_query, then one FP64 number per UAV instead of a row ----
struct ProxArgs {
  double   radius, weight, eps;
  double*  cost;
  int32_t* found;  // may be null
  int32_t  kind, accumulate;
};

// term = +0.0, then one separately rounded addition per listed neighbour, nearest first; steps past nf are predicated off and the list
// is indexed statically, so it stays in registers.  `kind` is the same in every lane.
template <int KC>
__device__ __forceinline__ double prox_term(const ProxArgs& p, const double (&ld)[KC], int nf) {
  double term = 0.0;
  if (p.kind == MRS_PROX_HINGE2) {
#pragma unroll
    for (int m = 0; m < KC; m++) {
      const double g = p.radius - sqrt(ld[m]);
      const double t = term + (p.weight * g) * g;
      term           = m < nf ? t : term;
    }
  } else if (p.kind == MRS_PROX_INVERSE) {
#pragma unroll
    for (int m = 0; m < KC; m++) {
      const double t = term + p.weight / (ld[m] + p.eps);
      term           = m < nf ? t : term;
    }
  } else {
#pragma unroll
    for (int m = 0; m < KC; m++) term = m < nf ? term + p.weight : term;
  }
  return term;
}

template <int KC, bool SORTED, class... W>
__global__ void __launch_bounds__(NN_BLOCK) k_nn_proximity(NnArgs a, ProxArgs p, W... labels) {
  constexpr bool  WORLDS = sizeof...(W) != 0;
  const uint32_t* wlab   = world_labels(labels...);
  const int    q  = blockIdx.x * NN_BLOCK + threadIdx.x;
  const size_t np = (size_t)a.npad;
  int          i;
  double       xi, yi, zi;
  int32_t      myw = 0;  // (the query UAV's label; unused without labels)
  if (SORTED) {
    if (q >= a.n) return;
    const NnRec r = a.rec[q];
    i             = r.idx;
    if (i < a.first || i >= a.first + a.count) return;
    xi = r.x;
    yi = r.y;
    zi = r.z;
    if constexpr (WORLDS) myw = r.pad;
  } else {
    if (q >= a.count) return;
    i  = a.first + q;
    xi = a.S[(size_t)F_X * np + i];
    yi = a.S[(size_t)(F_X + 1) * np + i];
    zi = a.S[(size_t)(F_X + 2) * np + i];
    if constexpr (WORLDS) myw = (int32_t)wlab[i];
  }
  const int row = i - a.first;
  double    ld[KC];
  int       lj[KC];
  const int found = nn_probe<KC, WORLDS>(a, i, xi, yi, zi, myw, ld, lj);
  const int nf    = found < a.k ? found : a.k;
  double    c     = 0.0;
  if (p.accumulate) c = p.cost[row];
  p.cost[row] = c + prox_term<KC>(p, ld, nf);
  if (p.found) p.found[row] = found;
}

template <int KC>
void launch_proximity(const NnArgs& a, const ProxArgs& p, bool sorted, hipStream_t st, const uint32_t* wlab) {
  if (wlab) {
    if (sorted)
      hipLaunchKernelGGL((k_nn_proximity<KC, true, const uint32_t*>), grid_of(a.n), dim3(NN_BLOCK), 0, st, a, p, wlab);
    else
      hipLaunchKernelGGL((k_nn_proximity<KC, false, const uint32_t*>), grid_of(a.count), dim3(NN_BLOCK), 0, st, a, p, wlab);
    return;
  }
  if (sorted)
    hipLaunchKernelGGL((k_nn_proximity<KC, true>), grid_of(a.n), dim3(NN_BLOCK), 0, st, a, p);
  else
    hipLaunchKernelGGL((k_nn_proximity<KC, false>), grid_of(a.count), dim3(NN_BLOCK), 0, st, a, p);
}

void launch_proximity_k(const NnArgs& a, const ProxArgs& p, bool sorted, hipStream_t st, const uint32_t* wlab) {
  if (a.k <= 8)
    launch_proximity<8>(a, p, sorted, st, wlab);
  else if (a.k <= 16)
    launch_proximity<16>(a, p, sorted, st, wlab);
  else
    launch_proximity<32>(a, p, sorted, st, wlab);
}

// lane order of the query: MRS_NN_ORDER=index / sorted; default (auto): sorted records when the query range covers at least a quarter
// of the swarm (a lane per record of a UAV outside the range only returns)
int nn_order() {
  static const int o = [] {
    const char* e = getenv("MRS_NN_ORDER");
    if (e && !strcmp(e, "index")) return 0;
    if (e && !strcmp(e, "sorted")) return 1;
    return -1;
  }();
  return o;
}

// The hash of one call, built on the swarm's stream behind the entry fence: the scratch layout in nn_buf, memset, bin, the two scans and
// scatter.  Fills the search part of `a` (everything but the outputs of a query kernel); radius * radius is rounded here, once.
int nn_build_hash(mrs_swarm* s, int32_t first, int32_t count, int32_t k, double radius, hipStream_t ext, NnArgs* out) {
  // scratch: records (n), rank (n), bucket (n), counts and starts (T + 1 padded to whole chunks), chunk totals
  const int n = s->n;
  uint32_t  T = 2;
  while (T < 2u * (uint32_t)n) T <<= 1;
  const int    nchunks  = (int)((T + 1 + SCAN_CH - 1) / SCAN_CH);
  const size_t ncnt     = (size_t)nchunks * SCAN_CH;
  const size_t off_rank = sizeof(NnRec) * (size_t)n;
  const size_t off_bkt  = off_rank + sizeof(int32_t) * (size_t)n;
  const size_t off_cnt  = (off_bkt + sizeof(int32_t) * (size_t)n + 15) & ~(size_t)15;
  const size_t off_st   = off_cnt + sizeof(int32_t) * ncnt;
  const size_t off_bs   = off_st + sizeof(int32_t) * ncnt;
  const size_t bytes    = off_bs + sizeof(int32_t) * (size_t)nchunks;
  HIPCHK(s->nn_buf.reserve(bytes));  // (every launch that reads the block is on the swarm's stream; hipFree waits for the device)
  char*    base  = static_cast<char*>(s->nn_buf.get());
  NnRec*   rec   = reinterpret_cast<NnRec*>(base);
  int32_t* rank  = reinterpret_cast<int32_t*>(base + off_rank);
  int32_t* bkt   = reinterpret_cast<int32_t*>(base + off_bkt);
  int32_t* cnt   = reinterpret_cast<int32_t*>(base + off_cnt);
  int32_t* start = reinterpret_cast<int32_t*>(base + off_st);
  int32_t* bsum  = reinterpret_cast<int32_t*>(base + off_bs);

  int rc = fence_in(s, ext);
  if (rc) return rc;
  const double inv_edge = 1.0 / (radius * (1.0 + CELL_MARGIN));
  HIPCHK(hipMemsetAsync(cnt, 0, sizeof(int32_t) * ncnt, s->stream));
  const uint32_t* wlab = s->dWorld;
  if (wlab)
    hipLaunchKernelGGL((k_nn_bin<const uint32_t*>), grid_of(n), dim3(NN_BLOCK), 0, s->stream, s->dS, n, s->npad, inv_edge, T - 1, cnt, rank, bkt, wlab);
  else
    hipLaunchKernelGGL((k_nn_bin<>), grid_of(n), dim3(NN_BLOCK), 0, s->stream, s->dS, n, s->npad, inv_edge, T - 1, cnt, rank, bkt);
  hipLaunchKernelGGL(k_nn_scan_chunks, dim3((unsigned)nchunks), dim3(NN_BLOCK), 0, s->stream, cnt, start, bsum);
  hipLaunchKernelGGL(k_nn_scan_top, dim3(1), dim3(NN_BLOCK), 0, s->stream, bsum, nchunks);
  if (wlab)
    hipLaunchKernelGGL((k_nn_scatter<const uint32_t*>), grid_of(n), dim3(NN_BLOCK), 0, s->stream, s->dS, n, s->npad, rank, bkt, start, bsum, rec, wlab);
  else
    hipLaunchKernelGGL((k_nn_scatter<>), grid_of(n), dim3(NN_BLOCK), 0, s->stream, s->dS, n, s->npad, rank, bkt, start, bsum, rec);
  NnArgs a;
  memset(&a, 0, sizeof a);
  a.S = s->dS;
  a.n = n;
  a.npad = s->npad;
  a.first = first;
  a.count = count;
  a.k = k;
  a.inv_edge = inv_edge;
  a.rr = radius * radius;
  a.tmask = T - 1;
  a.cnt = cnt;
  a.start = start;
  a.bsum = bsum;
  a.rec = rec;
  *out = a;
  return MRS_OK;
}

// sorted records when the query range covers at least a quarter of the swarm, unless MRS_NN_ORDER says otherwise
bool nn_sorted(const mrs_swarm* s, int32_t count) { return nn_order() >= 0 ? nn_order() == 1 : 4LL * count >= s->n; }

}  // namespace

namespace mrs_host {
// the hash of the swarm's positions for `radius`, for a kernel of another unit (range_scan_uavs.hip): nn_build_hash as it is — the entry
// fence, the scratch in nn_buf, the four launches on the swarm's stream — and what a probe needs of it
int nn_hash(mrs_swarm* s, double radius, hipStream_t ext, mrs_nn::NnHash* out) {
  NnArgs a;
  int    rc = nn_build_hash(s, 0, s->n, 1, radius, ext, &a);
  if (rc) return rc;
  out->rec      = a.rec;
  out->cnt      = a.cnt;
  out->start    = a.start;
  out->bsum     = a.bsum;
  out->inv_edge = a.inv_edge;
  out->tmask    = a.tmask;
  out->n        = a.n;
  return MRS_OK;
}
}  // namespace mrs_host

extern "C" {

int mrs_nearest_width(uint32_t fields, int32_t k, int32_t* width) {
  if (!width) return fail(MRS_ERR_ARG, "null width");
  if (fields & ~(uint32_t)MRS_NN_ALL) return fail(MRS_ERR_ARG, "unknown neighbour field bits");
  if (k < 1 || k > MRS_NN_MAX_K) return fail(MRS_ERR_ARG, "k must be in [1, MRS_NN_MAX_K]");
  int w = 0;
  for (int b = 0; b < 5; b++)
    if (fields & (1u << b)) w += kNnWidth[b];
  *width = k * w;
  return MRS_OK;
}

int mrs_swarm_nearest_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t k, double radius, uint32_t fields, void* dev_rows, int32_t dtype,
                             int32_t stride, int32_t* dev_index, int32_t index_stride, int32_t* dev_count, void* ext_stream) {
  MRS_ENTER_COMMANDS(s);
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, "mrs_swarm_nearest_device: not on a sharded swarm");
  int32_t width = 0;
  if ((rc = mrs_nearest_width(fields, k, &width))) return rc;
  if (!(radius > 0.0) || !std::isfinite(radius)) return fail(MRS_ERR_ARG, "radius must be finite and > 0");
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
  NnArgs      a;
  if ((rc = nn_build_hash(s, first, count, k, radius, ext, &a))) return rc;
  a.fields = dev_rows ? fields : 0u;
  a.rows = dev_rows;
  a.stride = stride;
  a.width = fields ? width / k : 0;
  a.index = dev_index;
  a.index_stride = index_stride;
  a.counts = dev_count;
  const uint32_t* wlab = s->dWorld;  // null: no label was ever set — the kernels without them
  const bool sorted = nn_sorted(s, count);
  if (dtype == MRS_DTYPE_F32)
    launch_query_k<float>(a, sorted, s->stream, wlab);
  else
    launch_query_k<double>(a, sorted, s->stream, wlab);
  HIPCHK(hipGetLastError());
  return fence_out(s, ext);
}

int mrs_swarm_proximity_cost_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t k, double radius, int32_t kind, double weight, double eps,
                                    double* dev_cost, int32_t accumulate, int32_t* dev_found, void* ext_stream) {
  MRS_ENTER_COMMANDS(s);
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, "mrs_swarm_proximity_cost_device: not on a sharded swarm");
  if (k < 1 || k > MRS_NN_MAX_K) return fail(MRS_ERR_ARG, "k must be in [1, MRS_NN_MAX_K]");
  if (!(radius > 0.0) || !std::isfinite(radius)) return fail(MRS_ERR_ARG, "radius must be finite and > 0");
  if (kind != MRS_PROX_HINGE2 && kind != MRS_PROX_INVERSE && kind != MRS_PROX_COUNT) return fail(MRS_ERR_ARG, "unknown proximity kind");
  if (kind == MRS_PROX_INVERSE && (!std::isfinite(eps) || eps < 0.0)) return fail(MRS_ERR_ARG, "eps must be finite and >= 0 (MRS_PROX_INVERSE)");
  if (!dev_cost) return fail(MRS_ERR_ARG, "dev_cost: null pointer");
  if (count == 0) return MRS_OK;
  if ((rc = check_device_ptr(s, dev_cost, (size_t)count * sizeof(double), "dev_cost"))) return rc;
  if (dev_found && (rc = check_device_ptr(s, dev_found, index_rows_bytes(count, 1, 1), "dev_found"))) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  NnArgs      a;
  if ((rc = nn_build_hash(s, first, count, k, radius, ext, &a))) return rc;
  ProxArgs p;
  p.radius = radius;
  p.weight = weight;
  p.eps = eps;
  p.cost = dev_cost;
  p.found = dev_found;
  p.kind = kind;
  p.accumulate = accumulate ? 1 : 0;
  launch_proximity_k(a, p, nn_sorted(s, count), s->stream, s->dWorld);
  HIPCHK(hipGetLastError());
  return fence_out(s, ext);
}

}  // extern "C"
