// nearest_visible.hip — line-of-sight neighbours (include/mrs_swarm.h, "line-of-sight neighbours"): the rows of nearest.hip, but a
// candidate that a static obstacle hides from the observer is not a neighbour: the first k VISIBLE candidates by (d2, j), and per
// observer how many candidates it sees and how many are hidden.  The join of three things that exist: the per-call hash of UAV positions
// that nearest.hip builds (nn_hash.h), the cell walk over the cached obstacle grid (mrs_obst::walk_cell; the set's `sight` entry, built
// for the call's radius) and the closed-solid ray test of the scans (mrs_scan::gate, mrs_scan::ray, through mrs_sight::hides).
// One 64-lane block (one wave) per observer.  The 27 buckets around the observer's cell are formed from the observer alone and
// de-duplicated as k_nn_query does (a count, unlike the minimum of k_range_scan_uavs, is not idempotent).  The records of a bucket are
// taken 64 at a time across the lanes; a lane whose record is a candidate forms the sight line and walks the observer's ONE obstacle cell
// (the same cell in every lane: the loads are wave-uniform).  Visible lanes append (d2, j) to a list in LDS at positions from a ballot and
// a prefix count; when the list cannot take the next group it is reduced in place to its first k entries, by rank: an entry's rank is the
// number of entries that order before it ((d2, j) are distinct, so the ranks are a permutation).  The same ranking decides at the end
// which lane writes which slot.  The slot text is nn_slot.h's, the very functions k_nn_query calls.
// Nothing here writes simulation state; entry, fence and scratch are those of nearest (the swarm's nn_buf) plus the cached grid.
#include "nn_hash.h"
#include "nn_slot.h"
#include "obstacle_set.h"
#include "sight_math.h"

namespace {

using namespace mrs_nn;

constexpr int NV_WAVE = 64;            // lanes of a block: one wave, so every barrier below is reached by all of its lanes or by none
constexpr int NV_CAP  = 256;           // entries of the visible list in LDS (tests/test_nearest_visible_gpu.py names this value): 3 KiB per block
constexpr int NV_PER  = NV_CAP / NV_WAVE;  // list entries a lane ranks
static_assert(MRS_NN_MAX_K + NV_WAVE <= NV_CAP, "a reduced list must take one more group of records");
static_assert(MRS_NN_MAX_K <= NV_WAVE, "lane m writes empty slot m");

struct VisArgs {
  NnArgs             a;  // the hash, the query range and the rows, as k_nn_query takes them
  mrs_obst::GridView v;  // the set through the sight lines' grid (built for radius)
  double             radius;
  int32_t *          visible, *hidden;  // each may be null
};

__device__ __forceinline__ double uniform(double x) {  // the first lane's value as a scalar (x is the same in every lane)
  const long long b = __double_as_longlong(x);
  const int       lo = __builtin_amdgcn_readfirstlane((int)(b & 0xFFFFFFFFll)), hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// ranks of the (up to NV_PER) list entries lane + 64 q, q < NV_PER, among the `fill` entries of the list (fill is the same in every
// lane); entries past fill: (inf, INT_MAX), rank fill
__device__ __forceinline__ void rank_list(int fill, int lane, const double* sd2, const int32_t* sj, double (&md)[NV_PER], int32_t (&mj)[NV_PER],
                                          int (&rk)[NV_PER]) {
#pragma unroll
  for (int q = 0; q < NV_PER; q++) {
    const int e = lane + NV_WAVE * q;
    md[q] = e < fill ? sd2[e] : __builtin_inf();
    mj[q] = e < fill ? sj[e] : 0x7FFFFFFF;
    rk[q] = 0;
  }
  for (int t = 0; t < fill; t++) {  // (every lane reads the same entry: a broadcast)
    const double  d = sd2[t];
    const int32_t j = sj[t];
#pragma unroll
    for (int q = 0; q < NV_PER; q++) rk[q] += mrs_sight::before(d, j, md[q], mj[q]) ? 1 : 0;
  }
}

// T: element type of the rows; W: empty, or the label column (const uint32_t*) — a swarm without labels runs the kernel without them
template <typename T, class... W>
__global__ void __launch_bounds__(NV_WAVE) k_nn_visible(VisArgs g, W... labels) {
  constexpr bool WORLDS = sizeof...(W) != 0;
  __shared__ double  sd2[NV_CAP];
  __shared__ int32_t sj[NV_CAP];
  const NnArgs& a    = g.a;
  const int     lane = (int)threadIdx.x;
  const int     row  = (int)blockIdx.x;
  const int     i    = a.first + row;  // the observer: the same in every lane
  const size_t  np   = (size_t)a.npad;
  const double  p[3] = {uniform(a.S[(size_t)F_X * np + i]), uniform(a.S[(size_t)(F_X + 1) * np + i]), uniform(a.S[(size_t)(F_X + 2) * np + i])};
  uint32_t      myw  = 0u;
  if constexpr (WORLDS) myw = (uint32_t)__builtin_amdgcn_readfirstlane((int)world_labels(labels...)[i]);
  int nvis = 0, nhid = 0, fill = 0;  // (the same in every lane)
  if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
    uint32_t wm = 0u;
    if constexpr (WORLDS) wm = world_mix(myw);
    const int cx = cell_coord(p[0], a.inv_edge), cy = cell_coord(p[1], a.inv_edge), cz = cell_coord(p[2], a.inv_edge);
    // lane pr < 27 forms the bucket of probe pr; bit pr of `dup`: probe pr hits a bucket an earlier probe reads already
    const int      pl   = lane < 27 ? lane : 26;
    const uint32_t mine = bucket_of_x<WORLDS>(cx + pl % 3 - 1, cy + (pl / 3) % 3 - 1, cz + pl / 9 - 1, a.tmask, wm);
    bool           d    = false;
    for (int o = 0; o < 26; o++) {
      const uint32_t bo = (uint32_t)__shfl((int)mine, o, NV_WAVE);
      d                 = d || (o < lane && bo == mine);
    }
    const unsigned long long dup = __ballot(d && lane < 27);
    // Every bound that decides whether a barrier is reached is formed from the observer alone (its cell, the buckets' starts and counts,
    // the list's fill as a ballot count) and passed through readfirstlane: block-uniform by construction, never a lane's own data.
    for (int pr = 0; pr < 27; pr++) {
      if ((dup >> pr) & 1ull) continue;
      const uint32_t bk  = (uint32_t)__builtin_amdgcn_readfirstlane((int)bucket_of_x<WORLDS>(cx + pr % 3 - 1, cy + (pr / 3) % 3 - 1, cz + pr / 9 - 1, a.tmask, wm));
      const int      beg = __builtin_amdgcn_readfirstlane(max(bucket_begin(a.start, a.bsum, bk), 0));
      const int      end = __builtin_amdgcn_readfirstlane(min(beg + a.cnt[bk], a.n));
      for (int s0 = beg; s0 < end; s0 += NV_WAVE) {
        const int s    = s0 + lane;
        bool      cand = false, hid = false;
        double    d2   = 0.0;
        int32_t   j    = -1;
        if (s < end) {
          const NnRec  r     = a.rec[s];
          const double dx[3] = {r.x - p[0], r.y - p[1], r.z - p[2]};
          d2   = ((dx[0] * dx[0]) + dx[1] * dx[1]) + dx[2] * dx[2];
          j    = r.idx;
          cand = d2 < a.rr && j != i && (unsigned)j < (unsigned)a.n;
          if constexpr (WORLDS) cand = cand && (uint32_t)r.pad == myw;  // another world: never a neighbour, however close
          if (cand && d2 != 0.0 && g.v.m > 0) {  // (a coincident UAV is visible, with no test)
            double       u[3];
            const double dist = mrs_sight::direction(dx, d2, u);
            mrs_obst::walk_cell(g.v, p, myw, [&](int, const mrs_obstacle_t& o) {
              if (!hid) hid = mrs_sight::hides(o, p, u, dist, g.radius);
            });
          }
        }
        const bool               vis  = cand && !hid;
        const unsigned long long mask = __ballot(vis);
        const int                c    = __builtin_amdgcn_readfirstlane(__popcll(mask));
        nhid += __builtin_amdgcn_readfirstlane(__popcll(__ballot(cand && hid)));
        nvis += c;
        if (fill + c > NV_CAP) {  // (the same in every lane) reduce the list in place to its first k entries
          __syncthreads();
          double  md[NV_PER];
          int32_t mj[NV_PER];
          int     rk[NV_PER];
          rank_list(fill, lane, sd2, sj, md, mj, rk);
          __syncthreads();  // (every lane has read what it ranks before any entry moves)
#pragma unroll
          for (int q = 0; q < NV_PER; q++)
            if (lane + NV_WAVE * q < fill && rk[q] < a.k) sd2[rk[q]] = md[q], sj[rk[q]] = mj[q];  // rk < k <= 32 < NV_CAP
          fill = min(fill, a.k);
          __syncthreads();
        }
        if (vis) {
          const int e = fill + __popcll(mask & ((1ull << lane) - 1ull));  // < fill + c <= NV_CAP
          sd2[e] = d2, sj[e] = j;
        }
        fill += c;
      }
    }
  }
  __syncthreads();
  const int nf = nvis < a.k ? nvis : a.k;  // (fill >= nf: a reduction keeps k entries)
  if (lane == 0) {
    if (a.counts) a.counts[row] = nf;
    if (g.visible) g.visible[row] = nvis;
    if (g.hidden) g.hidden[row] = nhid;
  }
  if (!a.index && !a.fields) return;
  double  md[NV_PER];
  int32_t mj[NV_PER];
  int     rk[NV_PER];
  rank_list(fill, lane, sd2, sj, md, mj, rk);
  int32_t* oi = a.index ? a.index + (size_t)row * (size_t)a.index_stride : nullptr;
  if (oi) {
#pragma unroll
    for (int q = 0; q < NV_PER; q++)
      if (lane + NV_WAVE * q < fill && rk[q] < nf) oi[rk[q]] = mj[q];
    if (lane >= nf && lane < a.k) oi[lane] = -1;
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
  T* o = static_cast<T*>(a.rows) + (size_t)row * (size_t)a.stride;
#pragma unroll
  for (int q = 0; q < NV_PER; q++)
    if (lane + NV_WAVE * q < fill && rk[q] < nf) write_slot(o + (size_t)rk[q] * (size_t)a.width, a, true, mj[q], md[q], p, vi, R);
  if (lane >= nf && lane < a.k) write_slot(o + (size_t)lane * (size_t)a.width, a, false, 0, 0.0, p, vi, R);
}

template <typename T>
void launch(const VisArgs& g, const uint32_t* wlab, hipStream_t st) {
  const dim3 grid((unsigned)g.a.count);
  if (wlab)
    hipLaunchKernelGGL((k_nn_visible<T, const uint32_t*>), grid, dim3(NV_WAVE), 0, st, g, wlab);
  else
    hipLaunchKernelGGL((k_nn_visible<T>), grid, dim3(NV_WAVE), 0, st, g);
}

}  // namespace

extern "C" {

int mrs_swarm_nearest_visible_device(mrs_swarm_t* s, int32_t first, int32_t count, int32_t k, double radius, uint32_t fields, void* dev_rows,
                                     int32_t dtype, int32_t stride, int32_t* dev_index, int32_t index_stride, int32_t* dev_count,
                                     int32_t* dev_visible, int32_t* dev_hidden, void* ext_stream) {
  MRS_ENTER_COMMANDS(s);
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, "mrs_swarm_nearest_visible_device: not on a sharded swarm");
  int32_t width = 0;
  if ((rc = mrs_nearest_width(fields, k, &width))) return rc;
  if (!(radius > 0.0) || !std::isfinite(radius)) return fail(MRS_ERR_ARG, "radius must be finite and > 0");
  if (!dev_index && !dev_count && !dev_visible && !dev_hidden && !(fields && dev_rows))
    return fail(MRS_ERR_ARG, "no output given (dev_rows with fields, dev_index, dev_count, dev_visible or dev_hidden)");
  if (fields) {
    if ((rc = check_dtype(dtype))) return rc;
    if (stride < width) return fail(MRS_ERR_ARG, "stride smaller than k * the width of the selected fields");
  }
  if (dev_index && index_stride < k) return fail(MRS_ERR_ARG, "index_stride smaller than k");
  if (count == 0) return MRS_OK;
  if (fields && (rc = check_device_ptr(s, dev_rows, rows_bytes(count, stride, width, dtype), "dev_rows"))) return rc;
  if (dev_index && (rc = check_device_ptr(s, dev_index, index_rows_bytes(count, index_stride, k), "dev_index"))) return rc;
  if (dev_count && (rc = check_device_ptr(s, dev_count, index_rows_bytes(count, 1, 1), "dev_count"))) return rc;
  if (dev_visible && (rc = check_device_ptr(s, dev_visible, index_rows_bytes(count, 1, 1), "dev_visible"))) return rc;
  if (dev_hidden && (rc = check_device_ptr(s, dev_hidden, index_rows_bytes(count, 1, 1), "dev_hidden"))) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  if ((rc = sight_grid(s, radius))) return rc;
  mrs_nn::NnHash h;
  if ((rc = nn_hash(s, radius, ext, &h))) return rc;  // (fences the caller's stream in)
  VisArgs g;
  memset(&g, 0, sizeof g);
  g.a.S            = s->dS;
  g.a.n            = h.n;
  g.a.npad         = s->npad;
  g.a.first        = first;
  g.a.count        = count;
  g.a.k            = k;
  g.a.inv_edge     = h.inv_edge;
  g.a.rr           = radius * radius;  // rounded here, once
  g.a.tmask        = h.tmask;
  g.a.cnt          = h.cnt;
  g.a.start        = h.start;
  g.a.bsum         = h.bsum;
  g.a.rec          = h.rec;
  g.a.fields       = dev_rows ? fields : 0u;
  g.a.rows         = dev_rows;
  g.a.stride       = stride;
  g.a.width        = fields ? width / k : 0;
  g.a.index        = dev_index;
  g.a.index_stride = index_stride;
  g.a.counts       = dev_count;
  g.v              = grid_view(*s->obst, s->obst->sight);
  g.radius         = radius;
  g.visible        = dev_visible;
  g.hidden         = dev_hidden;
  if (dtype == MRS_DTYPE_F32)
    launch<float>(g, s->dWorld, s->stream);
  else
    launch<double>(g, s->dWorld, s->stream);
  HIPCHK(hipGetLastError());
  return fence_out(s, ext);
}

}  // extern "C"
