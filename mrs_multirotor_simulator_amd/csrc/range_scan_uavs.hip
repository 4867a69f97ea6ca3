// range_scan_uavs.hip — range scans that also see the other UAVs of the observer's world (include/mrs_swarm.h, "range scans that see other
// UAVs"): the scan of range_scan.hip, and between its obstacles and its ground plane every same-world UAV as a closed sphere of radius
// arm_length + prop_radius.  The join of two things that exist: the ray tests of range_scan_math.h and the per-call hash of UAV positions
// that nearest.hip builds (nn_hash.h), for radius = max_range + the largest airframe radius, so that the 27 buckets around the observer's
// cell list every candidate of the contract's gate (DESIGN §7c has the argument).
// One 64-lane block (one wave) per (observer, group of 64 consecutive beams).  A UAV has on the order of a hundred candidate UAVs spread
// over 27 buckets, each with a dependent load for its airframe radius: the block gathers them once, 64 records at a time across its
// lanes, into a chunk in LDS, and every lane then runs ray + take_uav over the chunk for its own beam (all lanes read the same entry: a
// broadcast, no bank conflict).  Gather and sweep repeat until the buckets are exhausted: the running (t, j) minimum is associative.
// Beam set-up, obstacle pass, ground pass, range / hit stores, argument checks and fill are range_scan_common.h's, the very functions
// k_range_scan calls; what is this unit's own: the block shape, the live lanes, gather and sweep, the UAV / ground merge, the uav rows.
// Nothing here writes simulation state; entry, fence and scratch are those of the scans and of nearest (the swarm's nn_buf).
#include "nn_hash.h"
#include "range_scan_common.h"

namespace {

constexpr int RU_WAVE = 64;   // lanes of a block: one wave, so every barrier below is reached by all of its lanes or by none
constexpr int RU_CAP  = 256;  // entries of the candidate chunk in LDS (tests/test_range_scan_uavs_gpu.py names this value): 9 KiB per block

struct UavScanArgs {
  ScanCommon     c;
  mrs_nn::NnHash h;  // the hash of the UAV positions
  int32_t*       uav;
  int32_t        uav_stride, groups;
};

// every lane runs ray + take_uav over the `fill` chunk entries for its own beam (fill is the same in every lane)
__device__ __forceinline__ void sweep(int fill, const double* cx, const double* cy, const double* cz, const double* crad, const int32_t* cj,
                                      const double p[3], const double u[3], double* bt, int32_t* bj) {
  for (int e = 0; e < fill; e++) {
    const double         q[3] = {cx[e], cy[e], cz[e]};
    const mrs_obstacle_t o    = mrs_scan::uav_target(q, crad[e]);
    mrs_scan::take_uav(mrs_scan::ray(o, p, u), cj[e], bt, bj);
  }
}

// T: element type of the range rows; W: empty, or the label column (const uint32_t*) — a swarm without labels runs the kernel without them
template <typename T, class... W>
__global__ void __launch_bounds__(RU_WAVE) k_range_scan_uavs(UavScanArgs a, W... labels) {
  using namespace mrs_nn;
  constexpr bool WORLDS = sizeof...(W) != 0;
  __shared__ double  cx[RU_CAP], cy[RU_CAP], cz[RU_CAP], crad[RU_CAP];
  __shared__ int32_t cj[RU_CAP];
  const int  lane = (int)threadIdx.x;
  const int  r    = (int)(blockIdx.x / (unsigned)a.groups), grp = (int)(blockIdx.x - (unsigned)r * (unsigned)a.groups);
  const int  i    = a.c.first + r;  // the observer: the same in every lane
  const int  b    = RU_WAVE * grp + lane;
  const bool live = b < a.c.n_beams;  // lanes past the pattern stay in the block, take part in every barrier and store nothing
  double     p[3], u[3];
  scan_beam(a.c, i, live ? b : a.c.n_beams - 1, p, u);
  double     best = a.c.max_range;
  int        idx  = MRS_SCAN_HIT_NONE, who = -1;
  const bool seen = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);  // (the same in every lane)
  if (seen) {
    uint32_t myw = 0u;
    if constexpr (WORLDS) myw = world_labels(labels...)[i];
    if (a.c.v.m > 0) scan_obstacles(a.c, p, u, myw, &best, &idx);
    // ---- the UAVs: gather the candidates of the 27 buckets into the chunk, sweep it whenever it cannot take 64 more ----
    // Two probed cells may hash to one bucket, whose records are then gathered twice.  k_nn_query must not count a neighbour twice and
    // removes such probes; here a second arrival of (t, j) changes nothing — take_uav is a minimum, and a minimum is idempotent — so the
    // probes stay as they are.
    // Every bound that decides whether a barrier is reached is formed from the observer alone (its cell, the buckets' starts and counts,
    // the chunk's fill as a ballot count) and passed through readfirstlane: block-uniform by construction, never a lane's own data.
    double   bt = mrs_scan::miss();
    int32_t  bj = 0x7FFFFFFF;
    uint32_t wm = 0u;
    if constexpr (WORLDS) wm = world_mix(myw);
    const int ccx = cell_coord(p[0], a.h.inv_edge), ccy = cell_coord(p[1], a.h.inv_edge), ccz = cell_coord(p[2], a.h.inv_edge);
    int       fill = 0;
    for (int pr = 0; pr < 27; pr++) {
      const uint32_t bk  = (uint32_t)__builtin_amdgcn_readfirstlane(
          (int)bucket_of_x<WORLDS>(ccx + pr % 3 - 1, ccy + (pr / 3) % 3 - 1, ccz + pr / 9 - 1, a.h.tmask, wm));
      const int      beg = __builtin_amdgcn_readfirstlane(max(bucket_begin(a.h.start, a.h.bsum, bk), 0));
      const int      end = __builtin_amdgcn_readfirstlane(min(beg + a.h.cnt[bk], a.h.n));
      for (int s0 = beg; s0 < end; s0 += RU_WAVE) {
        const int s    = s0 + lane;
        bool      pass = false;
        double    q[3] = {0.0, 0.0, 0.0}, rad = 0.0;
        int32_t   j    = -1;
        if (s < end) {
          const NnRec rec = a.h.rec[s];
          j               = rec.idx;
          q[0] = rec.x, q[1] = rec.y, q[2] = rec.z;
          pass = j != i && (unsigned)j < (unsigned)a.h.n;
          if constexpr (WORLDS) pass = pass && (uint32_t)rec.pad == myw;  // another world: invisible, however close
          if (pass) {
            const TypeParams& tp = a.c.T[a.c.F[j] >> FLAG_TYPE_SHIFT];
            rad  = tp.arm_length + tp.prop_radius;
            pass = mrs_scan::gate(mrs_scan::uav_target(q, rad), p, a.c.max_range);
          }
        }
        const unsigned long long mask = __ballot(pass);
        const int                c    = __builtin_amdgcn_readfirstlane(__popcll(mask));
        if (fill + c > RU_CAP) {  // (the same in every lane)
          __syncthreads();
          sweep(fill, cx, cy, cz, crad, cj, p, u, &bt, &bj);
          __syncthreads();
          fill = 0;
        }
        if (pass) {
          const int e = fill + __popcll(mask & ((1ull << lane) - 1ull));  // < fill + c <= RU_CAP
          cx[e] = q[0], cy[e] = q[1], cz[e] = q[2], crad[e] = rad, cj[e] = j;
        }
        fill += c;
      }
    }
    __syncthreads();
    sweep(fill, cx, cy, cz, crad, cj, p, u, &bt, &bj);
    // ---- finish: an obstacle at the same range keeps the beam; then the ground ----
    if (bt < best) {
      best = bt;
      idx  = MRS_UAVSCAN_HIT_UAV;
      who  = bj;
    }
    if (scan_ground(a.c, i, p, u, &best, &idx)) who = -1;
  }
  if (!live) return;
  scan_store<T>(a.c, r, b, best, idx);
  if (a.uav) a.uav[(size_t)r * (size_t)a.uav_stride + (size_t)b] = who;
}

template <typename T>
void launch(const UavScanArgs& a, int32_t count, const uint32_t* wlab, hipStream_t st) {
  const dim3 grid((unsigned)((int64_t)count * a.groups));
  if (wlab)
    hipLaunchKernelGGL((k_range_scan_uavs<T, const uint32_t*>), grid, dim3(RU_WAVE), 0, st, a, wlab);
  else
    hipLaunchKernelGGL((k_range_scan_uavs<T>), grid, dim3(RU_WAVE), 0, st, a);
}

}  // namespace

extern "C" {

int mrs_swarm_range_scan_uavs_device(mrs_swarm_t* s, int32_t first, int32_t count, double max_range, uint32_t flags, void* dev_ranges, int32_t dtype,
                                     int32_t stride, int32_t* dev_hit, int32_t hit_stride, int32_t* dev_uav, int32_t uav_stride, void* ext_stream) {
  MRS_ENTER_COMMANDS(s);
  const int32_t  nb = scan_beam_count(s), groups = (nb + RU_WAVE - 1) / RU_WAVE;
  const ScanRows rows{dev_ranges, dtype, stride, dev_hit, hit_stride, dev_uav, uav_stride};
  int            rc = check_scan(s, "mrs_swarm_range_scan_uavs_device", nb, first, count, max_range, flags, rows, (int64_t)count * groups,
                                 "count * ceil(n_beams / 64) exceeds one launch (2^31 blocks)");
  if (rc || count == 0) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t ext = (hipStream_t)ext_stream;
  // the airframe radii (and the ground plane) are read from the airframe table: current before the launch
  if ((rc = upload_types(s, s->table_dt > 0 ? s->table_dt : 0.001))) return rc;
  if ((rc = scan_grid(s, max_range))) return rc;
  // the hash edge: every candidate passes |d_a| - rad_j < max_range, so |d_a| < max_range + rmax up to a few ulps, which the margin of
  // the edge (1e-6 relative) covers: the candidate's cell differs from the observer's by at most 1 on every axis
  double rmax = 0.0;
  for (const TypeParams& tp : s->tparams) {
    const double rad = tp.arm_length + tp.prop_radius;
    if (std::isfinite(rad) && rad > rmax) rmax = rad;
  }
  UavScanArgs a;
  memset(&a, 0, sizeof a);
  if ((rc = nn_hash(s, max_range + rmax, ext, &a.h))) return rc;  // (fences the caller's stream in)
  a.c          = scan_common(s, first, nb, max_range, flags, rows);
  a.uav        = dev_uav;
  a.uav_stride = uav_stride;
  a.groups     = groups;
  if (dtype == MRS_DTYPE_F32)
    launch<float>(a, count, s->dWorld, s->stream);
  else
    launch<double>(a, count, s->dWorld, s->stream);
  HIPCHK(hipGetLastError());
  return fence_out(s, ext);
}

}  // extern "C"
