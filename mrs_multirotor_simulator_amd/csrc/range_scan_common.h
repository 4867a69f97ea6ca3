// range_scan_common.h — what the two scan units share (range_scan.hip: k_range_scan; range_scan_uavs.hip: k_range_scan_uavs), each with ONE
// definition, because bit-for-bit agreement between the two calls rests on exactly these lines: the common argument block, the beam set-up
// (p and u of an observer and a beam), the obstacle pass (the walk of obstacle_grid.h with the gate / ray / strict-< body), the ground
// pass, the row stores, and on the host the argument checks and the fill of the block.  The pure functions are those of range_scan_math.h.
#pragma once
#include "host_internal.h"
#include "obstacle_set.h"
#include "pose_math.h"
#include "range_scan_math.h"

struct ScanCommon {
  const double*      S;
  const uint32_t*    F;
  const TypeParams*  T;
  int32_t            npad, first, n_beams;
  uint32_t           flags;
  const double*      beams;
  double             max_range;
  mrs_obst::GridView v;  // the set through the scans' grid (built for radius = max_range)
  void*              ranges;
  int32_t*           hit;
  int32_t            stride, hit_stride;
};

// position p of observer i and direction u of beam b in the world frame
__device__ __forceinline__ void scan_beam(const ScanCommon& a, int i, int b, double p[3], double u[3]) {
  const size_t np = (size_t)a.npad;
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
}

// the obstacles of p's cell into (*best, *idx); p is finite and the set is not empty (the callers' guards).  Obstacle indices ascend
// within a cell: a strict < keeps the lowest index among equal ranges.  The update is two selects, as the compiler made it when best and
// idx were the kernel's own locals: written as a conditional store through the pointers it stays a branch.
__device__ __forceinline__ void scan_obstacles(const ScanCommon& a, const double p[3], const double u[3], uint32_t myw, double* best, int* idx) {
  mrs_obst::walk_cell(a.v, p, myw, [&](int j, const mrs_obstacle_t& o) {
    if (!mrs_scan::gate(o, p, a.max_range)) return;
    const double t      = mrs_scan::ray(o, p, u);
    const bool   nearer = t < *best;
    *best = nearer ? t : *best;
    *idx  = nearer ? j : *idx;
  });
}

// the ground plane of observer i's airframe into (*best, *idx), if the call asks for it; true: the ground took the beam
__device__ __forceinline__ bool scan_ground(const ScanCommon& a, int i, const double p[3], const double u[3], double* best, int* idx) {
  if (!(a.flags & MRS_SCAN_GROUND)) return false;
  const double t      = mrs_scan::ground(p[2], u[2], a.T[a.F[i] >> FLAG_TYPE_SHIFT].ground_z);
  const bool   nearer = t < *best;  // (strictly: an obstacle or a UAV at the same range keeps the beam)
  *best = nearer ? t : *best;
  *idx  = nearer ? MRS_SCAN_HIT_GROUND : *idx;
  return nearer;
}

// beam b of row r: its range as T and, if asked for, its hit value
template <typename T>
__device__ __forceinline__ void scan_store(const ScanCommon& a, int r, int b, double best, int idx) {
  static_cast<T*>(a.ranges)[(size_t)r * (size_t)a.stride + (size_t)b] = (T)best;
  if (a.hit) a.hit[(size_t)r * (size_t)a.hit_stride + (size_t)b] = idx;
}

// the caller's output rows as an entry point received them; uav / uav_stride: null / 0 for the scan that has no UAV rows
struct ScanRows {
  void*    ranges;
  int32_t  dtype, stride;
  int32_t* hit;
  int32_t  hit_stride;
  int32_t* uav;
  int32_t  uav_stride;
};

// The argument checks of the scan entry point `call`, in the order its refusals are documented.  nb: beams of the pattern; blocks: the
// launch the call would make, refused with `too_many` when it exceeds one grid.  MRS_OK with count == 0 means there is nothing to do.
inline int check_scan(const mrs_swarm* s, const char* call, int32_t nb, int32_t first, int32_t count, double max_range, uint32_t flags,
                      const ScanRows& rows, int64_t blocks, const char* too_many) {
  int rc = check_range(s, first, count);
  if (rc) return rc;
  if (s->comm_world > 0) return fail(MRS_ERR_ARG, std::string(call) + ": not on a sharded swarm");
  if (nb == 0) return fail(MRS_ERR_ARG, "no beam pattern set (mrs_swarm_set_scan_beams)");
  if (!(max_range > 0.0) || !std::isfinite(max_range)) return fail(MRS_ERR_ARG, "max_range must be finite and > 0");
  if (flags & ~(uint32_t)(MRS_SCAN_BODY_FRAME | MRS_SCAN_GROUND)) return fail(MRS_ERR_ARG, "unknown scan flag bits");
  if ((rc = check_dtype(rows.dtype))) return rc;
  if (rows.stride < nb) return fail(MRS_ERR_ARG, "stride smaller than n_beams");
  if (rows.hit && rows.hit_stride < nb) return fail(MRS_ERR_ARG, "hit_stride smaller than n_beams");
  if (rows.uav && rows.uav_stride < nb) return fail(MRS_ERR_ARG, "uav_stride smaller than n_beams");
  if (!rows.ranges) return fail(MRS_ERR_ARG, "dev_ranges: null pointer");
  if (blocks > 0x7FFFFFFFll) return fail(MRS_ERR_ARG, too_many);
  if (count == 0) return MRS_OK;
  if ((rc = check_device_ptr(s, rows.ranges, rows_bytes(count, rows.stride, nb, rows.dtype), "dev_ranges"))) return rc;
  if (rows.hit && (rc = check_device_ptr(s, rows.hit, index_rows_bytes(count, rows.hit_stride, nb), "dev_hit"))) return rc;
  if (rows.uav && (rc = check_device_ptr(s, rows.uav, index_rows_bytes(count, rows.uav_stride, nb), "dev_uav"))) return rc;
  return MRS_OK;
}

// the common block of a checked call; the scans' grid is current (scan_grid)
inline ScanCommon scan_common(const mrs_swarm* s, int32_t first, int32_t nb, double max_range, uint32_t flags, const ScanRows& rows) {
  ScanCommon a;
  memset(&a, 0, sizeof a);
  a.S          = s->dS;
  a.F          = s->dF;
  a.T          = s->dT;
  a.npad       = s->npad;
  a.first      = first;
  a.n_beams    = nb;
  a.flags      = flags;
  a.beams      = scan_beams_dev(s);
  a.max_range  = max_range;
  a.v          = grid_view(*s->obst, s->obst->scan);
  a.ranges     = rows.ranges;
  a.hit        = rows.hit;
  a.stride     = rows.stride;
  a.hit_stride = rows.hit_stride;
  return a;
}
