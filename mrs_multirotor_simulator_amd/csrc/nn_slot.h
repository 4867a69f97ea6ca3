// nn_slot.h — one slot of a neighbour row (include/mrs_swarm.h, "nearest-neighbour observations"): the argument block of a query kernel
// and the field arithmetic of a listed neighbour, with ONE definition for the kernels that write such rows: k_nn_query of nearest.hip and
// k_nn_visible of nearest_visible.hip, whose rows must agree bit for bit wherever no obstacle hides anybody.  Device code only; the text
// is what nearest.hip held.
#pragma once
#include "host_internal.h"
#include "nn_hash.h"
#include "pose_math.h"

namespace mrs_nn {

struct NnArgs {
  const double* S;
  int32_t       n, npad, first, count, k;
  double        inv_edge, rr;
  uint32_t      tmask, fields;
  const int32_t *cnt, *start, *bsum;
  const NnRec*  rec;
  void*         rows;
  int32_t       stride, width;  // width: elements of one slot
  int32_t*      index;
  int32_t       index_stride;
  int32_t*      counts;
};

template <typename T>
__device__ __forceinline__ void put3(T* o, double a, double b, double c) {
  o[0] = (T)a;
  o[1] = (T)b;
  o[2] = (T)c;
}

// slot of neighbour j (d2 apart) of a UAV at xs with velocity vi and attitude R, or an empty slot (zeros)
template <typename T>
__device__ __forceinline__ void write_slot(T* o, const NnArgs& a, bool valid, int j, double d2, const double xs[3], const double vi[3],
                                           const double R[9]) {
  if (!valid) {
    for (int e = 0; e < a.width; e++) o[e] = (T)0;
    return;
  }
  const uint32_t f  = a.fields;
  const size_t   np = (size_t)a.npad;
  double         d[3], w[3];
  if (f & (MRS_NN_REL_POS | MRS_NN_REL_POS_BODY)) {
#pragma unroll
    for (int c = 0; c < 3; c++) d[c] = a.S[(size_t)(F_X + c) * np + j] - xs[c];
  }
  if (f & (MRS_NN_REL_VEL | MRS_NN_REL_VEL_BODY)) {
#pragma unroll
    for (int c = 0; c < 3; c++) w[c] = a.S[(size_t)(F_V + c) * np + j] - vi[c];
  }
  if (f & MRS_NN_REL_POS) {
    put3(o, d[0], d[1], d[2]);
    o += 3;
  }
  if (f & MRS_NN_REL_POS_BODY) {
    put3(o, body_velocity(R, d, 0), body_velocity(R, d, 1), body_velocity(R, d, 2));
    o += 3;
  }
  if (f & MRS_NN_REL_VEL) {
    put3(o, w[0], w[1], w[2]);
    o += 3;
  }
  if (f & MRS_NN_REL_VEL_BODY) {
    put3(o, body_velocity(R, w, 0), body_velocity(R, w, 1), body_velocity(R, w, 2));
    o += 3;
  }
  if (f & MRS_NN_DIST) o[0] = (T)sqrt(d2);
}

}  // namespace mrs_nn
