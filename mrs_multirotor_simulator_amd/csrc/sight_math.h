// sight_math.h — the pure functions of the line-of-sight neighbours (include/mrs_swarm.h, "line-of-sight neighbours";
// nearest_visible.hip): the direction of a sight line from the offset to a candidate, whether one obstacle hides the candidate, and the
// order in which visible candidates are listed, as the contract states them operation by operation.  No GPU call, so that all of it is
// exercised without one (tests/cpp/sight_math_test.cpp); these are the very functions the kernel of nearest_visible.hip calls.  FP64,
// one rounding per operation: every function turns contraction off for itself, and the units that include this are compiled without it.
#pragma once
#include "range_scan_math.h"

namespace mrs_sight {

// the sight line to a candidate at offset dx (d2 = ((dx*dx) + dy*dy) + dz*dz > 0, formed by the caller): its length d = sqrt(d2), which
// is returned, and its direction u = dx / d, three separately rounded divisions.  d2 == 0 has no direction: the caller does not ask.
MRS_OBST_HD double direction(const double dx[3], double d2, double u[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d = sqrt(d2);
  u[0] = dx[0] / d;
  u[1] = dx[1] / d;
  u[2] = dx[2] / d;
  return d;
}

// does obstacle o hide a target at range d along u from an observer at p: o is a candidate of the observer (mrs_scan::gate for the
// call's radius) and the sight line enters the closed solid strictly before the target (mrs_scan::ray).  A NaN never hides, a target
// exactly on the surface is visible, and an observer inside o (ray == 0) sees nothing at d > 0.
MRS_OBST_HD bool hides(const mrs_obstacle_t& o, const double p[3], const double u[3], double d, double radius) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!mrs_scan::gate(o, p, radius)) return false;
  return mrs_scan::ray(o, p, u) < d;
}

// (d2, j) is listed before (e2, m)
MRS_OBST_HD bool before(double d2, int32_t j, double e2, int32_t m) { return d2 < e2 || (d2 == e2 && j < m); }

}  // namespace mrs_sight
