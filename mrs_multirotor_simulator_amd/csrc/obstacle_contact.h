// obstacle_contact.h — the pure functions of the obstacle contacts (include/mrs_swarm.h, "obstacle contacts"; obstacle_contact.hip): the
// body radius and the threshold of one UAV, the fold of one visited obstacle into (count, best sd, best index), and the search of one
// UAV over the one grid cell that contains it (mrs_obst::walk_cell, obstacle_grid.h).  No GPU call, so that all of it is exercised
// without one (tests/cpp/obstacle_contact_math_test.cpp); these are the very functions k_obst_contact calls.  Units that include this
// are compiled without contraction; the pragmas below say so once more where an addition is the contract.
#pragma once
#include "obstacle_grid.h"

namespace mrs_obst {

// rad_i = arm_length + prop_radius: one FP64 addition, the sphere of the range scans that see UAVs, the prefix of the collision criterion
MRS_OBST_HD double contact_radius(double arm_length, double prop_radius) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return arm_length + prop_radius;
}
// thr_i = rad_i + margin: one more FP64 addition
MRS_OBST_HD double contact_threshold(double rad, double margin) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return rad + margin;
}

// what a UAV keeps of its touching set: |C_i|, and the lexicographic minimum of (sd, j) over it ((+inf, INT_MAX) while it is empty)
struct Contact {
  int    count;
  double sd;
  int    j;
};
MRS_OBST_HD Contact contact_none() { return {0, (double)INFINITY, 0x7FFFFFFF}; }

// obstacle j at signed distance sd folded into c: it belongs to the touching set if sd < thr, strictly (a NaN on either side misses);
// (sd, j) replaces the kept pair if it orders before it — -0.0 == +0.0, so such a tie goes to the lower index, whatever the order of
// the visits
MRS_OBST_HD void contact_fold(Contact& c, double sd, int j, double thr) {
  if (!(sd < thr)) return;
  c.count++;
  if (sd < c.sd || (sd == c.sd && j < c.j)) {
    c.sd = sd;
    c.j  = j;
  }
}

// The touching set of a UAV at p with world label myw and threshold thr, folded: empty when the set is, when a coordinate of p is not
// finite, and (by the comparison of contact_fold) when thr is NaN.  v is a grid built for a radius R >= thr: sd < thr implies sd < R, so
// the one cell that contains p lists every member (obstacle_grid.h), and every listed obstacle is tested literally.
MRS_OBST_HD Contact contact_search(const GridView& v, const double p[3], uint32_t myw, double thr) {
  Contact c = contact_none();
  if (v.m > 0 && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))
    walk_cell(v, p, myw, [&](int j, const mrs_obstacle_t& o) {
      double rel[3];
      contact_fold(c, eval(o, p, rel), j, thr);
    });
  return c;
}

// the index and the distance a caller is given: (-1, +inf) for an empty touching set
MRS_OBST_HD int    contact_index(const Contact& c) { return c.count > 0 ? c.j : -1; }
MRS_OBST_HD double contact_sd(const Contact& c) { return c.count > 0 ? c.sd : (double)INFINITY; }

}  // namespace mrs_obst
