// range_scan_math.h — the pure functions of the range scans (include/mrs_swarm.h, "range scans"; range_scan.hip): which obstacles a UAV's
// beams are tested against (gate), where a beam enters one closed solid (ray) and where it meets the ground plane (ground), as the
// contract states them operation by operation.  No GPU call, so that all of it is exercised without one
// (tests/cpp/range_scan_math_test.cpp); these are the very functions the kernel of range_scan.hip calls.  FP64, one rounding per
// operation: every function turns contraction off for itself, and the units that include this are compiled without it.
#pragma once
#include "obstacle_grid.h"

namespace mrs_scan {

using mrs_obst::mn;
using mrs_obst::mx;

// what ray() and ground() return for a beam that does not meet the solid: it orders behind every range, so `t < best` drops it
MRS_OBST_HD double miss() { return __builtin_inf(); }

// is obstacle o a candidate of a UAV at p for scans of max_range: on every axis the distance to o's bounding box (the half-extents of
// mrs_obst::half_extents) is below max_range.  The inequality the coverage proof of obstacle_grid.h passes through: the one cell of p in a
// grid built for radius = max_range lists every obstacle for which this holds.
MRS_OBST_HD bool gate(const mrs_obstacle_t& o, const double p[3], double max_range) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double hb[3];
  mrs_obst::half_extents(o, hb);
  return (fabs(p[0] - o.c[0]) - hb[0] < max_range) && (fabs(p[1] - o.c[1]) - hb[1] < max_range) && (fabs(p[2] - o.c[2]) - hb[2] < max_range);
}

// One axis of a slab |d + t u| <= h intersected into [*enter, *exit]; false: the beam runs beside the slab.  u == 0 is decided by where the
// origin lies and imposes no bound (no division, no 0 * inf); h = +inf (a pillar's z) gives (-inf, +inf).
MRS_OBST_HD bool slab(double d, double u, double h, double* enter, double* exit) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (u == 0.0) return !(fabs(d) > h);
  const double t1 = (-h - d) / u, t2 = (h - d) / u;
  *enter = mx(*enter, mn(t1, t2));
  *exit  = mn(*exit, mx(t1, t2));
  return true;
}

// The range t >= 0 at which the beam p + t u (u a unit vector) enters the closed solid o, 0 when p lies in it or on its surface, miss()
// when it does not meet it.  Every comparison is written so that a NaN misses.
MRS_OBST_HD double ray(const mrs_obstacle_t& o, const double p[3], const double u[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double dx = p[0] - o.c[0], dy = p[1] - o.c[1], dz = p[2] - o.c[2];
  if (o.kind == MRS_OBST_SPHERE) {
    const double r  = o.h[0];
    const double cc = (((dx * dx) + dy * dy) + dz * dz) - r * r;
    if (cc <= 0.0) return 0.0;
    const double b = ((dx * u[0]) + dy * u[1]) + dz * u[2];
    if (!(b < 0.0)) return miss();
    const double disc = b * b - cc;
    if (!(disc >= 0.0)) return miss();
    return cc / (-b + sqrt(disc));
  }
  double enter = 0.0, exit = __builtin_inf();
  if (o.kind == MRS_OBST_BOX) {
    if (!slab(dx, u[0], o.h[0], &enter, &exit)) return miss();
    if (!slab(dy, u[1], o.h[1], &enter, &exit)) return miss();
    if (!slab(dz, u[2], o.h[2], &enter, &exit)) return miss();
    return enter <= exit ? enter : miss();
  }
  // cylinder: the z slab, then the circle in the xy plane
  if (!slab(dz, u[2], o.h[2], &enter, &exit)) return miss();
  const double r  = o.h[0];
  const double a  = (u[0] * u[0]) + u[1] * u[1];
  const double cc = ((dx * dx) + dy * dy) - r * r;
  if (a == 0.0) {  // a vertical beam stays at its distance from the axis
    if (!(cc <= 0.0)) return miss();
  } else {
    const double b    = (dx * u[0]) + dy * u[1];
    const double disc = b * b - a * cc;
    if (!(disc >= 0.0)) return miss();
    const double q = -b + sqrt(disc);
    if (cc <= 0.0) {  // within the radius: the circle bounds the far end only
      exit = mn(exit, q / a);
    } else {
      if (!(b < 0.0)) return miss();
      enter = mx(enter, cc / q);
      exit  = mn(exit, q / a);
    }
  }
  return enter <= exit ? enter : miss();
}

// the range at which a beam from height pz with vertical direction component uz meets the plane z = gz from above: 0 at or below it
MRS_OBST_HD double ground(double pz, double uz, double gz) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (pz <= gz) return 0.0;
  if (uz < 0.0) return (pz - gz) / (-uz);
  return miss();
}

// ---- scans that see other UAVs (include/mrs_swarm.h, "range scans that see other UAVs"; range_scan_uavs.hip) ----

// UAV j as a beam sees it: the closed sphere of radius rad = fl(arm_length + prop_radius) around its position q, as the sphere record that
// gate() and ray() above take (so a UAV and a spherical obstacle of equal centre and radius give equal bits)
MRS_OBST_HD mrs_obstacle_t uav_target(const double q[3], double rad) {
  mrs_obstacle_t o;
  o.kind     = MRS_OBST_SPHERE;
  o.world    = 0;
  o.flags    = 0u;
  o.reserved = 0u;
  o.c[0] = q[0], o.c[1] = q[1], o.c[2] = q[2];
  o.h[0] = rad, o.h[1] = 0.0, o.h[2] = 0.0;
  return o;
}

// the running lexicographic minimum of (t, j): (t, j) replaces (*best_t, *best_j) when it orders before it.  A NaN t is never taken
// (both comparisons are false).  Idempotent and associative: the order and the number of times the candidates arrive do not matter.
MRS_OBST_HD void take_uav(double t, int32_t j, double* best_t, int32_t* best_j) {
  if (t < *best_t || (t == *best_t && j < *best_j)) {
    *best_t = t;
    *best_j = j;
  }
}

}  // namespace mrs_scan
