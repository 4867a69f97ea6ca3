// obstacle_grid.h — the pure functions of the static obstacles (include/mrs_swarm.h, "static obstacles"; obstacles.hip): validation of a
// set, the signed distance and offset of one obstacle as the contract states them, the cell coordinate of a value, and the host-side
// builder of the search grid, and the definition of how a kernel reads that grid: GridView, which every kernel's arguments embed, and
// walk_cell(), the cell walk of both range scans (range_scan_common.h; obst_search of obstacles.hip keeps the same steps as a loop of
// its own and says why).  No GPU call, so that all of it is exercised without one (tests/cpp/obstacle_grid_test.cpp,
// tests/cpp/obstacle_walk_test.cpp); eval(), cell_coord() and walk_cell() are the very functions the kernels call.
//
// The grid: cubic cells of one edge over the bounding box of the solids.  A cell lists every obstacle whose axis-aligned bounding
// box, grown by `grow` on every side, overlaps the cell, so a query reads ONE cell, the one that contains p — no 27 probes, no
// deduplication.  Why that is conservative:
//   * every sd of eval() is at least the per-axis distance to the obstacle's bounding box: sqrt of a sum of squares is at least each
//     |term| (sums of non-negatives and sqrt round monotonically, sqrt(x*x) == |x|), so sd < radius implies fl(|fl(p_a - c_a)| - h_a) <
//     radius on every axis, hence |fl(p_a - c_a)| < h_a + radius exactly and |p_a - c_a| <= (h_a + radius)(1 + 2^-52);
//   * grow = radius (1 + 1e-6) + 2^-50 ((|c_a| + h_a) + radius): the second term covers that rounding and the two of forming the bounds
//     whatever the magnitudes are (it is below 1e-6 radius unless a coordinate exceeds about 1e9 radii), so lo_a <= p_a <= hi_a as doubles;
//   * cell_coord() is one monotone expression, floor((v - org) * inv_edge) clamped to [0, dim), evaluated in FP64 without contraction by
//     the builder (for lo_a, hi_a) and by the kernel (for p_a): lo_a <= p_a <= hi_a gives cell(lo_a) <= cell(p_a) <= cell(hi_a).  The
//     clamp on both sides keeps infinite pillars (lo = -inf, hi = +inf) and UAVs outside the grid correct.
// The kernel still tests sd < radius and the world rule literally for every listed obstacle: the grid only limits what is tested, and
// correctness depends on neither the edge nor the extent.  Sizing: the grid spans the solids (not their grown boxes: the border cells take what lies outside), but no further from the median centre
// than 4 x the 90 % quantile of the centres' distance from it (outliers are reached through the clamp); edge = MRS_OBST_EDGE_FACTOR *
// radius (2), at least extent / MAX_DIM, doubled until the grid has at most MAX_CELLS cells and its lists together at most
// item_cap(count) = 32 count + 65536 entries (one cell always fits).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/mrs_swarm.h"

#if defined(__HIPCC__)
#define MRS_OBST_HD __host__ __device__ __forceinline__
#else
#define MRS_OBST_HD inline
#endif
#ifndef MRS_OBST_EDGE_FACTOR
#define MRS_OBST_EDGE_FACTOR 2.0
#endif

namespace mrs_obst {

constexpr double  GROW_MARGIN = 1e-6;
constexpr double  ULP_SLACK   = 0x1p-50;
constexpr double  FAR         = 1e12;     // bounds beyond +-FAR do not stretch the grid (their cells are reached through the clamp)
constexpr int     MAX_DIM     = 256;      // cells per axis
constexpr int64_t MAX_CELLS   = 1 << 21;
inline int64_t    item_cap(int64_t count) { return 32 * count + 65536; }

// what a query needs to find its cell (handed to the kernels by value)
struct Grid {
  double  org[3];
  double  inv_edge;
  int32_t dim[3];
  int32_t pad;
};

// the contract's max and min: comparisons, not fmax / fmin (signed zeros follow the comparison, as numpy's where does)
MRS_OBST_HD double mx(double a, double b) { return a < b ? b : a; }
MRS_OBST_HD double mn(double a, double b) { return b < a ? b : a; }

// cell coordinate of the value v on an axis with origin org: monotone in v; NaN and everything below the grid -> 0
MRS_OBST_HD int cell_coord(double v, double org, double inv_edge, int dim) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double c = floor((v - org) * inv_edge);
  return !(c > 0.0) ? 0 : (c < (double)(dim - 1) ? (int)c : dim - 1);
}
MRS_OBST_HD int64_t cell_of(const Grid& g, double x, double y, double z) {
  const int cx = cell_coord(x, g.org[0], g.inv_edge, g.dim[0]), cy = cell_coord(y, g.org[1], g.inv_edge, g.dim[1]),
            cz = cell_coord(z, g.org[2], g.inv_edge, g.dim[2]);
  return ((int64_t)cz * g.dim[1] + cy) * g.dim[0] + cx;
}

// what a kernel needs to read a grid and the set it indexes (handed to the kernels by value; obstacle_set.h fills it)
struct GridView {
  Grid                  g;
  const int32_t *       start, *items;  // [cells + 1], [n_items]
  const mrs_obstacle_t* obst;           // [m]
  int32_t               m, n_items;
};

// The cell walk: visit(j, record) for every obstacle listed in the one cell that contains p, in list order
// (indices ascend), that an observer with world label myw sees.  Reads nothing outside the arrays whatever they hold: the cell lies
// inside the grid by the clamp of cell_coord (NaN -> 0), the list bounds are clamped to [0, n_items], an item that is no index of the
// set is skipped.  Whether to walk at all (m > 0, p finite) is the caller's decision.
template <class Visit>
MRS_OBST_HD void walk_cell(const GridView& v, const double p[3], uint32_t myw, Visit&& visit) {
  const int64_t q  = cell_of(v.g, p[0], p[1], p[2]);
  const int     s0 = v.start[q], s1 = v.start[q + 1];
  const int     beg = s0 > 0 ? s0 : 0, end = s1 < v.n_items ? s1 : v.n_items;
  for (int s = beg; s < end; s++) {
    const int j = v.items[s];
    if ((unsigned)j >= (unsigned)v.m) continue;
    const mrs_obstacle_t o = v.obst[j];
    if (!(o.flags & (uint32_t)MRS_OBST_ALL_WORLDS) && (uint32_t)o.world != myw) continue;  // another world's obstacle
    visit(j, o);
  }
}

// signed distance of the point p to obstacle o, and the offset rel from p to the closest point of the solid (zero inside), as
// include/mrs_swarm.h states them: FP64, one rounding per operation (the units that include this are compiled without contraction)
MRS_OBST_HD double eval(const mrs_obstacle_t& o, const double p[3], double rel[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double dx = p[0] - o.c[0], dy = p[1] - o.c[1], dz = p[2] - o.c[2];
  if (o.kind == MRS_OBST_SPHERE) {
    const double r = o.h[0], rho = sqrt(((dx * dx) + dy * dy) + dz * dz);
    const double t = rho > r ? (r / rho - 1.0) : 0.0;
    rel[0] = t * dx, rel[1] = t * dy, rel[2] = t * dz;
    return rho - r;
  }
  if (o.kind == MRS_OBST_BOX) {
    const double a0 = fabs(dx) - o.h[0], a1 = fabs(dy) - o.h[1], a2 = fabs(dz) - o.h[2];
    const double m0 = mx(a0, 0.0), m1 = mx(a1, 0.0), m2 = mx(a2, 0.0);
    rel[0] = mn(mx(dx, -o.h[0]), o.h[0]) - dx;
    rel[1] = mn(mx(dy, -o.h[1]), o.h[1]) - dy;
    rel[2] = mn(mx(dz, -o.h[2]), o.h[2]) - dz;
    return sqrt(((m0 * m0) + m1 * m1) + m2 * m2) + mn(mx(a0, mx(a1, a2)), 0.0);
  }
  const double r = o.h[0], hz = o.h[2], rho = sqrt((dx * dx) + dy * dy);
  const double ar = rho - r, az = fabs(dz) - hz;
  const double mr = mx(ar, 0.0), mz = mx(az, 0.0);
  const double t = rho > r ? (r / rho - 1.0) : 0.0;
  rel[0] = t * dx, rel[1] = t * dy, rel[2] = mn(mx(dz, -hz), hz) - dz;
  return sqrt((mr * mr) + mz * mz) + mn(mx(ar, az), 0.0);
}

// half-extents of the bounding box of o
MRS_OBST_HD void half_extents(const mrs_obstacle_t& o, double h[3]) {
  if (o.kind == MRS_OBST_BOX)
    h[0] = o.h[0], h[1] = o.h[1], h[2] = o.h[2];
  else if (o.kind == MRS_OBST_SPHERE)
    h[0] = h[1] = h[2] = o.h[0];
  else
    h[0] = h[1] = o.h[0], h[2] = o.h[2];
}

// nullptr for a valid obstacle, else what is wrong with it
inline const char* invalid(const mrs_obstacle_t& o) {
  if (o.kind != MRS_OBST_SPHERE && o.kind != MRS_OBST_BOX && o.kind != MRS_OBST_CYLINDER) return "unknown obstacle kind";
  if (o.flags & ~(uint32_t)MRS_OBST_ALL_WORLDS) return "unknown obstacle flag bits";
  if (o.reserved != 0u) return "reserved must be 0";
  for (int a = 0; a < 3; a++)
    if (!isfinite(o.c[a])) return "obstacle centre must be finite";
  const bool used[3] = {true, o.kind == MRS_OBST_BOX, o.kind != MRS_OBST_SPHERE};
  for (int a = 0; a < 3; a++) {
    if (!used[a]) continue;
    const bool pillar = o.kind == MRS_OBST_CYLINDER && a == 2 && o.h[a] == INFINITY;
    if (!pillar && !(isfinite(o.h[a]) && o.h[a] >= 0.0)) return "obstacle sizes must be finite and >= 0 (a cylinder's half-height may be +inf)";
  }
  return nullptr;
}

// bounds of o's bounding box grown for `radius` (see the head of the file); +-inf for a pillar's ends
inline void grown_box(const mrs_obstacle_t& o, double radius, double lo[3], double hi[3]) {
  double h[3];
  half_extents(o, h);
  for (int a = 0; a < 3; a++) {
    const double g = radius * (1.0 + GROW_MARGIN) + ULP_SLACK * ((fabs(o.c[a]) + h[a]) + radius);
    lo[a] = (o.c[a] - h[a]) - g;
    hi[a] = (o.c[a] + h[a]) + g;
  }
}

struct Built {
  Grid                 g{};
  double               radius = 0.0, edge = 0.0;
  std::vector<int32_t> start;  // [cells + 1]: list of cell q = items[start[q] .. start[q + 1])
  std::vector<int32_t> items;  // obstacle indices, ascending within a cell
  int32_t              longest = 0;
  int64_t              cells() const { return (int64_t)g.dim[0] * g.dim[1] * g.dim[2]; }
};

// cell ranges [c0, c1] per axis of a grown box
inline void cell_range(const Grid& g, const double lo[3], const double hi[3], int c0[3], int c1[3]) {
  for (int a = 0; a < 3; a++) {
    c0[a] = cell_coord(lo[a], g.org[a], g.inv_edge, g.dim[a]);
    c1[a] = cell_coord(hi[a], g.org[a], g.inv_edge, g.dim[a]);
  }
}

// the grid of `count` valid obstacles for queries of `radius` (finite, > 0); cap_items / max_cells: the sizing limits (tests lower them to
// force the coarsening path)
inline Built build(const mrs_obstacle_t* obst, int32_t count, double radius, int64_t cap_items = -1, int64_t max_cells = MAX_CELLS) {
  if (cap_items < 0) cap_items = item_cap(count);
  if (cap_items < count) cap_items = count;  // (one cell holds every obstacle once)
  if (max_cells < 1) max_cells = 1;
  Built b;
  b.radius = radius;
  std::vector<double> lo((size_t)count * 3), hi((size_t)count * 3);
  double blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int32_t j = 0; j < count; j++) {
    grown_box(obst[j], radius, &lo[(size_t)j * 3], &hi[(size_t)j * 3]);
    double he[3];
    half_extents(obst[j], he);
    for (int a = 0; a < 3; a++) {  // the grid spans the solids themselves: what a grown box adds beyond them lands in the border cells
      const double l = obst[j].c[a] - he[a], h = obst[j].c[a] + he[a];
      if (fabs(l) <= FAR && l < blo[a]) blo[a] = l;
      if (fabs(h) <= FAR && h > bhi[a]) bhi[a] = h;
    }
  }
  double ext[3];
  std::vector<double> v((size_t)count);
  for (int a = 0; a < 3; a++) {
    if (count > 0) {  // a few outliers (a far obstacle, a huge one) do not stretch the grid: it reaches 4 x the 90 % quantile of the
                      // centres' distance from their median (all of a uniform scene); what lies beyond is reached through the clamp
      for (int32_t j = 0; j < count; j++) v[(size_t)j] = obst[j].c[a];
      std::nth_element(v.begin(), v.begin() + count / 2, v.end());
      const double med = v[(size_t)count / 2];
      for (int32_t j = 0; j < count; j++) v[(size_t)j] = fabs(obst[j].c[a] - med);
      const size_t q90 = (size_t)ceil(0.9 * (double)(count - 1));
      std::nth_element(v.begin(), v.begin() + (long)q90, v.end());
      const double reach = 4.0 * v[q90] + 2.0 * radius;
      blo[a] = mx(blo[a], med - reach);
      bhi[a] = mn(bhi[a], med + reach);
    }
    if (!(blo[a] <= bhi[a])) blo[a] = bhi[a] = (blo[a] <= FAR ? blo[a] : (bhi[a] >= -FAR ? bhi[a] : 0.0));  // no bound, or one: a single layer
    b.g.org[a] = blo[a];
    ext[a]     = bhi[a] - blo[a];
  }
  double edge = MRS_OBST_EDGE_FACTOR * radius;
  for (int a = 0; a < 3; a++) edge = mx(edge, ext[a] / (double)MAX_DIM);  // (MAX_DIM cells span the set: the clamp is for what lies outside)
  for (;;) {
    b.g.inv_edge = 1.0 / edge;
    for (int a = 0; a < 3; a++) {
      const double d = ceil(ext[a] * b.g.inv_edge);
      b.g.dim[a]     = !(d >= 1.0) ? 1 : (d < (double)MAX_DIM ? (int)d : MAX_DIM);
    }
    int64_t items = 0;
    for (int32_t j = 0; j < count && items <= cap_items; j++) {
      int c0[3], c1[3];
      cell_range(b.g, &lo[(size_t)j * 3], &hi[(size_t)j * 3], c0, c1);
      items += (int64_t)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
    }
    if ((b.cells() <= max_cells && items <= cap_items) || b.cells() == 1) break;
    edge *= 2.0;
  }
  b.edge = edge;
  const int64_t cells = b.cells();
  b.start.assign((size_t)cells + 1, 0);
  for (int pass = 0; pass < 2; pass++) {  // count, then fill (obstacles in index order: every list ascends)
    for (int32_t j = 0; j < count; j++) {
      int c0[3], c1[3];
      cell_range(b.g, &lo[(size_t)j * 3], &hi[(size_t)j * 3], c0, c1);
      for (int z = c0[2]; z <= c1[2]; z++)
        for (int y = c0[1]; y <= c1[1]; y++)
          for (int x = c0[0]; x <= c1[0]; x++) {
            const size_t q = (size_t)(((int64_t)z * b.g.dim[1] + y) * b.g.dim[0] + x);
            if (pass == 0)
              b.start[q + 1]++;
            else
              b.items[(size_t)b.start[q]++] = j;
          }
    }
    if (pass == 0) {
      for (int64_t q = 0; q < cells; q++) {
        if (b.start[(size_t)q + 1] > b.longest) b.longest = b.start[(size_t)q + 1];
        b.start[(size_t)q + 1] += b.start[(size_t)q];
      }
      b.items.assign((size_t)b.start[(size_t)cells], 0);
    } else {  // the fill advanced start[q] to the end of list q: shift back
      for (int64_t q = cells; q > 0; q--) b.start[(size_t)q] = b.start[(size_t)q - 1];
      b.start[0] = 0;
    }
  }
  return b;
}

}  // namespace mrs_obst
