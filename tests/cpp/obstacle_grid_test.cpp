// obstacle_grid_test.cpp — the pure host functions of the static obstacles (mrs_multirotor_simulator_amd/csrc/obstacle_grid.h) without a
// GPU: validation, the cell coordinate, and above all that the grid is CONSERVATIVE — for random sets (spheres, boxes, cylinders, huge
// boxes, pillars without ends, obstacles far from the rest) and random points (near the obstacles, just inside and just outside the
// radius of a face, far outside the grid), every obstacle with sd < radius for a point is listed in that point's one cell.  Also the
// coarsening path (lowered caps), the empty set and the shape of the lists.  Built by tests/test_obstacles.py with the host compiler,
// -ffp-contract=off and -fsanitize=address,undefined, and run directly.  Exit code 0 and "ok ..." lines on success.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../mrs_multirotor_simulator_amd/csrc/obstacle_grid.h"

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                  \
    }                                                            \
  } while (0)

using namespace mrs_obst;

static mrs_obstacle_t make(int kind, double x, double y, double z, double h0, double h1, double h2, int world = 0, unsigned flags = 0) {
  mrs_obstacle_t o;
  std::memset(&o, 0, sizeof o);
  o.kind = kind, o.world = world, o.flags = flags;
  o.c[0] = x, o.c[1] = y, o.c[2] = z;
  o.h[0] = h0, o.h[1] = h1, o.h[2] = h2;
  return o;
}

static int check_functions() {
  static_assert(sizeof(mrs_obstacle_t) == 64, "mrs_obstacle_t is 64 B");
  static_assert(sizeof(mrs_obstacle_stats_t) == 64, "mrs_obstacle_stats_t is 64 B");
  const double inf = INFINITY, nan = NAN;
  CHECK(!invalid(make(MRS_OBST_SPHERE, 1, 2, 3, 0.5, nan, -1)));  // a sphere's h[1], h[2] are not used
  CHECK(!invalid(make(MRS_OBST_BOX, 1, 2, 3, 0, 0, 0)));
  CHECK(!invalid(make(MRS_OBST_CYLINDER, 1, 2, 3, 0.5, nan, inf)));
  CHECK(!invalid(make(MRS_OBST_SPHERE, 0, 0, 0, 1, 0, 0, -7, MRS_OBST_ALL_WORLDS)));
  CHECK(invalid(make(3, 0, 0, 0, 1, 1, 1)) && invalid(make(-1, 0, 0, 0, 1, 1, 1)));
  CHECK(invalid(make(MRS_OBST_SPHERE, 0, 0, 0, 1, 1, 1, 0, 2u)));
  CHECK(invalid(make(MRS_OBST_SPHERE, nan, 0, 0, 1, 1, 1)) && invalid(make(MRS_OBST_BOX, 0, inf, 0, 1, 1, 1)));
  CHECK(invalid(make(MRS_OBST_SPHERE, 0, 0, 0, -1e-9, 1, 1)) && invalid(make(MRS_OBST_SPHERE, 0, 0, 0, inf, 1, 1)));
  CHECK(invalid(make(MRS_OBST_BOX, 0, 0, 0, 1, 1, inf)) && invalid(make(MRS_OBST_BOX, 0, 0, 0, 1, nan, 1)));
  CHECK(invalid(make(MRS_OBST_CYLINDER, 0, 0, 0, inf, 0, 1)) && invalid(make(MRS_OBST_CYLINDER, 0, 0, 0, 1, 0, -inf)));
  mrs_obstacle_t r = make(MRS_OBST_BOX, 0, 0, 0, 1, 1, 1);
  r.reserved = 1;
  CHECK(invalid(r));
  // the cell coordinate: clamped on both sides, NaN -> 0, monotone
  CHECK(cell_coord(-inf, 0.0, 0.5, 10) == 0 && cell_coord(inf, 0.0, 0.5, 10) == 9 && cell_coord(nan, 0.0, 0.5, 10) == 0);
  CHECK(cell_coord(-1e300, 3.0, 0.5, 10) == 0 && cell_coord(1e300, 3.0, 0.5, 10) == 9 && cell_coord(1e308, -1e308, 1e10, 7) == 6);
  CHECK(cell_coord(3.0, 3.0, 2.0, 10) == 0 && cell_coord(4.999, 3.0, 2.0, 10) == 3 && cell_coord(5.0, 3.0, 2.0, 10) == 4);
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> u(-40.0, 40.0);
  for (int t = 0; t < 20000; t++) {
    double a = u(rng), b = t % 3 ? u(rng) : std::nextafter(a, inf);
    if (b < a) std::swap(a, b);
    CHECK(cell_coord(a, -7.3, 1.0 / 3.7, 19) <= cell_coord(b, -7.3, 1.0 / 3.7, 19));
  }
  // signed distances with known answers
  double       rel[3];
  const double p[3] = {3.0, 0.0, 4.0};
  CHECK(eval(make(MRS_OBST_SPHERE, 0, 0, 0, 1, 0, 0), p, rel) == 4.0 && rel[0] == (1.0 / 5.0 - 1.0) * 3.0 && rel[1] == 0.0);
  CHECK(eval(make(MRS_OBST_BOX, 0, 0, 0, 1, 1, 1), p, rel) == std::sqrt(4.0 + 9.0) && rel[0] == -2.0 && rel[1] == 0.0 && rel[2] == -3.0);
  CHECK(eval(make(MRS_OBST_CYLINDER, 0, 0, 0, 1, 0, inf), p, rel) == 2.0 && rel[2] == 0.0);
  CHECK(eval(make(MRS_OBST_CYLINDER, 0, 0, 0, 5, 0, 6), p, rel) == -2.0 && rel[0] == 0.0 && rel[2] == 0.0);
  std::printf("ok functions\n");
  return 0;
}

// every obstacle with sd < radius at p is in p's cell; returns how many there were (-1: one was missing)
static long covered(const std::vector<mrs_obstacle_t>& set, const Built& b, double radius, const double p[3]) {
  const int64_t q = cell_of(b.g, p[0], p[1], p[2]);
  if (q < 0 || q >= b.cells()) return -1;
  long hits = 0;
  for (size_t j = 0; j < set.size(); j++) {
    double       rel[3];
    const double sd = eval(set[j], p, rel);
    if (!(sd < radius)) continue;
    hits++;
    bool listed = false;
    for (int32_t s = b.start[(size_t)q]; s < b.start[(size_t)q + 1]; s++) listed = listed || b.items[(size_t)s] == (int32_t)j;
    if (!listed) {
      std::printf("obstacle %zu (kind %d) with sd %.17g < %.17g missing from cell %lld of (%.17g, %.17g, %.17g)\n", j, set[j].kind, sd, radius,
                  (long long)q, p[0], p[1], p[2]);
      return -1;
    }
  }
  return hits;
}

static int well_formed(const Built& b, size_t count) {
  const int64_t cells = b.cells();
  CHECK(cells >= 1 && (int64_t)b.start.size() == cells + 1 && b.start[0] == 0 && b.start[(size_t)cells] == (int32_t)b.items.size());
  int32_t longest = 0;
  for (int64_t q = 0; q < cells; q++) {
    const int32_t beg = b.start[(size_t)q], end = b.start[(size_t)q + 1];
    CHECK(beg <= end);
    longest = std::max(longest, end - beg);
    for (int32_t s = beg; s < end; s++) {
      CHECK(b.items[(size_t)s] >= 0 && (size_t)b.items[(size_t)s] < count);
      CHECK(s == beg || b.items[(size_t)s - 1] < b.items[(size_t)s]);  // ascending: no obstacle twice in a cell
    }
  }
  CHECK(longest == b.longest);
  for (int a = 0; a < 3; a++) CHECK(b.g.dim[a] >= 1 && b.g.dim[a] <= MAX_DIM);
  CHECK(b.g.inv_edge == 1.0 / b.edge && b.edge >= MRS_OBST_EDGE_FACTOR * b.radius);
  return 0;
}

static int check_random(bool coarsen) {
  std::mt19937_64                        rng(coarsen ? 77 : 42);
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  long                                   hits = 0, points = 0, grids_coarsened = 0, multi = 0;
  for (int round = 0; round < 24; round++) {
    const int    count  = 1 + (int)(u01(rng) * 300);
    const double side   = 20.0 + 200.0 * u01(rng);
    const double radius = round % 6 == 5 ? 1e-3 : 0.5 + 6.0 * u01(rng);
    std::vector<mrs_obstacle_t> set;
    for (int j = 0; j < count; j++) {
      const int    kind = (int)(u01(rng) * 3) % 3;
      const double x = side * (u01(rng) - 0.5), y = side * (u01(rng) - 0.5), z = 0.2 * side * u01(rng);
      double       h0 = 0.1 + 2.0 * u01(rng), h1 = 0.1 + 2.0 * u01(rng), h2 = 0.1 + 4.0 * u01(rng);
      const double sel = u01(rng);
      if (sel < 0.03) h0 = 1e7 * u01(rng), h1 = 1e3 * u01(rng);                        // a huge box / sphere / cylinder
      if (sel > 0.97) h0 = 0.0, h1 = 0.0, h2 = 0.0;                                    // a point
      if (kind == MRS_OBST_CYLINDER && u01(rng) < 0.5) h2 = INFINITY;                  // a pillar without ends
      set.push_back(make(kind, x, y, z, h0, h1, h2));
      if (sel > 0.45 && sel < 0.47) set.back().c[0] = 1e9 * (u01(rng) - 0.5);           // far from the rest
      if (sel > 0.47 && sel < 0.48) set.back().c[2] = -3e13;                           // beyond what stretches the grid
      CHECK(!invalid(set.back()));
    }
    const Built b = coarsen ? build(set.data(), count, radius, count + (int64_t)(u01(rng) * 3 * count), 1 + (int64_t)(u01(rng) * 500))
                            : build(set.data(), count, radius);
    if (well_formed(b, set.size())) return 1;
    grids_coarsened += b.edge > MRS_OBST_EDGE_FACTOR * radius * 1.5;
    multi += b.g.dim[0] > 1 && b.g.dim[1] > 1;
    if (!coarsen) CHECK((int64_t)b.items.size() <= item_cap(count) && b.cells() <= MAX_CELLS);
    for (int t = 0; t < 1500; t++) {
      double p[3];
      const int mode = t % 5;
      if (mode == 0) {  // anywhere around the scene
        for (int a = 0; a < 3; a++) p[a] = 1.5 * side * (u01(rng) - 0.5);
      } else if (mode == 4) {  // far outside the grid
        for (int a = 0; a < 3; a++) p[a] = (u01(rng) < 0.5 ? -1.0 : 1.0) * std::pow(10.0, 3.0 + 12.0 * u01(rng));
        if (t % 2) p[2] = 1.0;
      } else {  // at a face of an obstacle's bounding box: about `radius` outside it (mode 1: just inside, 2: just outside), or anywhere within it
        const mrs_obstacle_t& o = set[(size_t)(u01(rng) * count) % (size_t)count];
        double                h[3];
        half_extents(o, h);
        for (int a = 0; a < 3; a++) p[a] = o.c[a] + (std::isfinite(h[a]) ? h[a] : 50.0) * (2.0 * u01(rng) - 1.0);
        const int    a = (int)(u01(rng) * 3) % 3;
        const double f = mode == 1 ? 1.0 - 1e-15 * (t % 7) : (mode == 2 ? 1.0 + 1e-15 * (t % 7) : u01(rng));
        if (std::isfinite(h[a])) p[a] = o.c[a] + (u01(rng) < 0.5 ? -1.0 : 1.0) * (h[a] + radius * f);
      }
      const long c = covered(set, b, radius, p);
      CHECK(c >= 0);
      hits += c;
      points++;
    }
  }
  CHECK(hits > points / 4);  // (the points do meet obstacles)
  CHECK(multi > 12);
  if (coarsen) CHECK(grids_coarsened > 12);
  std::printf("ok %s %ld %ld\n", coarsen ? "coarsened" : "random", points, hits);
  return 0;
}

static int check_empty_and_single() {
  const Built e = build(nullptr, 0, 5.0);
  CHECK(e.cells() == 1 && e.start.size() == 2 && e.start[0] == 0 && e.start[1] == 0 && e.items.empty() && e.longest == 0);
  const double far[3] = {1e9, -1e9, 3.0};
  CHECK(cell_of(e.g, far[0], far[1], far[2]) == 0 && cell_of(e.g, NAN, 0.0, 0.0) == 0);
  // one pillar: a single layer in z, every z lands in it
  std::vector<mrs_obstacle_t> one{make(MRS_OBST_CYLINDER, 2.0, 3.0, 0.0, 0.5, 0.0, INFINITY)};
  const Built                 b = build(one.data(), 1, 2.0);
  CHECK(b.g.dim[2] == 1 && well_formed(b, 1) == 0);
  for (double z : {-1e30, -5.0, 0.0, 7.0, 1e30}) {
    const double p[3] = {2.0, 4.0, z};
    CHECK(covered(one, b, 2.0, p) == 1);
  }
  // a grid of pillars 10 m apart, radius 2: several cells per axis and short lists
  std::vector<mrs_obstacle_t> forest;
  for (int i = 0; i < 100; i++) forest.push_back(make(MRS_OBST_CYLINDER, 10.0 * (i % 10), 10.0 * (i / 10), 0.0, 0.3, 0.0, INFINITY));
  const Built f = build(forest.data(), 100, 2.0);
  CHECK(f.g.dim[0] > 10 && f.g.dim[1] > 10 && f.g.dim[2] == 1 && f.longest <= 4 && well_formed(f, 100) == 0);
  std::printf("ok empty_and_single\n");
  return 0;
}

// obstacle_grid_test SET RADIUS: the grid the library would build for the obstacle records of the file SET (tests/test_obstacles.py)
static int describe(const char* path, double radius) {
  std::vector<mrs_obstacle_t> set;
  FILE*                       f = std::fopen(path, "rb");
  CHECK(f);
  mrs_obstacle_t o;
  while (std::fread(&o, sizeof o, 1, f) == 1) set.push_back(o);
  std::fclose(f);
  for (const mrs_obstacle_t& e : set) CHECK(!invalid(e));
  CHECK(radius > 0.0 && std::isfinite(radius));
  const Built b = build(set.data(), (int32_t)set.size(), radius);
  if (well_formed(b, set.size())) return 1;
  std::printf("grid dims %d %d %d cells %lld items %zu longest %d edge %.17g\n", b.g.dim[0], b.g.dim[1], b.g.dim[2], (long long)b.cells(),
              b.items.size(), b.longest, b.edge);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3) return describe(argv[1], std::atof(argv[2]));
  if (check_functions() || check_empty_and_single() || check_random(false) || check_random(true)) return 1;
  std::printf("ok all\n");
  return 0;
}
