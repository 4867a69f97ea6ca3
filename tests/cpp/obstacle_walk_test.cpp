// obstacle_walk_test.cpp — the cell walk of the obstacle queries and the range scans (mrs_obst::walk_cell of
// mrs_multirotor_simulator_amd/csrc/obstacle_grid.h) without a GPU: this is the function the kernels of range_scan.hip and
// range_scan_uavs.hip call (obst_search of obstacles.hip has the same steps as a loop of its own), so this checks the device function's
// text on the CPU.  A dozen obstacles of the three kinds in two worlds, one
// of them for all worlds, in the grid mrs_obst::build makes; query points in every cell, outside the grid on each side and with a NaN
// coordinate: the callable receives exactly the indices of the cell's list that the observer's world sees, ascending, each with its own
// record, and every obstacle within the radius is among them.  Then damaged arrays (an item of m, an item of -1, a start entry below 0, a
// start entry above n_items): nothing outside the arrays is read — they are heap blocks of the exact size, so the address sanitizer
// would see it — and the bad items are skipped.  Then m == 0 with a caller that does not guard.  Built by tests/test_obstacles.py with
// the host compiler, -ffp-contract=off and -fsanitize=address,undefined, and run directly.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../mrs_multirotor_simulator_amd/csrc/obstacle_grid.h"

using mrs_obst::GridView;

static int failures = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      std::printf("FAILED %s: ", #cond);  \
      std::printf(__VA_ARGS__);           \
      std::printf("\n");                  \
      failures++;                         \
    }                                     \
  } while (0)

static mrs_obstacle_t make(int kind, double x, double y, double z, double h0, double h1, double h2, int world, uint32_t flags) {
  mrs_obstacle_t o;
  std::memset(&o, 0, sizeof o);
  o.kind = kind, o.world = world, o.flags = flags;
  o.c[0] = x, o.c[1] = y, o.c[2] = z;
  o.h[0] = h0, o.h[1] = h1, o.h[2] = h2;
  return o;
}

static bool sees(const mrs_obstacle_t& o, uint32_t myw) { return (o.flags & (uint32_t)MRS_OBST_ALL_WORLDS) || (uint32_t)o.world == myw; }

// what the walk must visit, from the arrays as vectors (every access checked), with the clamps the contract states
static std::vector<int> expected(const mrs_obst::Grid& g, const std::vector<int32_t>& start, const std::vector<int32_t>& items,
                                 const std::vector<mrs_obstacle_t>& ob, int32_t m, const double p[3], uint32_t myw) {
  const int64_t q = mrs_obst::cell_of(g, p[0], p[1], p[2]);
  long long     beg = start.at((size_t)q), end = start.at((size_t)q + 1);
  if (beg < 0) beg = 0;
  if (end > (long long)items.size()) end = (long long)items.size();
  std::vector<int> out;
  for (long long s = beg; s < end; s++) {
    const int j = items.at((size_t)s);
    if (j < 0 || j >= m) continue;
    if (sees(ob.at((size_t)j), myw)) out.push_back(j);
  }
  return out;
}

// walks p for myw and compares with `want`; the record handed over is that of the index
static void walk_and_compare(const GridView& v, const std::vector<mrs_obstacle_t>& ob, const double p[3], uint32_t myw, const std::vector<int>& want,
                             const char* what) {
  std::vector<int> got;
  bool             own_record = true;
  mrs_obst::walk_cell(v, p, myw, [&](int j, const mrs_obstacle_t& o) {
    got.push_back(j);
    own_record = own_record && j >= 0 && j < (int)ob.size() && std::memcmp(&o, &ob[(size_t)j], sizeof o) == 0;
  });
  CHECK(got == want, "%s at (%g, %g, %g) world %u: %zu visited, %zu expected", what, p[0], p[1], p[2], myw, got.size(), want.size());
  CHECK(own_record, "%s at (%g, %g, %g): a visit with another obstacle's record", what, p[0], p[1], p[2]);
}

int main() {
  const double                radius = 1.5;
  std::vector<mrs_obstacle_t> ob;
  for (int j = 0; j < 12; j++) {  // kinds in turn; worlds 0 and 5 in turn; a pillar; obstacle 7 for all worlds
    const double x = -9.0 + 5.5 * (j % 4) + 0.3 * j, y = -6.0 + 6.0 * ((j / 4) % 3) + 0.2 * j, z = 1.0 + 1.7 * (j % 5);
    ob.push_back(make(j % 3, x, y, z, 0.6 + 0.1 * j, 0.9, j == 5 ? INFINITY : 1.2, j % 2 ? 5 : 0, 0u));
  }
  ob[7].flags = MRS_OBST_ALL_WORLDS, ob[7].world = 77;
  ob[10].c[0] = ob[2].c[0] + 0.4, ob[10].c[1] = ob[2].c[1], ob[10].c[2] = ob[2].c[2];  // two that overlap: a list of several entries
  const int32_t m = (int32_t)ob.size();
  for (const mrs_obstacle_t& o : ob) CHECK(mrs_obst::invalid(o) == nullptr, "the scene holds an invalid obstacle");
  const mrs_obst::Built b = mrs_obst::build(ob.data(), m, radius);
  CHECK(b.g.dim[0] > 2 && b.g.dim[1] > 2 && b.g.dim[2] > 1 && b.longest >= 2, "grid %d x %d x %d, longest list %d", b.g.dim[0], b.g.dim[1], b.g.dim[2],
        b.longest);
  const GridView v{b.g, b.start.data(), b.items.data(), ob.data(), m, (int32_t)b.items.size()};

  // query points: the centre of every cell, a point outside the grid on each side, a NaN in each coordinate
  std::vector<std::vector<double>> pts;
  const double                     edge = b.edge;
  for (int z = 0; z < b.g.dim[2]; z++)
    for (int y = 0; y < b.g.dim[1]; y++)
      for (int x = 0; x < b.g.dim[0]; x++) pts.push_back({b.g.org[0] + (x + 0.5) * edge, b.g.org[1] + (y + 0.5) * edge, b.g.org[2] + (z + 0.5) * edge});
  const size_t n_inside = pts.size();
  for (int a = 0; a < 3; a++)
    for (double side : {-1.0, 1.0}) {
      std::vector<double> p = {ob[2].c[0], ob[2].c[1], ob[2].c[2]};
      p[(size_t)a] = side < 0 ? b.g.org[a] - 1000.0 : b.g.org[a] + b.g.dim[a] * edge + 1000.0;
      pts.push_back(p);
    }
  for (int a = 0; a < 3; a++) {
    std::vector<double> p = {ob[7].c[0], ob[7].c[1], ob[7].c[2]};
    p[(size_t)a] = NAN;
    pts.push_back(p);
  }
  for (const mrs_obstacle_t& o : ob) pts.push_back({o.c[0] + 0.3, o.c[1] - 0.2, std::isfinite(o.h[2]) ? o.c[2] + 0.1 : 40.0});

  size_t visits = 0, nonempty = 0, filtered = 0;
  for (const std::vector<double>& p : pts)
    for (uint32_t myw : {0u, 5u, 9u}) {
      const std::vector<int> want = expected(b.g, b.start, b.items, ob, m, p.data(), myw);
      walk_and_compare(v, ob, p.data(), myw, want, "intact");
      for (size_t e = 1; e < want.size(); e++) CHECK(want[e - 1] < want[e], "the list of a cell does not ascend");
      visits += want.size();
      nonempty += !want.empty();
      const int64_t q = mrs_obst::cell_of(b.g, p[0], p[1], p[2]);
      filtered += (int)want.size() < b.start[(size_t)q + 1] - b.start[(size_t)q];
      // coverage: whatever lies within the radius and is seen is visited (finite points only: the callers guard the others)
      if (std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))
        for (int j = 0; j < m; j++) {
          double rel[3];
          if (sees(ob[(size_t)j], myw) && mrs_obst::eval(ob[(size_t)j], p.data(), rel) < radius)
            CHECK(std::find(want.begin(), want.end(), j) != want.end(), "obstacle %d within the radius of (%g, %g, %g) is not listed", j, p[0], p[1], p[2]);
        }
    }
  CHECK(visits > 40 && nonempty > 20 && filtered > 20, "%zu visits, %zu non-empty walks, %zu filtered by the world rule", visits, nonempty, filtered);
  {  // world 9 sees the all-worlds obstacle alone
    const double     p[3] = {ob[7].c[0], ob[7].c[1], ob[7].c[2]};
    std::vector<int> got;
    mrs_obst::walk_cell(v, p, 9u, [&](int j, const mrs_obstacle_t&) { got.push_back(j); });
    CHECK(got == std::vector<int>{7}, "world 9 at obstacle 7 visits %zu obstacles", got.size());
  }

  // damaged copies, each a heap block of the exact size
  const int64_t cells = b.cells();
  int64_t       q_two = -1, q_other = -1;  // two different cells with non-empty lists, the first with >= 2 entries
  for (int64_t q = 0; q < cells; q++) {
    const int len = b.start[(size_t)q + 1] - b.start[(size_t)q];
    if (len >= 2 && q_two < 0)
      q_two = q;
    else if (len >= 1 && q_two >= 0 && q_other < 0 && q > q_two + 1)
      q_other = q;
  }
  CHECK(q_two >= 0 && q_other > q_two + 1 && q_other + 2 < cells + 1, "cells to damage: %lld, %lld of %lld", (long long)q_two, (long long)q_other,
        (long long)cells);
  if (failures == 0) {
    std::vector<int32_t> start(b.start), items(b.items);
    items[(size_t)start[(size_t)q_two]]     = m;   // one past the set
    items[(size_t)start[(size_t)q_two] + 1] = -1;  // below it
    start[(size_t)q_other]                  = -5;  // the list of q_other begins below 0 (and that of q_other - 1 ends there)
    start[(size_t)q_other + 2]              = (int32_t)items.size() + 7;  // the list of q_other + 1 ends above n_items
    const GridView dv{b.g, start.data(), items.data(), ob.data(), m, (int32_t)items.size()};
    size_t         dvisits = 0;
    for (size_t k = 0; k < n_inside; k++)
      for (uint32_t myw : {0u, 5u}) {
        const std::vector<int> want = expected(b.g, start, items, ob, m, pts[k].data(), myw);
        walk_and_compare(dv, ob, pts[k].data(), myw, want, "damaged");
        dvisits += want.size();
      }
    CHECK(dvisits > 0, "the damaged walk visited nothing");
    // the two bad items are skipped, the rest of that list is visited
    const double* p = pts[(size_t)q_two].data();
    CHECK(mrs_obst::cell_of(b.g, p[0], p[1], p[2]) == q_two, "point %lld is not the centre of cell %lld", (long long)q_two, (long long)q_two);
    for (uint32_t myw : {0u, 5u}) {  // exactly the intact list without its first two entries, as far as myw sees them
      std::vector<int> rest, got;
      for (int s = b.start[(size_t)q_two] + 2; s < b.start[(size_t)q_two + 1]; s++)
        if (sees(ob[(size_t)b.items[(size_t)s]], myw)) rest.push_back(b.items[(size_t)s]);
      mrs_obst::walk_cell(dv, p, myw, [&](int j, const mrs_obstacle_t&) { got.push_back(j); });
      CHECK(got == rest, "cell %lld world %u: %zu visits, %zu expected behind the two bad items", (long long)q_two, myw, got.size(), rest.size());
    }
  }

  // m == 0 and a caller that does not guard: the empty set's own grid, and the arrays above with m = 0 and no records at all
  {
    const mrs_obst::Built e = mrs_obst::build(nullptr, 0, radius);
    const GridView        ev{e.g, e.start.data(), e.items.data(), nullptr, 0, (int32_t)e.items.size()};
    const GridView        zv{b.g, b.start.data(), b.items.data(), nullptr, 0, (int32_t)b.items.size()};
    int                   seen = 0;
    for (const std::vector<double>& p : pts) {
      mrs_obst::walk_cell(ev, p.data(), 0u, [&](int, const mrs_obstacle_t&) { seen++; });
      mrs_obst::walk_cell(zv, p.data(), 0u, [&](int, const mrs_obstacle_t&) { seen++; });
    }
    CHECK(e.cells() == 1 && e.items.empty() && seen == 0, "m == 0: %d visits", seen);
  }

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok obstacle_walk %zu points %zu visits\n", pts.size(), visits);
  return 0;
}
