// obstacle_contact_math_test.cpp — the pure functions of the obstacle contacts (mrs_multirotor_simulator_amd/csrc/obstacle_contact.h)
// without a GPU: the very functions k_obst_contact calls, so this checks the device function's text on the CPU.
//   functions  the radius and the threshold are one addition each, in that order; the fold at sd == thr, one ulp inside, with NaN on either
//              side, with ties (lower index, whatever the order of the visits) and with -0.0 against +0.0
//   random     random sets with huge boxes, pillars without ends and far obstacles, in the grid mrs_obst::build makes for R; query points
//              among the obstacles, far outside the grid and not finite, in three worlds, each with a threshold of its own <= R: the
//              search over the ONE cell that contains the point equals the fold over all obstacles, bit for bit
//   coarsened  the same with the sizing limits lowered until the grid coarsens, down to one cell, and with other R for the same thresholds:
//              the result depends on neither
//   listed     argv[1] (a set), argv[2] (points: x, y, z, thr, world) -> argv[3] (sd, index, count) for tests/test_obstacle_contacts.py
//              to compare with the numpy restatement
// Built by tests/test_obstacle_contacts.py with the host compiler, -ffp-contract=off and -fsanitize=address,undefined, and run directly.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../mrs_multirotor_simulator_amd/csrc/obstacle_contact.h"

using mrs_obst::Contact;
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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same(const Contact& a, const Contact& b) { return a.count == b.count && a.j == b.j && same_bits(a.sd, b.sd); }

struct Point {
  double   p[3], thr;
  uint32_t world, pad;
};
struct Result {
  double  sd;
  int32_t index, count;
};

// the definition: every obstacle of the set, in descending order (the search visits ascending ones)
static Contact brute(const std::vector<mrs_obstacle_t>& ob, const Point& q) {
  Contact c = mrs_obst::contact_none();
  if (!(std::isfinite(q.p[0]) && std::isfinite(q.p[1]) && std::isfinite(q.p[2]))) return c;
  for (int j = (int)ob.size() - 1; j >= 0; j--) {
    const mrs_obstacle_t& o = ob[(size_t)j];
    if (!(o.flags & (uint32_t)MRS_OBST_ALL_WORLDS) && (uint32_t)o.world != q.world) continue;
    double rel[3];
    mrs_obst::contact_fold(c, mrs_obst::eval(o, q.p, rel), j, q.thr);
  }
  return c;
}

static GridView view_of(const mrs_obst::Built& b, const std::vector<mrs_obstacle_t>& ob) {
  return {b.g, b.start.data(), b.items.data(), ob.data(), (int32_t)ob.size(), (int32_t)b.items.size()};
}

static void test_functions() {
  const double arm = 0.27, prop = 0.11, margin = 0.1;
  volatile double s1 = arm + prop;
  volatile double s2 = s1 + margin;
  CHECK(same_bits(mrs_obst::contact_radius(arm, prop), s1), "the radius is arm_length + prop_radius");
  CHECK(same_bits(mrs_obst::contact_threshold(mrs_obst::contact_radius(arm, prop), margin), s2), "the threshold is rad + margin");
  volatile double t1 = prop + margin;
  volatile double t2 = arm + t1;
  CHECK(!same_bits(s2, t2), "these values tell the two orders of the additions apart");
  Contact c = mrs_obst::contact_none();
  CHECK(c.count == 0 && mrs_obst::contact_index(c) == -1 && std::isinf(mrs_obst::contact_sd(c)) && mrs_obst::contact_sd(c) > 0, "the empty fold");
  mrs_obst::contact_fold(c, 0.65, 3, 0.65);  // sd == thr: outside
  mrs_obst::contact_fold(c, NAN, 4, 0.65);
  mrs_obst::contact_fold(c, 0.1, 5, NAN);
  mrs_obst::contact_fold(c, INFINITY, 6, INFINITY);
  CHECK(c.count == 0 && mrs_obst::contact_index(c) == -1, "sd == thr and NaN miss");
  mrs_obst::contact_fold(c, std::nextafter(0.65, 0.0), 3, 0.65);  // one ulp inside
  CHECK(c.count == 1 && c.j == 3 && same_bits(c.sd, std::nextafter(0.65, 0.0)), "one ulp inside touches");
  mrs_obst::contact_fold(c, 0.5, 9, 0.65);
  mrs_obst::contact_fold(c, 0.5, 7, 0.65);  // a tie: the lower index, though visited later
  mrs_obst::contact_fold(c, 0.5, 8, 0.65);
  CHECK(c.count == 4 && c.j == 7 && c.sd == 0.5, "a tie goes to the lower index");
  Contact z = mrs_obst::contact_none(), y = mrs_obst::contact_none();
  mrs_obst::contact_fold(z, 0.0, 2, 0.4), mrs_obst::contact_fold(z, -0.0, 5, 0.4);
  mrs_obst::contact_fold(y, -0.0, 5, 0.4), mrs_obst::contact_fold(y, 0.0, 2, 0.4);
  CHECK(z.j == 2 && y.j == 2 && same_bits(z.sd, 0.0) && same_bits(y.sd, 0.0) && z.count == 2, "-0.0 == +0.0 goes to the lower index, with its own zero");
  mrs_obst::contact_fold(z, -1.5, 11, 0.4);
  CHECK(z.j == 11 && z.sd == -1.5 && mrs_obst::contact_index(z) == 11 && mrs_obst::contact_sd(z) == -1.5, "inside a solid orders first");
  if (!failures) std::printf("ok functions\n");
}

static std::vector<mrs_obstacle_t> random_set(std::mt19937_64& rng, int m) {
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::vector<mrs_obstacle_t>            ob((size_t)m);
  for (int j = 0; j < m; j++) {
    mrs_obstacle_t& o = ob[(size_t)j];
    std::memset(&o, 0, sizeof o);
    o.kind  = j % 3;
    o.world = (j / 3) % 3 == 1 ? 5 : 0;
    o.flags = (j / 3) % 3 == 2 ? (uint32_t)MRS_OBST_ALL_WORLDS : 0u;
    for (int a = 0; a < 3; a++) o.c[a] = (a == 2 ? 10.0 : 40.0) * (2.0 * u(rng) - 1.0);
    for (int a = 0; a < 3; a++) o.h[a] = 0.2 + 2.0 * u(rng);
    if (o.kind == MRS_OBST_CYLINDER && j % 2 == 0) o.h[2] = INFINITY;               // a pillar without ends
    if (o.kind == MRS_OBST_BOX && j % 17 == 1) o.h[0] = 300.0, o.h[1] = 0.05 + u(rng);  // a huge box: a wall across the scene
    if (j % 29 == 3) o.c[0] = 5000.0 + 100.0 * u(rng), o.flags = (uint32_t)MRS_OBST_ALL_WORLDS;  // far away
    if (j % 31 == 4) o.h[0] = 0.0;                                                  // a degenerate solid
    CHECK(mrs_obst::invalid(o) == nullptr, "the random set holds an invalid obstacle");
  }
  return ob;
}

static std::vector<Point> random_points(std::mt19937_64& rng, const std::vector<mrs_obstacle_t>& ob, int n, double R) {
  std::uniform_real_distribution<double> u(0.0, 1.0);
  std::vector<Point>                     pts((size_t)n);
  for (int i = 0; i < n; i++) {
    Point& q = pts[(size_t)i];
    std::memset(&q, 0, sizeof q);
    const mrs_obstacle_t& o = ob[(size_t)(rng() % ob.size())];
    for (int a = 0; a < 3; a++) {  // around an obstacle, out to a few R from its surface
      const double h = std::isfinite(o.h[a]) ? o.h[a] : 30.0;
      q.p[a] = o.c[a] + (h + 2.0 * R) * (2.0 * u(rng) - 1.0);
    }
    if (i % 13 == 0) q.p[i % 3] = (i % 2 ? 1.0 : -1.0) * 1e7;  // far outside the grid
    if (i % 41 == 0) q.p[i % 3] = i % 2 ? NAN : INFINITY;
    if (i % 7 == 0 && o.kind == MRS_OBST_SPHERE) q.p[0] = o.c[0] + o.h[0], q.p[1] = o.c[1], q.p[2] = o.c[2];  // on a surface
    q.world = i % 3 == 0 ? 5u : (i % 3 == 1 ? 0u : 9u);
    q.thr   = i % 5 == 0 ? R : R * (0.3 + 0.7 * u(rng));  // per-point thresholds <= R
    if (i % 97 == 0) q.thr = NAN;
  }
  return pts;
}

static void test_random() {
  std::mt19937_64 rng(20240607);
  long long       touching = 0, several = 0, inside = 0, none = 0;
  for (int round = 0; round < 12; round++) {
    const int                         m  = round == 0 ? 1 : 20 + 37 * round;
    const double                      R  = round % 3 == 0 ? 0.4 : (round % 3 == 1 ? 0.76 : 1.515);
    const std::vector<mrs_obstacle_t> ob = random_set(rng, m);
    const std::vector<Point>          pts = random_points(rng, ob, 600, R);
    const mrs_obst::Built             b  = mrs_obst::build(ob.data(), m, R);
    const GridView                    v  = view_of(b, ob);
    for (const Point& q : pts) {
      const Contact want = brute(ob, q), got = mrs_obst::contact_search(v, q.p, q.world, q.thr);
      CHECK(same(got, want), "round %d at (%g, %g, %g) thr %g world %u: count %d / %d, index %d / %d, sd %.17g / %.17g", round, q.p[0], q.p[1], q.p[2],
            q.thr, q.world, got.count, want.count, got.j, want.j, got.sd, want.sd);
      touching += want.count > 0, several += want.count > 1, inside += want.count > 0 && want.sd < 0.0, none += want.count == 0;
    }
  }
  CHECK(touching > 500 && several > 100 && inside > 100 && none > 500, "%lld touching, %lld several, %lld inside, %lld none", touching, several, inside, none);
  {  // the empty set, with a caller's view that holds no arrays worth reading
    const mrs_obst::Built e = mrs_obst::build(nullptr, 0, 0.4);
    const GridView        ev{e.g, e.start.data(), e.items.data(), nullptr, 0, (int32_t)e.items.size()};
    const double          p[3] = {1.0, 2.0, 3.0};
    CHECK(mrs_obst::contact_search(ev, p, 0u, 0.4).count == 0, "an empty set touches nobody");
  }
  if (!failures) std::printf("ok random %lld touching %lld several %lld inside\n", touching, several, inside);
}

static void test_coarsened() {
  std::mt19937_64                   rng(77);
  const int                         m  = 240;
  const double                      R  = 0.65;
  const std::vector<mrs_obstacle_t> ob = random_set(rng, m);
  const std::vector<Point>          pts = random_points(rng, ob, 500, R);
  std::vector<Contact>              want;
  for (const Point& q : pts) want.push_back(brute(ob, q));
  int grids = 0, one_cell = 0;
  // lowered sizing limits (the grid coarsens), and larger R for the same thresholds: the result must not move
  const struct {
    double  R;
    int64_t cap_items, max_cells;
  } shapes[] = {{R, -1, mrs_obst::MAX_CELLS}, {R, 4000, 4096}, {R, 1000, 64}, {R, m, 1}, {2.0 * R, -1, mrs_obst::MAX_CELLS},
                {37.5, -1, mrs_obst::MAX_CELLS}, {1e4, -1, mrs_obst::MAX_CELLS}};
  for (const auto& s : shapes) {
    const mrs_obst::Built b = mrs_obst::build(ob.data(), m, s.R, s.cap_items, s.max_cells);
    const GridView        v = view_of(b, ob);
    grids++;
    one_cell += b.cells() == 1;
    for (size_t i = 0; i < pts.size(); i++) {
      const Contact got = mrs_obst::contact_search(v, pts[i].p, pts[i].world, pts[i].thr);
      CHECK(same(got, want[i]), "grid of R %g, %lld cells: point %zu count %d / %d index %d / %d", s.R, (long long)b.cells(), i, got.count, want[i].count,
            got.j, want[i].j);
    }
  }
  CHECK(grids == 7 && one_cell >= 1, "%d grids, %d of one cell", grids, one_cell);
  if (!failures) std::printf("ok coarsened %d grids\n", grids);
}

template <class T>
static bool read_all(const char* path, std::vector<T>* out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  out->resize((size_t)bytes / sizeof(T));
  const bool ok = bytes % (long)sizeof(T) == 0 && std::fread(out->data(), sizeof(T), out->size(), f) == out->size();
  std::fclose(f);
  return ok;
}

static void test_listed(const char* set_path, const char* pts_path, const char* out_path) {
  std::vector<mrs_obstacle_t> ob;
  std::vector<Point>          pts;
  CHECK(read_all(set_path, &ob) && read_all(pts_path, &pts) && !ob.empty() && !pts.empty(), "cannot read %s / %s", set_path, pts_path);
  if (failures) return;
  double R = 0.0;
  for (const Point& q : pts)
    if (std::isfinite(q.thr) && q.thr > R) R = q.thr;
  const mrs_obst::Built b = mrs_obst::build(ob.data(), (int32_t)ob.size(), R);
  const GridView        v = view_of(b, ob);
  std::vector<Result>   res;
  for (const Point& q : pts) {
    const Contact c = mrs_obst::contact_search(v, q.p, q.world, q.thr);
    CHECK(same(c, brute(ob, q)), "listed point (%g, %g, %g)", q.p[0], q.p[1], q.p[2]);
    res.push_back({mrs_obst::contact_sd(c), mrs_obst::contact_index(c), c.count});
  }
  FILE* f = std::fopen(out_path, "wb");
  CHECK(f && std::fwrite(res.data(), sizeof(Result), res.size(), f) == res.size(), "cannot write %s", out_path);
  if (f) std::fclose(f);
  if (!failures) std::printf("ok listed %zu points %zu obstacles R %g\n", pts.size(), ob.size(), R);
}

int main(int argc, char** argv) {
  static_assert(sizeof(Point) == 40 && sizeof(Result) == 16, "the records tests/test_obstacle_contacts.py writes and reads");
  test_functions();
  test_random();
  test_coarsened();
  if (argc == 4) test_listed(argv[1], argv[2], argv[3]);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("ok all\n");
  return 0;
}
