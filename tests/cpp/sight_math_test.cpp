// sight_math_test.cpp — the pure functions of the line-of-sight neighbours (mrs_multirotor_simulator_amd/csrc/sight_math.h: direction,
// hides, before) without a GPU: reads a binary file of cases and prints, per case, the bits of d and u that direction forms from
// dx = q - p, the answers of mrs_scan::gate and of hides for the obstacle, and the answer of before for the case's two keys, which
// tests/test_nearest_visible.py compares with its numpy restatement bit for bit.  These are the functions the kernel of
// nearest_visible.hip calls.  Built by that test with the host compiler, -ffp-contract=off and -fsanitize=address,undefined, and run
// directly.
// A case is 152 B: the obstacle record (64 B), p[3], q[3], radius, d2a, d2b, ja, jb, one double of padding.  Usage: sight_math_test cases.bin
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mrs_multirotor_simulator_amd/csrc/sight_math.h"

struct Case {
  mrs_obstacle_t o;
  double         p[3], q[3], radius, d2a, d2b;
  int32_t        ja, jb;
  double         pad;
};
static_assert(sizeof(mrs_obstacle_t) == 64, "the obstacle record is 64 B");
static_assert(sizeof(Case) == 152, "a case is 152 B");

static unsigned long long bits(double v) {
  unsigned long long b;
  std::memcpy(&b, &v, sizeof b);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: %s cases.bin\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::printf("cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<Case> cases;
  Case              c;
  while (std::fread(&c, sizeof c, 1, f) == 1) cases.push_back(c);
  std::fclose(f);
  for (const Case& k : cases) {
    // the candidate's offset and d2 as the kernel forms them (this unit is compiled without contraction)
    const volatile double dx0 = k.q[0] - k.p[0], dx1 = k.q[1] - k.p[1], dx2 = k.q[2] - k.p[2];
    const double          dx[3] = {dx0, dx1, dx2};
    const volatile double xx = dx[0] * dx[0], yy = dx[1] * dx[1], zz = dx[2] * dx[2];
    const volatile double xy = xx + yy;
    const double          d2 = xy + zz;
    double                u[3];
    const double          d = mrs_sight::direction(dx, d2, u);
    std::printf("%016llx %016llx %016llx %016llx %016llx %d %d %d\n", bits(d2), bits(d), bits(u[0]), bits(u[1]), bits(u[2]),
                mrs_scan::gate(k.o, k.p, k.radius) ? 1 : 0, mrs_sight::hides(k.o, k.p, u, d, k.radius) ? 1 : 0,
                mrs_sight::before(k.d2a, k.ja, k.d2b, k.jb) ? 1 : 0);
  }
  std::printf("ok %zu cases\n", cases.size());
  return 0;
}
