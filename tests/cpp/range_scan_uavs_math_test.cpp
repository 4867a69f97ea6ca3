// range_scan_uavs_math_test.cpp — the pure functions of the range scans that see other UAVs
// (mrs_multirotor_simulator_amd/csrc/range_scan_math.h: uav_target, take_uav, and gate and ray on the record uav_target returns) without
// a GPU: reads a binary file of cases and prints, per case, whether uav_target returned the stated sphere record, the answer of gate and
// the bits of ray on it, and what take_uav left in (best_t, best_j), which tests/test_range_scan_uavs.py compares with its numpy
// restatement bit for bit.  These are the functions the kernel of range_scan_uavs.hip calls.  Built by that test with the host compiler,
// -ffp-contract=off and -fsanitize=address,undefined, and run directly.
// A case is 128 B: q[3], rad, p[3], u[3], max_range, t, best_t, j, best_j, two doubles of padding.  Usage: range_scan_uavs_math_test cases.bin
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mrs_multirotor_simulator_amd/csrc/range_scan_math.h"

struct Case {
  double  q[3], rad, p[3], u[3], max_range, t, best_t;
  int32_t j, best_j;
  double  pad[2];
};
static_assert(sizeof(Case) == 128, "a case is 128 B");

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
    const mrs_obstacle_t o = mrs_scan::uav_target(k.q, k.rad);
    const bool record = o.kind == MRS_OBST_SPHERE && o.flags == 0u && bits(o.c[0]) == bits(k.q[0]) && bits(o.c[1]) == bits(k.q[1]) &&
                        bits(o.c[2]) == bits(k.q[2]) && bits(o.h[0]) == bits(k.rad);
    double  best_t = k.best_t;
    int32_t best_j = k.best_j;
    mrs_scan::take_uav(k.t, k.j, &best_t, &best_j);
    std::printf("%d %d %016llx %016llx %d\n", record ? 1 : 0, mrs_scan::gate(o, k.p, k.max_range) ? 1 : 0, bits(mrs_scan::ray(o, k.p, k.u)), bits(best_t),
                (int)best_j);
  }
  std::printf("ok %zu cases\n", cases.size());
  return 0;
}
