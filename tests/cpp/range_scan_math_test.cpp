// range_scan_math_test.cpp — the pure functions of the range scans (mrs_multirotor_simulator_amd/csrc/range_scan_math.h) without a GPU:
// reads a binary file of cases and prints, per case, the bits of mrs_scan::ray, the answer of mrs_scan::gate and the bits of
// mrs_scan::ground, which tests/test_range_scan.py compares with its numpy restatement bit for bit.  These are the functions the kernel
// of range_scan.hip calls, so this checks the device function's text on the CPU.  Built by tests/test_range_scan.py with the host
// compiler, -ffp-contract=off and -fsanitize=address,undefined, and run directly.
// A case is 128 B: mrs_obstacle_t (64 B), p[3], u[3], max_range, ground_z.  Usage: range_scan_math_test cases.bin
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mrs_multirotor_simulator_amd/csrc/range_scan_math.h"

struct Case {
  mrs_obstacle_t o;
  double         p[3], u[3], max_range, ground_z;
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
  for (const Case& k : cases)
    std::printf("%016llx %d %016llx\n", bits(mrs_scan::ray(k.o, k.p, k.u)), mrs_scan::gate(k.o, k.p, k.max_range) ? 1 : 0,
                bits(mrs_scan::ground(k.p[2], k.u[2], k.ground_z)));
  std::printf("ok %zu cases\n", cases.size());
  return 0;
}
