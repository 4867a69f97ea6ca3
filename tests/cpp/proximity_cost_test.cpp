// proximity_cost_test.cpp — UavSwarm::proximityCostDevice with plain hipMalloc'd outputs: the 2 000 UAVs of nearest_test.cpp on their
// jittered lattice, k = 8 within 5 m, the three kinds each into a vector of its own, and a fourth vector that holds HINGE2 with COUNT
// accumulated onto it.  Checked here against a brute-force search and the contract's sum (bit for bit, `found` uncapped), and written to
// argv[1] (the four cost vectors, then found) for tests/test_proximity_cost_gpu.py to compare with
// mrs_multirotor_simulator_amd.tensors.proximity_cost.  Exit code 0 and "ok ..." lines on success.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>
#include <mrs_multirotor_simulator/uav_system/uav_system.hpp>

using namespace mrs_multirotor_simulator;

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                  \
    }                                                            \
  } while (0)
#define HIP(c) CHECK((c) == hipSuccess)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main(int argc, char** argv) {
  const int    n = 2000, k = 8;
  const double radius = 5.0, weight = 0.75, eps = 0.125;
  MultirotorModel::ModelParams mp;
  std::vector<Eigen::Vector3d> pos;
  for (int i = 0; i < n; i++)  // (the same expressions as nearest_test.cpp)
    pos.push_back(Eigen::Vector3d(3.1 * (i % 20) + 0.01 * (i % 7), 2.9 * ((i / 20) % 20) - 0.02 * (i % 5), 3.3 * (i / 400) + 0.005 * (i % 11)));
  UavSwarm sw(n);
  sw.construct(0, n, mp, pos, std::vector<double>((size_t)n, 0.0));

  double*  d_cost  = nullptr;  // four vectors of n
  int32_t* d_found = nullptr;
  HIP(hipMalloc((void**)&d_cost, sizeof(double) * (size_t)n * 4));
  HIP(hipMalloc((void**)&d_found, sizeof(int32_t) * (size_t)n));
  HIP(hipMemset(d_cost, 0xFF, sizeof(double) * (size_t)n * 4));  // (NaN bits: accumulate == 0 must not read them)
  sw.proximityCostDevice(0, n, k, radius, MRS_PROX_HINGE2, weight, eps, d_cost, false, d_found);
  sw.proximityCostDevice(0, n, k, radius, MRS_PROX_INVERSE, weight, eps, d_cost + n, false);
  sw.proximityCostDevice(0, n, k, radius, MRS_PROX_COUNT, weight, eps, d_cost + 2 * n, false);
  sw.proximityCostDevice(0, n, k, radius, MRS_PROX_HINGE2, weight, eps, d_cost + 3 * n, false);
  sw.proximityCostDevice(0, n, k, radius, MRS_PROX_COUNT, weight, eps, d_cost + 3 * n, true);
  std::vector<double>  cost((size_t)n * 4);
  std::vector<int32_t> found((size_t)n);
  HIP(hipMemcpy(cost.data(), d_cost, sizeof(double) * cost.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(found.data(), d_found, sizeof(int32_t) * found.size(), hipMemcpyDeviceToHost));

  const double rr = radius * radius;
  int          listed = 0, over = 0;
  for (int i = 0; i < n; i++) {
    std::vector<std::pair<double, int>> nb;
    for (int j = 0; j < n; j++) {
      if (j == i) continue;
      const double dx = pos[j](0) - pos[i](0), dy = pos[j](1) - pos[i](1), dz = pos[j](2) - pos[i](2);
      const volatile double xx = dx * dx, yy = dy * dy, zz = dz * dz;  // (no contraction, whatever the host compiler's default)
      const volatile double s  = xx + yy;
      const double          d2 = s + zz;
      if (d2 < rr) nb.push_back({d2, j});
    }
    std::sort(nb.begin(), nb.end());
    const int nf = (int)std::min<size_t>(nb.size(), (size_t)k);
    CHECK(found[i] == (int)nb.size());
    listed += nf;
    over += (int)nb.size() > k;
    volatile double hinge = 0.0, inverse = 0.0, cnt = 0.0;
    for (int m = 0; m < nf; m++) {
      const double          d2 = nb[(size_t)m].first;
      const volatile double g  = radius - std::sqrt(d2);
      const volatile double wg = weight * g;
      const volatile double t  = wg * g;
      hinge                    = hinge + t;
      const volatile double de = d2 + eps;
      const volatile double q  = weight / de;
      inverse                  = inverse + q;
      cnt                      = cnt + weight;
    }
    const volatile double both = hinge + cnt;
    CHECK(same_bits(cost[(size_t)i], hinge));
    CHECK(same_bits(cost[(size_t)n + i], inverse));
    CHECK(same_bits(cost[(size_t)2 * n + i], cnt));
    CHECK(same_bits(cost[(size_t)3 * n + i], both));
  }
  CHECK(listed > n);
  CHECK(over > 0);  // (some UAVs have more than k neighbours: found is not capped)
  std::printf("ok proximity_equals_brute_force %d %d %d\n", n, listed, over);

  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f);
    CHECK(std::fwrite(cost.data(), sizeof(double), cost.size(), f) == cost.size());
    CHECK(std::fwrite(found.data(), sizeof(int32_t), found.size(), f) == found.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  HIP(hipFree(d_cost));
  HIP(hipFree(d_found));
  return 0;
}
