// obstacles_test.cpp — UavSwarm::setObstacles / nearestObstaclesDevice / obstacleCostDevice with plain hipMalloc'd outputs: the 2 000 UAVs
// of nearest_test.cpp on their jittered lattice among 60 spheres, boxes and cylinders (every other cylinder a pillar without ends), k = 4
// within 5 m: all fields as FP64 rows with indices and counts, HINGE2 into a cost vector and COUNT accumulated onto it, `found` uncapped.
// Checked here against a search over all obstacles with the contract's own expressions (csrc/obstacle_grid.h eval, compiled for the host),
// and written to argv[1] (rows, index, count, cost, found) for tests/test_obstacles_gpu.py to compare with
// mrs_multirotor_simulator_amd.tensors.  Exit code 0 and "ok ..." lines on success.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>
#include <mrs_multirotor_simulator/uav_system/uav_system.hpp>

#include "../../mrs_multirotor_simulator_amd/csrc/obstacle_grid.h"

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
  const int    n = 2000, k = 4, m = 60, w = 7;
  const double radius = 5.0, weight = 0.75;
  MultirotorModel::ModelParams mp;
  std::vector<Eigen::Vector3d> pos;
  for (int i = 0; i < n; i++)  // (the same expressions as nearest_test.cpp)
    pos.push_back(Eigen::Vector3d(3.1 * (i % 20) + 0.01 * (i % 7), 2.9 * ((i / 20) % 20) - 0.02 * (i % 5), 3.3 * (i / 400) + 0.005 * (i % 11)));
  UavSwarm sw(n);
  sw.construct(0, n, mp, pos, std::vector<double>((size_t)n, 0.0));
  std::vector<mrs_obstacle_t> set((size_t)m);
  for (int j = 0; j < m; j++) {
    mrs_obstacle_t& o = set[(size_t)j];
    std::memset(&o, 0, sizeof o);
    o.kind = j % 3;
    o.c[0] = 6.2 * (j % 8) + 0.5, o.c[1] = 7.1 * ((j / 8) % 8) - 0.25, o.c[2] = 3.0 + 1.5 * (j % 4);
    o.h[0] = 1.4 + 0.3 * (j % 5), o.h[1] = 1.3 + 0.4 * (j % 3), o.h[2] = j % 6 == 2 ? INFINITY : 2.0 + 0.5 * (j % 4);
  }
  sw.setObstacles(set);
  const std::vector<mrs_obstacle_t> back = sw.getObstacles();
  CHECK(back.size() == set.size() && std::memcmp(back.data(), set.data(), sizeof(mrs_obstacle_t) * set.size()) == 0);
  int32_t width = 0;
  CHECK(mrs_obstacle_width(MRS_ON_ALL, k, &width) == MRS_OK && width == k * w);

  double * d_rows = nullptr, *d_cost = nullptr;
  int32_t *d_index = nullptr, *d_count = nullptr, *d_found = nullptr;
  HIP(hipMalloc((void**)&d_rows, sizeof(double) * (size_t)n * k * w));
  HIP(hipMalloc((void**)&d_cost, sizeof(double) * (size_t)n));
  HIP(hipMalloc((void**)&d_index, sizeof(int32_t) * (size_t)n * k));
  HIP(hipMalloc((void**)&d_count, sizeof(int32_t) * (size_t)n));
  HIP(hipMalloc((void**)&d_found, sizeof(int32_t) * (size_t)n));
  HIP(hipMemset(d_cost, 0xFF, sizeof(double) * (size_t)n));  // (NaN bits: accumulate == 0 must not read them)
  sw.nearestObstaclesDevice(0, n, k, radius, MRS_ON_ALL, d_rows, MRS_DTYPE_F64, k * w, d_index, k, d_count);
  sw.obstacleCostDevice(0, n, k, radius, MRS_PROX_HINGE2, weight, d_cost, false, d_found);
  sw.obstacleCostDevice(0, n, k, radius, MRS_PROX_COUNT, weight, d_cost, true);
  const mrs_obstacle_stats_t st = sw.obstacleStats();
  CHECK(st.count == m && st.grid_builds == 1 && st.grid_radius == radius && st.dims[0] > 1 && st.dims[1] > 1 && st.list_items >= m);
  std::vector<double>  rows((size_t)n * k * w), cost((size_t)n);
  std::vector<int32_t> index((size_t)n * k), count((size_t)n), found((size_t)n);
  HIP(hipMemcpy(rows.data(), d_rows, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(cost.data(), d_cost, sizeof(double) * cost.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(index.data(), d_index, sizeof(int32_t) * index.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(count.data(), d_count, sizeof(int32_t) * count.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(found.data(), d_found, sizeof(int32_t) * found.size(), hipMemcpyDeviceToHost));

  int listed = 0, over = 0, inside = 0;
  for (int i = 0; i < n; i++) {
    const double p[3] = {pos[(size_t)i](0), pos[(size_t)i](1), pos[(size_t)i](2)};
    std::vector<std::pair<double, int>> hit;
    for (int j = 0; j < m; j++) {
      double       rel[3];
      const double sd = mrs_obst::eval(set[(size_t)j], p, rel);
      if (sd < radius) hit.push_back({sd, j});
    }
    std::sort(hit.begin(), hit.end());
    const int nf = (int)std::min<size_t>(hit.size(), (size_t)k);
    CHECK(found[(size_t)i] == (int)hit.size() && count[(size_t)i] == nf);
    listed += nf;
    over += (int)hit.size() > k;
    volatile double hinge = 0.0, cnt = 0.0;
    for (int s = 0; s < k; s++) {
      const double* row = &rows[((size_t)i * k + s) * w];
      if (s >= nf) {
        CHECK(index[(size_t)i * k + s] == -1);
        for (int e = 0; e < w; e++) CHECK(same_bits(row[e], 0.0));
        continue;
      }
      const int j = hit[(size_t)s].second;
      CHECK(index[(size_t)i * k + s] == j);
      double       rel[3];
      const double sd = mrs_obst::eval(set[(size_t)j], p, rel);
      inside += sd < 0.0;
      for (int e = 0; e < 3; e++) {
        CHECK(same_bits(row[e], rel[e]));
        CHECK(same_bits(row[3 + e], rel[e]) || (row[3 + e] == 0.0 && rel[e] == 0.0));  // heading 0: R = I, up to the sign of a zero sum
      }
      CHECK(same_bits(row[6], sd));
      const volatile double g  = radius - sd;
      const volatile double wg = weight * g;
      const volatile double t  = wg * g;
      hinge                    = hinge + t;
      cnt                      = cnt + weight;
    }
    const volatile double h0   = 0.0 + hinge;
    const volatile double both = h0 + cnt;
    CHECK(same_bits(cost[(size_t)i], both));
  }
  CHECK(listed > n && over > 0 && inside > 0);
  std::printf("ok obstacles_equal_brute_force %d %d %d %d\n", n, listed, over, inside);

  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f);
    CHECK(std::fwrite(rows.data(), sizeof(double), rows.size(), f) == rows.size());
    CHECK(std::fwrite(index.data(), sizeof(int32_t), index.size(), f) == index.size());
    CHECK(std::fwrite(count.data(), sizeof(int32_t), count.size(), f) == count.size());
    CHECK(std::fwrite(cost.data(), sizeof(double), cost.size(), f) == cost.size());
    CHECK(std::fwrite(found.data(), sizeof(int32_t), found.size(), f) == found.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  for (void* q : {(void*)d_rows, (void*)d_cost, (void*)d_index, (void*)d_count, (void*)d_found}) HIP(hipFree(q));
  return 0;
}
