// nearest_visible_test.cpp — UavSwarm::nearestVisibleDevice with plain hipMalloc'd outputs: the 2 000 UAVs and the 60 obstacles of
// obstacles_test.cpp, radius 4 m, k = 8, MRS_NN_REL_POS | MRS_NN_DIST as FP64 rows with 3 elements of slack.  Checked here against a
// search over all UAVs and all obstacles with the contract's own functions (csrc/sight_math.h, compiled for the host), and written to
// argv[1] (rows, index, count, visible, hidden) for tests/test_nearest_visible_gpu.py to compare with
// mrs_multirotor_simulator_amd.tensors.  Exit code 0 and "ok ..." lines on success.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>
#include <mrs_multirotor_simulator/uav_system/uav_system.hpp>

#include "../../mrs_multirotor_simulator_amd/csrc/sight_math.h"

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
  const int    n = 2000, m = 60, k = 8, width = 4, stride = k * width + 3;
  const double radius = 4.0, mark = -123.456;
  MultirotorModel::ModelParams mp;
  std::vector<Eigen::Vector3d> pos;
  for (int i = 0; i < n; i++)  // (the same expressions as obstacles_test.cpp)
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

  double*  d_rows = nullptr;
  int32_t *d_index = nullptr, *d_count = nullptr, *d_visible = nullptr, *d_hidden = nullptr;
  HIP(hipMalloc((void**)&d_rows, sizeof(double) * (size_t)n * stride));
  HIP(hipMalloc((void**)&d_index, sizeof(int32_t) * (size_t)n * k));
  HIP(hipMalloc((void**)&d_count, sizeof(int32_t) * (size_t)n));
  HIP(hipMalloc((void**)&d_visible, sizeof(int32_t) * (size_t)n));
  HIP(hipMalloc((void**)&d_hidden, sizeof(int32_t) * (size_t)n));
  std::vector<double> rows((size_t)n * stride, mark);
  HIP(hipMemcpy(d_rows, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));

  bool refused = false;
  try {
    sw.nearestVisibleDevice(0, n, k, radius, 0u, nullptr, MRS_DTYPE_F64, 0);  // no output at all
  } catch (const std::exception&) {
    refused = true;
  }
  CHECK(refused);
  sw.nearestVisibleDevice(0, n, k, radius, MRS_NN_REL_POS | MRS_NN_DIST, d_rows, MRS_DTYPE_F64, stride, d_index, k, d_count, d_visible, d_hidden);
  const mrs_obstacle_stats_t st = sw.obstacleStats();
  CHECK(st.count == m && st.grid_builds == 1 && st.cells == 0);  // the sight lines' grid was built, once; the queries' grid was not
  std::vector<int32_t> index((size_t)n * k), count((size_t)n), visible((size_t)n), hidden((size_t)n);
  HIP(hipMemcpy(rows.data(), d_rows, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(index.data(), d_index, sizeof(int32_t) * index.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(count.data(), d_count, sizeof(int32_t) * count.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(visible.data(), d_visible, sizeof(int32_t) * visible.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hidden.data(), d_hidden, sizeof(int32_t) * hidden.size(), hipMemcpyDeviceToHost));

  const double rr = radius * radius;
  long         seen = 0, unseen = 0, blind = 0;
  for (int i = 0; i < n; i++) {
    const double                        p[3] = {pos[(size_t)i](0), pos[(size_t)i](1), pos[(size_t)i](2)};
    std::vector<std::pair<double, int>> vis;
    int                                 hid = 0;
    for (int j = 0; j < n; j++) {
      if (j == i) continue;
      const volatile double dx0 = pos[(size_t)j](0) - p[0], dx1 = pos[(size_t)j](1) - p[1], dx2 = pos[(size_t)j](2) - p[2];
      const double          dx[3] = {dx0, dx1, dx2};
      const volatile double xx = dx[0] * dx[0], yy = dx[1] * dx[1], zz = dx[2] * dx[2];
      const volatile double xy = xx + yy;
      const double          d2 = xy + zz;
      if (!(d2 < rr)) continue;
      bool h = false;
      if (d2 != 0.0) {
        double       u[3];
        const double d = mrs_sight::direction(dx, d2, u);
        for (int o = m - 1; o >= 0 && !h; o--) h = mrs_sight::hides(set[(size_t)o], p, u, d, radius);  // (the order of the obstacles does not matter)
      }
      if (h)
        hid++;
      else
        vis.push_back({d2, j});
    }
    std::sort(vis.begin(), vis.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) {
      return mrs_sight::before(a.first, a.second, b.first, b.second);
    });
    const int nf = std::min((int)vis.size(), k);
    CHECK(visible[(size_t)i] == (int)vis.size() && hidden[(size_t)i] == hid && count[(size_t)i] == nf);
    const double* r = &rows[(size_t)i * stride];
    for (int s = 0; s < k; s++) {
      CHECK(index[(size_t)i * k + s] == (s < nf ? vis[(size_t)s].second : -1));
      if (s < nf) {
        const int j = vis[(size_t)s].second;
        for (int c = 0; c < 3; c++) {
          const volatile double rel = pos[(size_t)j](c) - p[c];
          CHECK(same_bits(r[s * width + c], (double)rel));
        }
        CHECK(same_bits(r[s * width + 3], std::sqrt(vis[(size_t)s].first)));
      } else {
        for (int c = 0; c < width; c++) CHECK(same_bits(r[s * width + c], 0.0));
      }
    }
    for (int c = k * width; c < stride; c++) CHECK(same_bits(r[c], mark));  // the slack is untouched
    seen += (long)vis.size();
    unseen += hid;
    blind += vis.empty() && hid > 0;
  }
  CHECK(seen > 4000 && unseen > 700);  // (the numpy restatement counts 9 288 visible and 1 512 hidden pairs on this scene)
  std::printf("ok visible_equals_brute_force %d %ld %ld %ld\n", n, seen, unseen, blind);

  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f);
    CHECK(std::fwrite(rows.data(), sizeof(double), rows.size(), f) == rows.size());
    CHECK(std::fwrite(index.data(), sizeof(int32_t), index.size(), f) == index.size());
    CHECK(std::fwrite(count.data(), sizeof(int32_t), count.size(), f) == count.size());
    CHECK(std::fwrite(visible.data(), sizeof(int32_t), visible.size(), f) == visible.size());
    CHECK(std::fwrite(hidden.data(), sizeof(int32_t), hidden.size(), f) == hidden.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  for (void* q : {(void*)d_rows, (void*)d_index, (void*)d_count, (void*)d_visible, (void*)d_hidden}) HIP(hipFree(q));
  return 0;
}
