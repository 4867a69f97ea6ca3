// nearest_test.cpp — UavSwarm::nearestDevice with plain hipMalloc'd outputs: 2 000 UAVs on a jittered lattice, k = 8 nearest within 5 m,
// all fields in FP64.  Checked here against a brute-force search (indices, counts, relative positions and distances bit for bit), and
// written to argv[1] (index rows, then the field rows) for tests/test_nearest_gpu.py to compare with mrs_multirotor_simulator_amd.tensors.
// Exit code 0 and "ok ..." lines on success.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
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

int main(int argc, char** argv) {
  const int    n = 2000, k = 8;
  const double radius = 5.0;
  MultirotorModel::ModelParams mp;
  std::vector<Eigen::Vector3d> pos;
  for (int i = 0; i < n; i++)  // (the same expressions as test_nearest_gpu.lattice_positions)
    pos.push_back(Eigen::Vector3d(3.1 * (i % 20) + 0.01 * (i % 7), 2.9 * ((i / 20) % 20) - 0.02 * (i % 5), 3.3 * (i / 400) + 0.005 * (i % 11)));
  UavSwarm sw(n);
  sw.construct(0, n, mp, pos, std::vector<double>((size_t)n, 0.0));

  int32_t width = 0;
  mrs_throw_on_error(mrs_nearest_width(MRS_NN_ALL, k, &width));
  CHECK(width == 13 * k);
  double*  d_rows = nullptr;
  int32_t *d_idx = nullptr, *d_cnt = nullptr;
  HIP(hipMalloc((void**)&d_rows, sizeof(double) * (size_t)n * width));
  HIP(hipMalloc((void**)&d_idx, sizeof(int32_t) * (size_t)n * k));
  HIP(hipMalloc((void**)&d_cnt, sizeof(int32_t) * (size_t)n));
  sw.nearestDevice(0, n, k, radius, MRS_NN_ALL, d_rows, MRS_DTYPE_F64, width, d_idx, k, d_cnt);
  std::vector<double>  rows((size_t)n * width);
  std::vector<int32_t> idx((size_t)n * k), cnt((size_t)n);
  HIP(hipMemcpy(rows.data(), d_rows, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(idx.data(), d_idx, sizeof(int32_t) * idx.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(cnt.data(), d_cnt, sizeof(int32_t) * cnt.size(), hipMemcpyDeviceToHost));

  const double rr     = radius * radius;
  int          listed = 0;
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
    const int m = (int)std::min<size_t>(nb.size(), (size_t)k);
    CHECK(cnt[i] == m);
    listed += m;
    for (int s = 0; s < k; s++) {
      const double* o = &rows[(size_t)i * width + (size_t)s * 13];
      if (s >= m) {
        CHECK(idx[(size_t)i * k + s] == -1);
        for (int e = 0; e < 13; e++) CHECK(o[e] == 0.0);
        continue;
      }
      const int j = nb[(size_t)s].second;
      CHECK(idx[(size_t)i * k + s] == j);
      for (int c = 0; c < 3; c++) CHECK(o[c] == pos[j](c) - pos[i](c));
      CHECK(o[12] == std::sqrt(nb[(size_t)s].first));
    }
  }
  CHECK(listed > n);
  std::printf("ok nearest_equals_brute_force %d %d\n", n, listed);

  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f);
    CHECK(std::fwrite(idx.data(), sizeof(int32_t), idx.size(), f) == idx.size());
    CHECK(std::fwrite(rows.data(), sizeof(double), rows.size(), f) == rows.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  HIP(hipFree(d_rows));
  HIP(hipFree(d_idx));
  HIP(hipFree(d_cnt));
  return 0;
}
