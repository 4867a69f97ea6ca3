// range_scan_uavs_test.cpp — UavSwarm::rangeScanUavsDevice with plain hipMalloc'd outputs: the 2 000 UAVs, the 60 obstacles and the 10
// beams of range_scan_test.cpp, body frame (heading 0) with the ground plane, max_range 9 m, FP64 ranges, hit values and UAV indices.
// Checked here against a search over all obstacles and all UAVs with the contract's own functions (csrc/range_scan_math.h, compiled for
// the host), and written to argv[1] (ranges, hits, uavs) for tests/test_range_scan_uavs_gpu.py to compare with
// mrs_multirotor_simulator_amd.tensors.  Exit code 0 and "ok ..." lines on success.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <mrs_multirotor_simulator/uav_system/uav_system.hpp>

#include "../../mrs_multirotor_simulator_amd/csrc/range_scan_math.h"

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
  const int    n = 2000, m = 60, nb = 10;
  const double max_range = 9.0;
  MultirotorModel::ModelParams mp;
  const double                 rad = mp.arm_length + mp.prop_radius;
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
  const std::vector<double> beams = {1.0, 0.0, 0.0,  0.0, 1.0, 0.0,  -1.0, 0.0,  0.0,  0.0,  -1.0, 0.0,  0.0,  0.0,   -1.0,
                                     0.0, 0.0, 1.0,  0.6, 0.8, 0.0,  0.0,  -0.6, -0.8, -0.8, 0.0,  0.6,  0.28, -0.96, 0.0};
  sw.setScanBeams(beams);

  double * d_ranges = nullptr;
  int32_t *d_hit = nullptr, *d_uav = nullptr;
  HIP(hipMalloc((void**)&d_ranges, sizeof(double) * (size_t)n * nb));
  HIP(hipMalloc((void**)&d_hit, sizeof(int32_t) * (size_t)n * nb));
  HIP(hipMalloc((void**)&d_uav, sizeof(int32_t) * (size_t)n * nb));
  bool refused = false;
  try {
    sw.rangeScanUavsDevice(0, n, max_range, 4u, d_ranges, MRS_DTYPE_F64, nb, d_hit, nb, d_uav, nb);  // an unknown flag bit
  } catch (const std::exception&) {
    refused = true;
  }
  CHECK(refused);
  sw.rangeScanUavsDevice(0, n, max_range, MRS_SCAN_BODY_FRAME | MRS_SCAN_GROUND, d_ranges, MRS_DTYPE_F64, nb, d_hit, nb, d_uav, nb);
  std::vector<double>  ranges((size_t)n * nb);
  std::vector<int32_t> hit((size_t)n * nb), uav((size_t)n * nb);
  HIP(hipMemcpy(ranges.data(), d_ranges, sizeof(double) * ranges.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hit.data(), d_hit, sizeof(int32_t) * hit.size(), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(uav.data(), d_uav, sizeof(int32_t) * uav.size(), hipMemcpyDeviceToHost));

  int on_obstacle = 0, on_uav = 0, on_ground = 0, none = 0;
  for (int i = 0; i < n; i++) {
    const double p[3] = {pos[(size_t)i](0), pos[(size_t)i](1), pos[(size_t)i](2)};
    for (int b = 0; b < nb; b++) {
      const double* u    = &beams[(size_t)b * 3];  // heading 0: R = I, and 1.0 * x + 0.0 * y + 0.0 * z == x for these components
      double        best = max_range;
      int           idx = MRS_SCAN_HIT_NONE, who = -1;
      for (int j = 0; j < m; j++) {
        if (!mrs_scan::gate(set[(size_t)j], p, max_range)) continue;
        const double t = mrs_scan::ray(set[(size_t)j], p, u);
        if (t < best) best = t, idx = j;
      }
      double  bt = mrs_scan::miss();
      int32_t bj = 0x7FFFFFFF;
      for (int j = 0; j < n; j++) {
        if (j == i) continue;
        const double         q[3] = {pos[(size_t)j](0), pos[(size_t)j](1), pos[(size_t)j](2)};
        const mrs_obstacle_t o    = mrs_scan::uav_target(q, rad);
        if (!mrs_scan::gate(o, p, max_range)) continue;
        mrs_scan::take_uav(mrs_scan::ray(o, p, u), j, &bt, &bj);
      }
      if (bt < best) best = bt, idx = MRS_UAVSCAN_HIT_UAV, who = bj;
      const double tg = mrs_scan::ground(p[2], u[2], mp.ground_z);
      if (tg < best) best = tg, idx = MRS_SCAN_HIT_GROUND, who = -1;
      CHECK(hit[(size_t)i * nb + b] == idx);
      CHECK(uav[(size_t)i * nb + b] == who);
      CHECK(same_bits(ranges[(size_t)i * nb + b], best) || (best == 0.0 && ranges[(size_t)i * nb + b] == 0.0));
      on_obstacle += idx >= 0, on_uav += idx == MRS_UAVSCAN_HIT_UAV, on_ground += idx == MRS_SCAN_HIT_GROUND, none += idx == MRS_SCAN_HIT_NONE;
    }
  }
  CHECK(on_obstacle > n / 2 && on_uav > n / 2 && on_ground > n / 4 && none > n / 2);
  std::printf("ok range_scan_uavs_equals_brute_force %d %d %d %d %d\n", n, on_obstacle, on_uav, on_ground, none);

  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f);
    CHECK(std::fwrite(ranges.data(), sizeof(double), ranges.size(), f) == ranges.size());
    CHECK(std::fwrite(hit.data(), sizeof(int32_t), hit.size(), f) == hit.size());
    CHECK(std::fwrite(uav.data(), sizeof(int32_t), uav.size(), f) == uav.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  HIP(hipFree(d_ranges));
  HIP(hipFree(d_hit));
  HIP(hipFree(d_uav));
  return 0;
}
