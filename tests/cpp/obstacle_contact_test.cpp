// obstacle_contact_test.cpp — UavSwarm::obstacleContactsDevice with plain hipMalloc'd outputs: the 2 000 UAVs and the 60 obstacles of
// obstacles_test.cpp, margin 1 m around the default airframe (arm_length + prop_radius): first the read-only form with all four
// outputs and a cost vector that holds NaN payloads, then the marking form with the hit bytes alone, read back through crashedDevice.
// Checked here against a search over all obstacles with the contract's own functions (csrc/obstacle_contact.h, compiled for the host),
// and written to argv[1] (hit, index, sd, count, cost, crashed) for tests/test_obstacle_contacts_gpu.py to compare with
// mrs_multirotor_simulator_amd.tensors.  Exit code 0 and "ok ..." lines on success.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <mrs_multirotor_simulator/uav_system/uav_system.hpp>

#include "../../mrs_multirotor_simulator_amd/csrc/obstacle_contact.h"

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
  const int    n = 2000, m = 60;
  const double margin = 1.0, hit_cost = 1000.0;
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

  uint8_t *d_hit = nullptr, *d_hit2 = nullptr, *d_crashed = nullptr;
  int32_t *d_index = nullptr, *d_count = nullptr;
  double * d_sd = nullptr, *d_cost = nullptr;
  HIP(hipMalloc((void**)&d_hit, (size_t)n));
  HIP(hipMalloc((void**)&d_hit2, (size_t)n));
  HIP(hipMalloc((void**)&d_crashed, (size_t)n));
  HIP(hipMalloc((void**)&d_index, sizeof(int32_t) * (size_t)n));
  HIP(hipMalloc((void**)&d_count, sizeof(int32_t) * (size_t)n));
  HIP(hipMalloc((void**)&d_sd, sizeof(double) * (size_t)n));
  HIP(hipMalloc((void**)&d_cost, sizeof(double) * (size_t)n));
  std::vector<double> cost0((size_t)n);
  for (int i = 0; i < n; i++) {  // every third element a NaN with a payload, the others numbers
    const uint64_t payload = 0x7FF8000000000000ull | (uint64_t)(i + 1);
    cost0[(size_t)i] = 0.5 * i;
    if (i % 3 == 0) std::memcpy(&cost0[(size_t)i], &payload, sizeof payload);
  }
  HIP(hipMemcpy(d_cost, cost0.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));

  bool refused = false;
  try {
    sw.obstacleContactsDevice(0, n, margin, 2u, d_hit);  // an unknown flag bit
  } catch (const std::exception&) {
    refused = true;
  }
  CHECK(refused);
  sw.obstacleContactsDevice(0, n, margin, 0u, d_hit, d_index, d_sd, d_count, d_cost, hit_cost);
  sw.crashedDevice(0, n, d_crashed);
  std::vector<uint8_t> hit((size_t)n), hit2((size_t)n), crashed((size_t)n);
  std::vector<int32_t> index((size_t)n), count((size_t)n);
  std::vector<double>  sd((size_t)n), cost((size_t)n);
  HIP(hipMemcpy(crashed.data(), d_crashed, (size_t)n, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) CHECK(crashed[(size_t)i] == 0);  // the read-only form marks nobody
  sw.obstacleContactsDevice(0, n, margin, MRS_CONTACT_CRASH, d_hit2);
  sw.crashedDevice(0, n, d_crashed);
  const mrs_obstacle_stats_t st = sw.obstacleStats();
  CHECK(st.count == m && st.grid_builds == 1 && st.cells == 0);  // the contacts' grid was built, once; the queries' grid was not
  HIP(hipMemcpy(hit.data(), d_hit, (size_t)n, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hit2.data(), d_hit2, (size_t)n, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(crashed.data(), d_crashed, (size_t)n, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(index.data(), d_index, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(count.data(), d_count, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(sd.data(), d_sd, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(cost.data(), d_cost, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));

  const double thr = mrs_obst::contact_threshold(mrs_obst::contact_radius(mp.arm_length, mp.prop_radius), margin);
  int          touching = 0, several = 0, inside = 0;
  for (int i = 0; i < n; i++) {
    const double      p[3] = {pos[(size_t)i](0), pos[(size_t)i](1), pos[(size_t)i](2)};
    mrs_obst::Contact c    = mrs_obst::contact_none();
    for (int j = m - 1; j >= 0; j--) {  // (descending: the fold does not depend on the order of the visits)
      double rel[3];
      mrs_obst::contact_fold(c, mrs_obst::eval(set[(size_t)j], p, rel), j, thr);
    }
    const bool h = c.count > 0;
    CHECK(hit[(size_t)i] == (h ? 1 : 0) && hit2[(size_t)i] == hit[(size_t)i] && crashed[(size_t)i] == hit[(size_t)i]);
    CHECK(count[(size_t)i] == c.count && index[(size_t)i] == mrs_obst::contact_index(c) && same_bits(sd[(size_t)i], mrs_obst::contact_sd(c)));
    const volatile double added = cost0[(size_t)i] + hit_cost;
    CHECK(same_bits(cost[(size_t)i], h ? (double)added : cost0[(size_t)i]));
    touching += h;
    several += c.count > 1;
    inside += h && c.sd < 0.0;
  }
  CHECK(touching > 50 && touching < n - 50 && several > 0 && inside > 0);
  std::printf("ok contacts_equal_brute_force %d %d %d %d\n", n, touching, several, inside);

  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f);
    CHECK(std::fwrite(hit.data(), 1, hit.size(), f) == hit.size());
    CHECK(std::fwrite(index.data(), sizeof(int32_t), index.size(), f) == index.size());
    CHECK(std::fwrite(sd.data(), sizeof(double), sd.size(), f) == sd.size());
    CHECK(std::fwrite(count.data(), sizeof(int32_t), count.size(), f) == count.size());
    CHECK(std::fwrite(cost.data(), sizeof(double), cost.size(), f) == cost.size());
    CHECK(std::fwrite(crashed.data(), 1, crashed.size(), f) == crashed.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  for (void* q : {(void*)d_hit, (void*)d_hit2, (void*)d_crashed, (void*)d_index, (void*)d_count, (void*)d_sd, (void*)d_cost}) HIP(hipFree(q));
  return 0;
}
