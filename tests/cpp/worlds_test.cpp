// worlds_test.cpp — collision worlds through the C++ facade (UavSwarm::setWorlds / getWorlds / setWorldsDevice).
// Without an argument (no GPU needed): the facade methods compile against the header, and the refusals that never reach the device —
// a null swarm is MRS_ERR_ARG for all three calls — are what the header says.  Like nearest_test it links the library itself, not
// tests/cpp/hip_stub: that stand-in covers the owning types of hip_owned.h and cannot carry host_api.hip, whose calls create a swarm
// (streams, kernels) before they look at a pointer or a range.  So null pointers, bad ranges, short rows and count == 0 on a live swarm
// are checked where a swarm exists: below with a path, and in test_collision_worlds_gpu.test_round_trip_and_bad_arguments.
// With a path (tests/test_collision_worlds_gpu.py): 150 UAVs, three interleaved worlds of which two share their coordinates; labels set
// from host memory, part of them again from device memory, read back; one elastic collision pass; labels and forces are written to the
// path for the test to compare with the Python calls.  Exit code 0 and "ok ..." lines on success.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
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
  {
    int32_t w[4] = {1, 2, 3, 4};
    CHECK(mrs_swarm_set_worlds(nullptr, 0, 4, w) == MRS_ERR_ARG);
    CHECK(mrs_swarm_get_worlds(nullptr, 0, 4, w) == MRS_ERR_ARG);
    CHECK(mrs_swarm_set_worlds_device(nullptr, 0, 4, w, nullptr) == MRS_ERR_ARG);
    CHECK(w[0] == 1 && w[3] == 4);
    void (UavSwarm::*a)(int, const std::vector<int32_t>&)       = &UavSwarm::setWorlds;
    std::vector<int32_t> (UavSwarm::*b)(int, int)               = &UavSwarm::getWorlds;
    void (UavSwarm::*c)(int, int, const int32_t*, void*)        = &UavSwarm::setWorldsDevice;
    CHECK(a && b && c);
    std::printf("ok refusals_without_a_device\n");
  }
  if (argc < 2) return 0;

  const int n = 150;
  MultirotorModel::ModelParams mp;
  std::vector<Eigen::Vector3d> pos;
  std::vector<int32_t>         world;
  const int32_t                labels[3] = {7, -2000000000, 1234567890};
  for (int i = 0; i < n; i++) {  // (the same expressions as test_collision_worlds_gpu.facade_scene: worlds 0 and 1 coincide)
    const int w = i % 3, k = i / 3, s = w == 2 ? 1 : 0;
    pos.push_back(Eigen::Vector3d(0.85 * (k % 5) + 0.0013 * k + 0.31 * s, 1.6 * ((k / 5) % 5) - 0.0007 * k, 10.0 + 2.0 * (k / 25) + 0.11 * s));
    world.push_back(labels[w]);
  }
  UavSwarm sw(n);
  sw.construct(0, n, mp, pos, std::vector<double>((size_t)n, 0.0));
  CHECK(sw.getWorlds(0, n) == std::vector<int32_t>((size_t)n, 0));
  sw.setWorlds(0, world);
  CHECK(sw.getWorlds(0, n) == world);
  // UAVs [60, 100) once more, from device memory, reversed and then restored
  int32_t* d = nullptr;
  HIP(hipMalloc((void**)&d, sizeof(int32_t) * 40));
  std::vector<int32_t> part(world.begin() + 60, world.begin() + 100), rev(part.rbegin(), part.rend());
  HIP(hipMemcpy(d, rev.data(), sizeof(int32_t) * 40, hipMemcpyHostToDevice));
  sw.setWorldsDevice(60, 40, d);
  CHECK(sw.getWorlds(60, 40) == rev && sw.getWorlds(0, 60) == std::vector<int32_t>(world.begin(), world.begin() + 60));
  HIP(hipMemcpy(d, part.data(), sizeof(int32_t) * 40, hipMemcpyHostToDevice));
  sw.setWorldsDevice(60, 40, d);
  CHECK(sw.getWorlds(0, n) == world);
  CHECK(mrs_swarm_set_worlds(sw.handle(), 140, 11, world.data()) == MRS_ERR_RANGE);
  CHECK(mrs_swarm_set_worlds_device(sw.handle(), 0, 4, world.data(), nullptr) == MRS_ERR_ARG);  // host memory
  CHECK(mrs_swarm_set_worlds(sw.handle(), 0, 4, nullptr) == MRS_ERR_ARG && mrs_swarm_get_worlds(sw.handle(), 0, 4, nullptr) == MRS_ERR_ARG);
  CHECK(mrs_swarm_set_worlds_device(sw.handle(), 0, 4, nullptr, nullptr) == MRS_ERR_ARG);
  CHECK(mrs_swarm_get_worlds(sw.handle(), -1, 4, part.data()) == MRS_ERR_RANGE && mrs_swarm_set_worlds_device(sw.handle(), 140, 11, d, nullptr) == MRS_ERR_RANGE);
  CHECK(mrs_swarm_set_worlds(sw.handle(), n, 0, nullptr) == MRS_OK && mrs_swarm_get_worlds(sw.handle(), n, 0, nullptr) == MRS_OK);  // count == 0
  CHECK(mrs_swarm_set_worlds_device(sw.handle(), 0, 0, nullptr, nullptr) == MRS_OK);
  CHECK(sw.getWorlds(0, n) == world);
  std::printf("ok labels_round_trip\n");

  sw.handleCollisions(true, false, 100.0);
  std::vector<double> force((size_t)n * 3);
  mrs_throw_on_error(mrs_swarm_get_external_force(sw.handle(), 0, n, force.data()));
  int pushed = 0;
  for (int i = 0; i < n; i++) {
    for (int c = 0; c < 3; c++) CHECK(std::isfinite(force[(size_t)i * 3 + c]));
    pushed += force[(size_t)i * 3] != 0.0 || force[(size_t)i * 3 + 1] != 0.0 || force[(size_t)i * 3 + 2] != 0.0;
  }
  CHECK(pushed > 30);
  std::printf("ok forces_finite %d\n", pushed);

  FILE* f = std::fopen(argv[1], "wb");
  CHECK(f);
  const std::vector<int32_t> got = sw.getWorlds(0, n);
  CHECK(std::fwrite(got.data(), sizeof(int32_t), got.size(), f) == got.size());
  CHECK(std::fwrite(force.data(), sizeof(double), force.size(), f) == force.size());
  std::fclose(f);
  std::printf("ok written\n");
  HIP(hipFree(d));
  return 0;
}
