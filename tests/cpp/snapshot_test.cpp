// snapshot_test.cpp — UavSwarm::saveDevice / loadDevice with plain hipMalloc'd records: 1 000 UAVs fly 150 position-command steps, are
// saved, fly 150 more, and are loaded back: a second save must equal the first byte for byte, and the positions must equal the pose
// array of the first moment.  One record forked into 10 UAVs through an index reports its status bytes.  The first save is written to
// argv[1] for tests/test_snapshot_gpu.py to compare with mrs_multirotor_simulator_amd.tensors.save of the same swarm.
// Exit code 0 and "ok ..." lines on success.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
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
  const int                    n = 1000;
  MultirotorModel::ModelParams mp;
  mp.ground_enabled = true;
  mp.ground_z       = 0.0;
  std::vector<Eigen::Vector3d> pos;
  std::vector<double>          hdg;
  std::vector<double>          cmd((size_t)n * 4);
  for (int i = 0; i < n; i++) {  // (the same expressions as test_snapshot_gpu.test_cpp_facade_equals_python)
    pos.push_back(Eigen::Vector3d(4.0 * (i % 32), 4.0 * (i / 32), 0.0));
    hdg.push_back(0.003 * i);
    cmd[(size_t)i * 4 + 0] = 4.0 * (i % 32) + 1.0;
    cmd[(size_t)i * 4 + 1] = 4.0 * (i / 32) - 0.5;
    cmd[(size_t)i * 4 + 2] = 2.0 + 0.002 * i;
    cmd[(size_t)i * 4 + 3] = 0.001 * i - 0.5;
  }
  UavSwarm sw(n);
  sw.construct(0, n, mp, pos, hdg);
  mrs_throw_on_error(mrs_swarm_set_input(sw.handle(), 0, n, MRS_POSITION_CMD, cmd.data(), 4));
  sw.makeSteps(0.001, 150);

  static_assert(sizeof(mrs_uav_snapshot_t) == 496, "snapshot record = 496 B");
  mrs_uav_snapshot_t *d_rec = nullptr, *d_rec2 = nullptr;
  int32_t*            d_idx    = nullptr;
  uint8_t*            d_status = nullptr;
  HIP(hipMalloc((void**)&d_rec, sizeof(mrs_uav_snapshot_t) * (size_t)n));
  HIP(hipMalloc((void**)&d_rec2, sizeof(mrs_uav_snapshot_t) * (size_t)n));
  HIP(hipMalloc((void**)&d_idx, sizeof(int32_t) * 10));
  HIP(hipMalloc((void**)&d_status, 10));
  sw.saveDevice(0, n, d_rec);
  std::vector<mrs_uav_snapshot_t> rec((size_t)n), rec2((size_t)n);
  HIP(hipMemcpy(rec.data(), d_rec, sizeof(mrs_uav_snapshot_t) * (size_t)n, hipMemcpyDeviceToHost));
  std::vector<mrs_uav_pose_t> poses = sw.getPoseArray(0, n);
  for (int i = 0; i < n; i++) {
    CHECK(rec[(size_t)i].magic == MRS_SNAP_MAGIC && rec[(size_t)i].airframe == rec[0].airframe && rec[(size_t)i]._reserved == 0u);
    CHECK(std::memcmp(rec[(size_t)i].x, poses[(size_t)i].position, sizeof(double) * 3) == 0);
  }
  std::printf("ok save_equals_pose_array %d\n", n);

  sw.makeSteps(0.001, 150);
  std::vector<mrs_uav_pose_t> later = sw.getPoseArray(0, n);
  CHECK(std::memcmp(later.data(), poses.data(), sizeof(mrs_uav_pose_t) * (size_t)n) != 0);
  sw.loadDevice(0, n, d_rec, n);
  sw.saveDevice(0, n, d_rec2);
  HIP(hipMemcpy(rec2.data(), d_rec2, sizeof(mrs_uav_snapshot_t) * (size_t)n, hipMemcpyDeviceToHost));
  CHECK(std::memcmp(rec.data(), rec2.data(), sizeof(mrs_uav_snapshot_t) * (size_t)n) == 0);
  std::vector<mrs_uav_pose_t> back = sw.getPoseArray(0, n);
  CHECK(std::memcmp(back.data(), poses.data(), sizeof(mrs_uav_pose_t) * (size_t)n) == 0);
  std::printf("ok load_restores_the_save\n");

  // UAVs 20 .. 29 <- record 7, except UAV 25 (index -1) and UAV 26 (index n: out of range)
  std::vector<int32_t> idx(10, 7);
  idx[5] = -1;
  idx[6] = n;
  HIP(hipMemcpy(d_idx, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice));
  sw.loadDevice(20, 10, d_rec, n, d_idx, d_status);
  std::vector<uint8_t> status(10);
  HIP(hipMemcpy(status.data(), d_status, status.size(), hipMemcpyDeviceToHost));
  std::vector<mrs_uav_pose_t> fork = sw.getPoseArray(0, n);
  for (int k = 0; k < 10; k++) {
    const uint8_t want = k == 5 ? MRS_SNAP_SKIPPED : (k == 6 ? MRS_SNAP_BAD_INDEX : MRS_SNAP_LOADED);
    CHECK(status[(size_t)k] == want);
    const mrs_uav_pose_t& expect = want == MRS_SNAP_LOADED ? poses[7] : poses[(size_t)20 + k];
    CHECK(std::memcmp(&fork[(size_t)20 + k], &expect, sizeof(mrs_uav_pose_t)) == 0);
  }
  std::printf("ok fork_through_index\n");

  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "wb");
    CHECK(f);
    CHECK(std::fwrite(rec.data(), sizeof(mrs_uav_snapshot_t), rec.size(), f) == rec.size());
    std::fclose(f);
    std::printf("ok written\n");
  }
  HIP(hipFree(d_rec));
  HIP(hipFree(d_rec2));
  HIP(hipFree(d_idx));
  HIP(hipFree(d_status));
  return 0;
}
