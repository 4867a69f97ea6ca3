// pose_publisher_test.cpp — MultirotorSimulator (include/mrs_multirotor_simulator/multirotor_simulator.hpp) over the real UavSwarm with
// BOTH publishers set: the per-UAV payload (src/uav_system_ros.cpp:278-282) and the pose array (src/multirotor_simulator.cpp:215,
// 365-389).  Both downloads are started behind the same launch every tick, with collisions on and a few UAVs fast enough to make
// the lazily evaluated collision ticks stall.  Every tick's pose array must equal the position / orientation of that tick's wide payload bit for
// bit, with the same stamp and count, one tick late; after flushPublisher() nothing is left in flight.  A twin swarm stepped in lock
// step with synchronous downloads gives the expected pose arrays.  Exit code 0 and "ok ..." lines on success.
#include <cmath>
#include <cstdio>
#include <vector>
#include <mrs_multirotor_simulator/multirotor_simulator.hpp>

using namespace mrs_multirotor_simulator;

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                  \
    }                                                            \
  } while (0)

static bool close_to(double a, double b) { return std::fabs(a - b) <= 1e-9 * std::fmax(1.0, std::fabs(b)); }

// a few UAVs at 170 m/s: they leave their neighbour-list skin within one step
static void make_fast(UavSwarm& s, int n, int n_fast) {
  std::vector<double> x((size_t)n * 3), v((size_t)n * 3), R((size_t)n * 9), w((size_t)n * 3), rpm((size_t)n * MRS_MAX_MOTORS);
  mrs_throw_on_error(mrs_swarm_get_state(s.handle(), 0, n, x.data(), v.data(), nullptr, R.data(), w.data(), rpm.data()));
  for (int u = 0; u < n_fast; u++) v[(size_t)u * 3 + 1] = 170.0;
  mrs_throw_on_error(mrs_swarm_set_state(s.handle(), 0, n, x.data(), v.data(), R.data(), w.data(), rpm.data()));
}

int main() {
  const int                    n = 4000;
  MultirotorModel::ModelParams mp;
  mp.ground_enabled = true;
  mp.ground_z       = 0.0;
  std::vector<Eigen::Vector3d> pos;
  std::vector<double>          hdg;
  for (int i = 0; i < n; i++) {  // 2.5 m grid: neighbours within the collision radius everywhere
    pos.push_back(Eigen::Vector3d(2.5 * (i % 20), 2.5 * ((i / 20) % 20), 10.0 + 2.5 * (i / 400)));
    hdg.push_back(0.37 * i);
  }
  UavSwarm twin(n, -1, true), pub(n, -1, true);
  for (UavSwarm* s : {&twin, &pub}) {
    s->construct(0, n, mp, pos, hdg);
    s->warmUp();
    for (int u = 0; u < n; u++) {
      reference::Position c;
      c.position = Eigen::Vector3d(pos[(size_t)u](0) + 1.0, pos[(size_t)u](1) - 1.0, pos[(size_t)u](2) + 0.5);
      c.heading  = 0.3 + 0.01 * u;
      (*s)[u].setInput(c);
    }
    make_fast(*s, n, 6);
  }

  SimulatorConfig cfg;
  cfg.simulation_rate       = 1000.0;
  cfg.clock_rate            = 250.0;
  cfg.iterate_without_input = true;
  cfg.collisions_enabled    = true;
  cfg.collisions_crash      = false;
  MultirotorSimulator sim(pub, n, cfg);

  std::vector<std::vector<mrs_uav_pose_t>> want;
  std::vector<double>                      stamps;
  std::vector<mrs_uav_output_t>            last_wide;
  double                                   last_wide_stamp = -1.0;
  int                                      last_wide_count = -1;
  int                                      seen_wide = 0, seen_pose = 0, bad = 0, bad_twin = 0;
  sim.setPublisher([&](double t, const void* payload, int count) {
    const mrs_uav_output_t* o = static_cast<const mrs_uav_output_t*>(payload);
    last_wide.assign(o, o + count);  // the pose publisher of the same tick is called right after this one
    last_wide_stamp = t;
    last_wide_count = count;
    seen_wide++;
  });
  sim.setPosePublisher([&](double t, const void* payload, int count) {
    const mrs_uav_pose_t* p = static_cast<const mrs_uav_pose_t*>(payload);
    const size_t          k = (size_t)seen_pose;
    if (count != n || last_wide_count != count || seen_wide != seen_pose + 1 || t != last_wide_stamp || k >= want.size() ||
        std::fabs(t - stamps[k]) > 1e-12) {
      bad++;
    } else {
      for (int u = 0; u < n; u++) {
        for (int j = 0; j < 3; j++) {
          if (p[u].position[j] != last_wide[(size_t)u].position[j]) bad++;
          if (!close_to(p[u].position[j], want[k][(size_t)u].position[j])) bad_twin++;
        }
        for (int j = 0; j < 4; j++) {
          if (p[u].orientation[j] != last_wide[(size_t)u].orientation[j]) bad++;
          if (!close_to(p[u].orientation[j], want[k][(size_t)u].orientation[j])) bad_twin++;
        }
      }
    }
    seen_pose++;
  });

  const int ticks = 240;
  for (int k = 0; k < ticks; k++) {
    twin.makeStep(1.0 / cfg.simulation_rate);
    want.push_back(twin.getPoseArray(0, n));
    twin.handleCollisions(cfg.collisions_enabled, cfg.collisions_crash, cfg.collisions_rebounce);
    stamps.push_back(sim.simTime() + 1.0 / cfg.simulation_rate);
    sim.timerMain();
    CHECK(seen_pose == k && seen_wide == k);  // one tick late
  }
  std::printf("ok both_publishers %d ticks handed out before the flush, %d mismatches against the wide payload, %d against the twin\n", seen_pose, bad, bad_twin);
  CHECK(bad == 0 && bad_twin == 0);
  sim.flushPublisher();
  CHECK(seen_pose == ticks && seen_wide == ticks);
  CHECK(bad == 0 && bad_twin == 0);
  sim.flushPublisher();  // nothing left: a second flush hands out nothing
  CHECK(seen_pose == ticks && seen_wide == ticks);
  int64_t issued = 0, reissued = 0, fused = 0, stalls = 0, replayed = 0, ahead = 0;
  mrs_throw_on_error(mrs_swarm_get_download_stats(pub.handle(), &issued, &reissued));
  mrs_throw_on_error(mrs_swarm_get_fused_stats(pub.handle(), &fused, &stalls, &replayed, &ahead));
  CHECK(issued == 2 * ticks);
  std::printf("ok flushed: %lld packs issued, %lld re-issued after %lld stalls (%lld fused launches)\n", (long long)issued, (long long)reissued,
              (long long)stalls, (long long)fused);
  return 0;
}
