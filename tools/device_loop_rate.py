#!/usr/bin/env python3
"""A closed loop with a GPU-resident policy against the same loop through the host.  n x500 UAVs in VELOCITY_HDG mode follow a torch /
numpy policy v = clamp(k (goal - x), +-v_max), heading 0:
  device  gather POS into a torch tensor -> torch policy -> set_input_device -> one tick           (mrs_multirotor_simulator_amd.tensors)
  host    get_poses_async / poses_wait -> numpy policy -> input_staging / commit_input -> one tick   (tools/pose_io_rate.py's loop)
each with collisions off and on, alternating in one process (a warm-up, then `reps` rounds of `ticks` ticks).  Prints ms per tick (median,
min-max).  The policy is one correctly rounded subtract, multiply and clamp in FP64, so the two loops must end bit-identical; the tool
asserts it for every pair of swarms.

    python tools/device_loop_rate.py [n_uavs=100000] [ticks=200] [reps=3] [loops=device,host]

(`loops=device` runs the device loop alone, e.g. under rocprofv3 --kernel-trace --stats; the bit-identity check then has no partner.)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import mrs_multirotor_simulator_amd as M  # noqa: E402

DT, K_GAIN, V_MAX = 0.001, 0.8, 3.0


def main():
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    kinds = sys.argv[4].split(",") if len(sys.argv) > 4 else ["device", "host"]
    st, cmd = bench.make_inputs(n, "position+collisions", seed=3)
    goal = cmd[:, :3]
    p = M.model_params("x500", ground_enabled=True, ground_z=0.0)

    def make():
        g = M.Swarm(n, arith=M.ARITH_FAST)
        g.construct(0, n, p)
        g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
        return g

    swarms = {(kind, coll): make() for kind in kinds for coll in (False, True)}
    dev = torch.device("cuda", swarms[kinds[0], False].device())
    goal_t = torch.tensor(goal, device=dev)
    rows_t = {coll: torch.zeros((n, 4), dtype=torch.float64, device=dev) for coll in (False, True)}

    def device_loop(g, coll, k):
        rows = rows_t[coll]
        for _ in range(k):
            x = T.gather(g, T.OBS_POS, dtype=torch.float64)
            rows[:, :3] = torch.clamp(K_GAIN * (goal_t - x), -V_MAX, V_MAX)
            T.set_input(g, M.VELOCITY_HDG_CMD, rows)
            g.tick_n(DT, 1, coll, False, 100.0)

    def host_loop(g, coll, k):
        for _ in range(k):
            pos = g.poses_wait(g.get_poses_async())["position"]
            rows = g.input_staging(n, 4)
            rows[:, :3] = np.clip(K_GAIN * (goal - pos), -V_MAX, V_MAX)
            rows[:, 3] = 0.0
            g.commit_input(0, n, M.VELOCITY_HDG_CMD, 4)
            g.tick_n(DT, 1, coll, False, 100.0)

    loops = {"device": device_loop, "host": host_loop}
    for (kind, coll), g in swarms.items():  # warm-up: code objects, pinned blocks, torch kernels, the first neighbour search
        loops[kind](g, coll, 20)
        g.synchronize()
    torch.cuda.synchronize(dev)
    times = {key: [] for key in swarms}
    for _ in range(reps):
        for (kind, coll), g in swarms.items():
            g.synchronize()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            loops[kind](g, coll, ticks)
            g.synchronize()
            torch.cuda.synchronize(dev)
            times[kind, coll].append((time.perf_counter() - t0) / ticks * 1e3)
    print(f"closed loop (observe -> policy -> command -> one tick), {n} x500 UAVs in VELOCITY_HDG, {ticks} ticks x {reps} rounds, alternating")
    med = {}
    for (kind, coll), t in times.items():
        t = np.array(t)
        med[kind, coll] = float(np.median(t))
        fused, stalls, replayed, _ = swarms[kind, coll].fused_stats()
        print(f"  {kind:6s} loop, collisions {'on ' if coll else 'off'}: {med[kind, coll]:.3f} ms/tick (min {t.min():.3f}, max {t.max():.3f})"
              + (f"  [{fused} fused launches, {stalls} stalls, {replayed} replayed]" if coll else ""))
    if len(kinds) < 2:
        return
    for coll in (False, True):
        print(f"  host / device, collisions {'on ' if coll else 'off'}: {med['host', coll] / med['device', coll]:.1f}x")
        a, b = swarms["device", coll].get_states(), swarms["host", coll].get_states()
        for f in a.dtype.names:
            assert np.array_equal(a[f], b[f]), f"device and host loops differ (collisions {coll}): {f}"
    print("  the device and host loops end bit-identical")


if __name__ == "__main__":
    main()
