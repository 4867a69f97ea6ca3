#!/usr/bin/env python3
"""The pipelined host loop with the publisher download every tick, three payloads: the wide record (odometry / IMU / range / pose,
136 B per UAV), the pose array alone (publishPoses, 56 B per UAV), and both behind the same launch (what a simulator with both
publishers starts).  Per tick: a staged command block up (n x 4 doubles), one makeStep, the download(s) started behind the step and
waited for after the NEXT tick has been queued — bench.py's io_tick loop (BASELINE configs[2] inputs), with the payload kind varied.
The variants alternate in one process (ticks each after a warm-up, `reps` rounds); prints ms per tick (median, min-max) and the GB/s of
payload downloaded.

    python tools/pose_io_rate.py [n_uavs=100000] [ticks=150] [reps=3]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import mrs_multirotor_simulator_amd as M  # noqa: E402
from mrs_multirotor_simulator_amd.swarm import OUTPUT_DTYPE, POSE_DTYPE  # noqa: E402

DT = 0.001


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 150
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    st, cmd = bench.make_inputs(n, "actuator", seed=3)
    sw = M.Swarm(n, arith=M.ARITH_FAST)
    sw.construct(0, n, M.model_params("x500", ground_enabled=True))
    sw.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    for _ in range(2):  # both row blocks
        sw.input_staging(n, 4)[:] = cmd
        sw.commit_input(0, n, M.ACTUATOR_CMD, 4)

    kinds = {"wide": ((sw.get_outputs_async, sw.outputs_wait),),
             "pose": ((sw.get_poses_async, sw.poses_wait),),
             "both": ((sw.get_outputs_async, sw.outputs_wait), (sw.get_poses_async, sw.poses_wait))}
    payload = {"wide": OUTPUT_DTYPE.itemsize, "pose": POSE_DTYPE.itemsize, "both": OUTPUT_DTYPE.itemsize + POSE_DTYPE.itemsize}

    def loop(calls, k):
        pending = None
        for _ in range(k):
            sw.input_staging(n, 4)
            sw.commit_input(0, n, M.ACTUATOR_CMD, 4)
            sw.step(DT)
            tickets = [start() for start, _ in calls]
            if pending is not None:
                for (_, wait), t in zip(calls, pending):
                    wait(t)
            pending = tickets
        for (_, wait), t in zip(calls, pending):
            wait(t)

    times = {name: [] for name in kinds}
    for name, calls in kinds.items():  # warm-up of every variant (pinned blocks, code objects)
        loop(calls, 20)
    for _ in range(reps):
        for name, calls in kinds.items():
            sw.synchronize()
            t0 = time.perf_counter()
            loop(calls, ticks)
            sw.synchronize()
            times[name].append((time.perf_counter() - t0) / ticks * 1e3)
    print(f"pipelined tick (staged commands up, makeStep, download(s) down), {n} x500 UAVs, {ticks} ticks x {reps} rounds, alternating")
    for name in kinds:
        t = np.array(times[name])
        med = float(np.median(t))
        print(f"  {name:5s} {payload[name]:4d} B/UAV: {med:.3f} ms/tick (min {t.min():.3f}, max {t.max():.3f}), "
              f"{n * payload[name] / (med * 1e-3) / 1e9:.1f} GB/s of payload")
    w, p = np.median(times["wide"]), np.median(times["pose"])
    print(f"  pose / wide = {p / w:.2f} (bytes {POSE_DTYPE.itemsize / OUTPUT_DTYPE.itemsize:.2f})")


if __name__ == "__main__":
    main()
