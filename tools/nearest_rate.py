#!/usr/bin/env python3
"""Device time of one mrs_swarm_nearest_device call (tensors.nearest into preallocated tensors), and what a nearest() call per tick costs
the closed device loop of tools/device_loop_rate.py.

  call  n x500 UAVs of bench.make_inputs(n, "position+collisions") (64 m^3 per UAV), radius 5 m, k = 8 and 32, FP32,
        REL_POS | REL_VEL | DIST: hipEvents on torch's stream around `calls` back-to-back calls, after a warm-up, `reps` rounds;
        median and min-max in us per call
  loop  gather POS -> torch policy -> set_input_device -> one tick (collisions off), with and without a nearest() call (k = 8) per
        tick, alternating: ms per tick

    python tools/nearest_rate.py [sizes=100000,1000000] [calls=50] [reps=5] [loop_n=100000] [loop_ticks=200]

MRS_NN_ORDER=index / sorted picks the lane order of the query kernel (default: sorted records for ranges of at least n/4).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import mrs_multirotor_simulator_amd as M  # noqa: E402

RADIUS = 5.0
DT, K_GAIN, V_MAX = 0.001, 0.8, 3.0


def make(n, seed=3):
    st, cmd = bench.make_inputs(n, "position+collisions", seed=seed)
    g = M.Swarm(n, arith=M.ARITH_FAST)
    g.construct(0, n, M.model_params("x500", ground_enabled=True, ground_z=0.0))
    g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    return g, cmd


def call_rate(n, calls, reps):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, _ = make(n)
    dev = torch.device("cuda", g.device())
    fields = T.NN_REL_POS | T.NN_REL_VEL | T.NN_DIST
    for k in (8, 32):
        out = torch.empty((n, T.nearest_width(fields, k)), dtype=torch.float32, device=dev)
        idx = torch.empty((n, k), dtype=torch.int32, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        for _ in range(5):
            T.nearest(g, k, RADIUS, fields, out=out, index=idx, counts=cnt)
        torch.cuda.synchronize(dev)
        us = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                T.nearest(g, k, RADIUS, fields, out=out, index=idx, counts=cnt)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / calls)
        c = cnt.cpu().numpy()
        us = np.array(us)
        print(f"  n {n:8d}  k {k:2d}: {np.median(us):8.1f} us per call (min {us.min():.1f}, max {us.max():.1f})   "
              f"neighbours listed per UAV {c.mean():.2f}, full rows {np.mean(c == k) * 100:.0f} %", flush=True)
    g.close()


def loop_rate(n, ticks, reps):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    fields = T.NN_REL_POS | T.NN_REL_VEL | T.NN_DIST
    swarms = {}
    for with_nn in (False, True):
        swarms[with_nn] = make(n)
    g0, cmd = swarms[False]
    dev = torch.device("cuda", g0.device())
    goal_t = torch.tensor(cmd[:, :3], device=dev)
    rows = {w: torch.zeros((n, 4), dtype=torch.float64, device=dev) for w in (False, True)}
    out = torch.empty((n, T.nearest_width(fields, 8)), dtype=torch.float32, device=dev)
    idx = torch.empty((n, 8), dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)

    def loop(w, k):
        g = swarms[w][0]
        for _ in range(k):
            x = T.gather(g, T.OBS_POS, dtype=torch.float64)
            if w:
                T.nearest(g, 8, RADIUS, fields, out=out, index=idx, counts=cnt)
            rows[w][:, :3] = torch.clamp(K_GAIN * (goal_t - x), -V_MAX, V_MAX)
            T.set_input(g, M.VELOCITY_HDG_CMD, rows[w])
            g.tick_n(DT, 1, False, False, 100.0)

    for w in (False, True):
        loop(w, 20)
        swarms[w][0].synchronize()
    times = {w: [] for w in (False, True)}
    for _ in range(reps):
        for w in (False, True):
            g = swarms[w][0]
            g.synchronize()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            loop(w, ticks)
            g.synchronize()
            torch.cuda.synchronize(dev)
            times[w].append((time.perf_counter() - t0) / ticks * 1e3)
    for w in (False, True):
        t = np.array(times[w])
        print(f"  device loop {'with' if w else 'without'} nearest (k 8), {n} UAVs: {np.median(t):.3f} ms/tick (min {t.min():.3f}, "
              f"max {t.max():.3f})", flush=True)
    a, b = swarms[False][0].get_states(), swarms[True][0].get_states()
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), f"the nearest calls changed the loop: {f}"
    print("  both loops end bit-identical")


def main():
    sizes = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [100_000, 1_000_000]
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    loop_n = int(sys.argv[4]) if len(sys.argv) > 4 else 100_000
    loop_ticks = int(sys.argv[5]) if len(sys.argv) > 5 else 200
    print(f"nearest per call, radius {RADIUS} m, FP32 REL_POS|REL_VEL|DIST, order {os.environ.get('MRS_NN_ORDER', 'auto')}, "
          f"{calls} calls x {reps} rounds", flush=True)
    for n in sizes:
        call_rate(n, calls, reps)
    if loop_n > 0:
        print(f"closed device loop, {loop_ticks} ticks x {reps} rounds, alternating", flush=True)
        loop_rate(loop_n, loop_ticks, reps)


if __name__ == "__main__":
    main()
