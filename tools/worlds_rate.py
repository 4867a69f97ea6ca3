#!/usr/bin/env python3
"""What collision worlds cost (include/mrs_swarm.h, "collision worlds"; DESIGN §7 / §7c, MEASUREMENTS §7.4).

  (a) search  n x500 UAVs of bench.make_inputs(n, "position+collisions") (64 m^3 per UAV) as ONE world: mrs_swarm_debug_search_ms (pack +
              insert, list-building query) without labels — the kernels a swarm always launched, the figure to hold against the parent
              commit's — and with every label set to 0 explicitly (the world-aware kernels on the same table layout)
  (b) stacked `worlds` copies of the box of n / worlds UAVs on the same coordinates, label i // (n / worlds): the search tick, and
              `ticks` ticks of tick_n (collisions on) in ms per tick.  With MRS_SWARM_LIB pointing at a library built with
              -DMRS_WORLDS_PLAIN_HASH for collide.hip (labels compared but left out of the hashes) the same lines show what the label in
              the bucket hash and the cell tag is worth: every occupied cell is a chain of `worlds` members there
  (c) nearest tensors.nearest (k = 8, radius 5 m, FP32 REL_POS | DIST) at n UAVs without labels, with all labels 0, and on the stacked swarm

    python tools/worlds_rate.py [n=100000] [worlds=100] [ticks=200] [reps=5]
    python -m mrs_multirotor_simulator_amd.build --out variants/libmrs_plain_hash.so --flags collide.hip=-DMRS_WORLDS_PLAIN_HASH
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import mrs_multirotor_simulator_amd as M  # noqa: E402

DT = 0.001


def make(n, copies=1, seed=3):
    st, cmd = bench.make_inputs(n, "position+collisions", seed=seed)
    g = M.Swarm(n * copies, arith=M.ARITH_FAST)
    g.construct(0, n * copies, M.model_params("x500", ground_enabled=True, ground_z=0.0))
    t = lambda a: np.tile(a, (copies,) + (1,) * (a.ndim - 1))
    g.set_state(0, n * copies, t(st["x"]), t(st["v"]), t(st["R"]), t(st["omega"]), t(st["motor_rpm"]))
    g.set_input(0, n * copies, M.POSITION_CMD, t(cmd))
    return g


def med(xs):
    xs = np.array(xs)
    return f"{np.median(xs):9.2f} (min {xs.min():.2f}, max {xs.max():.2f})"


def search_us(g, reps):
    g.debug_search_ms(4)
    return [g.debug_search_ms(20) * 1e3 for _ in range(reps)]


def tick_us(g, ticks, reps):
    g.tick_n(DT, 20, True, False, 100.0)
    g.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        g.tick_n(DT, ticks, True, False, 100.0)
        g.synchronize()
        out.append((time.perf_counter() - t0) / ticks * 1e6)
    return out


def nearest_us(g, reps, calls=20):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    dev = torch.device("cuda", g.device())
    fields, k = T.NN_REL_POS | T.NN_DIST, 8
    out = torch.empty((g.n, T.nearest_width(fields, k)), dtype=torch.float32, device=dev)
    idx, cnt = torch.empty((g.n, k), dtype=torch.int32, device=dev), torch.empty(g.n, dtype=torch.int32, device=dev)
    for _ in range(3):
        T.nearest(g, k, 5.0, fields, out=out, index=idx, counts=cnt)
    torch.cuda.synchronize(dev)
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            T.nearest(g, k, 5.0, fields, out=out, index=idx, counts=cnt)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / calls)
    return us, float(cnt.float().mean())


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    worlds = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    ticks = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    print(f"library {M.swarm.LIB_PATH}", flush=True)
    g = make(n)
    print(f"(a) search, {n} UAVs, one world, no labels      : {med(search_us(g, reps))} us", flush=True)
    print(f"(c) nearest, no labels                          : {med(nearest_us(g, reps)[0])} us per call", flush=True)
    print(f"    {ticks} ticks, no labels                        : {med(tick_us(g, ticks, reps))} us per tick", flush=True)
    g.close()
    if not hasattr(M.load_library(), "mrs_swarm_set_worlds"):
        print("this library has no collision worlds: (a) and (c) without labels only")
        return
    g = make(n)
    g.set_worlds(np.zeros(n, dtype=np.int32))
    print(f"(a) search, {n} UAVs, every label 0 (set)      : {med(search_us(g, reps))} us", flush=True)
    us, listed = nearest_us(g, reps)
    print(f"(c) nearest, every label 0 (set)                : {med(us)} us per call, {listed:.2f} listed per UAV", flush=True)
    print(f"    {ticks} ticks, every label 0 (set)              : {med(tick_us(g, ticks, reps))} us per tick", flush=True)
    g.close()
    m = n // worlds
    g = make(m, worlds)
    g.set_worlds(np.arange(m * worlds, dtype=np.int32) // m)
    print(f"(b) search, {worlds} worlds x {m} UAVs stacked        : {med(search_us(g, reps))} us", flush=True)
    us, listed = nearest_us(g, reps)
    print(f"(c) nearest, stacked                            : {med(us)} us per call, {listed:.2f} listed per UAV", flush=True)
    print(f"(b) {ticks} ticks, stacked                          : {med(tick_us(g, ticks, reps))} us per tick", flush=True)
    print(f"    collision ticks / searches {g.collision_stats()}, fused stats {g.fused_stats()}", flush=True)
    g.close()


if __name__ == "__main__":
    main()
