#!/usr/bin/env python3
"""Time of one range scan that sees other UAVs, legs alternating within one run (host clock around windows of back-to-back calls that end
with a device synchronise, after a warm-up; each window is sized to last at least `window` seconds):

  u16  tensors.range_scan_uavs, scan_ring(16), body frame, ground, FP32 rows, hit values and UAV indices
  u64  tensors.range_scan_uavs, scan_grid(16, 4, 120 deg, 40 deg), the same outputs
  s16  tensors.range_scan on the same swarm and pattern with hit values: what the scan cost before it saw UAVs (u - s: the increment)
  s64  the same with 64 beams
  n    tensors.nearest(k = 32, radius = max_range + 0.4, REL_POS | DIST, FP32) alone: the floor any caller-side merge of a neighbour list
       into the range image pays before its ray tests.  It needs nothing of this feature: the yardstick, never the code under test

on the swarm and the forests of tools/obstacle_rate.py (`n` x500 UAVs, 64 m^3 per UAV; M = 100 and M = 10 000 obstacles, half pillars
without ends, half boxes).  max_range 10 m.  Besides the times it prints what the beams hit.

    python tools/range_scan_uavs_rate.py [n=100000] [rounds=7] [window=0.3] [--package-root DIR]

--package-root DIR imports mrs_multirotor_simulator_amd from DIR (another checkout with a library of its own) instead of this tree: a
package without range_scan_uavs is timed on s16, s64 and n alone — the comparison that shows whether the old calls are what they were.
MRS_SWARM_LIB=variants/libmrs_....so times a compile-time variant of the library (tools/build_variants.sh).
"""
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = [a for a in sys.argv[1:]]
PKG = ROOT
if "--package-root" in ARGS:
    at = ARGS.index("--package-root")
    PKG = os.path.abspath(ARGS[at + 1])
    del ARGS[at:at + 2]
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
sys.path.insert(0, PKG)
import mrs_multirotor_simulator_amd as M  # noqa: E402,F401
import obstacle_rate as OR  # noqa: E402  (the swarm and the forests)

MAX_RANGE, K = 10.0, 32


def measure(n, count, rounds, window):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, scene = OR.make(n, 1)
    n = g.n
    dev = torch.device("cuda", g.device())
    kinds, centres, sizes, density = OR.forest(scene, count)
    T.set_obstacles(g, kinds, centres, sizes, all_worlds=np.ones(count, bool))
    have = hasattr(T, "range_scan_uavs")
    print(f"  {count} obstacles, {density:.2f} per hectare of footprint", flush=True)
    ring, grid = T.scan_ring(16), T.scan_grid(16, 4, math.radians(120.0), math.radians(40.0))
    out = {16: torch.empty((n, 16), dtype=torch.float32, device=dev), 64: torch.empty((n, 64), dtype=torch.float32, device=dev)}
    hit = {b: torch.empty((n, b), dtype=torch.int32, device=dev) for b in (16, 64)}
    uav = {b: torch.empty((n, b), dtype=torch.int32, device=dev) for b in (16, 64)}
    rows = torch.empty((n, K * 4), dtype=torch.float32, device=dev)
    idx = torch.empty((n, K), dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    paths = {}  # (one pattern per swarm: a leg sets its pattern before its windows, outside the clock)
    for b, beams in ((16, ring), (64, grid)):
        if have:
            paths[f"u{b}"] = (lambda b=b: T.range_scan_uavs(g, MAX_RANGE, True, True, out=out[b], hits=hit[b], uavs=uav[b]), beams)
        paths[f"s{b}"] = (lambda b=b: T.range_scan(g, MAX_RANGE, True, True, out=out[b], hits=hit[b]), beams)
    paths["n"] = (lambda: T.nearest(g, K, MAX_RANGE + 0.4, T.NN_REL_POS | T.NN_DIST, out=rows, index=idx, counts=cnt), None)

    def timed(fn, calls):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / calls

    if have:
        T.set_scan_beams(g, grid)
        _, h, w = T.range_scan_uavs(g, MAX_RANGE, True, True, hits=True, uavs=True)
        h = h.cpu().numpy()
        print(f"  64 beams: {np.mean(h == T.UAVSCAN_HIT_UAV) * 100:.1f} % end on a UAV, {np.mean(h >= 0) * 100:.1f} % on an obstacle, "
              f"{np.mean(h == T.SCAN_HIT_GROUND) * 100:.1f} % on the ground, {np.mean(h == T.SCAN_HIT_NONE) * 100:.1f} % on nothing within "
              f"{MAX_RANGE} m", flush=True)
        assert ((w.cpu().numpy() >= 0) == (h == T.UAVSCAN_HIT_UAV)).all()
    calls = {}
    for name, (fn, beams) in paths.items():
        if beams is not None:
            T.set_scan_beams(g, beams)
        timed(fn, 3)  # warm-up
        calls[name] = max(3, math.ceil(window / timed(fn, 3)))
    us = {name: [] for name in paths}
    for _ in range(rounds):
        for name, (fn, beams) in paths.items():
            if beams is not None:
                T.set_scan_beams(g, beams)
            us[name].append(timed(fn, calls[name]) * 1e6)
    what = {"u16": "u16 range_scan_uavs 16 beams + hit + uav", "u64": "u64 range_scan_uavs 64 beams + hit + uav", "s16": "s16 range_scan 16 beams + hit",
            "s64": "s64 range_scan 64 beams + hit", "n": f"n nearest k {K} radius {MAX_RANGE + 0.4} REL_POS|DIST f32"}
    med = {}
    for name in paths:
        t = np.array(us[name])
        med[name] = float(np.median(t))
        print(f"  {what[name]:44s} {med[name]:10.1f} us per evaluation (min {t.min():.1f}, max {t.max():.1f}, spread "
              f"{(t.max() - t.min()) / med[name] * 100:.1f} %, {calls[name]} calls per window)", flush=True)
    if have:
        print(f"  u16 - s16 = {med['u16'] - med['s16']:.1f} us   u64 - s64 = {med['u64'] - med['s64']:.1f} us   u16 / n = {med['u16'] / med['n']:.2f}   "
              f"u64 / n = {med['u64'] / med['n']:.2f}   u64 / u16 = {med['u64'] / med['u16']:.2f}", flush=True)
    g.close()


def main():
    n = int(ARGS[0]) if len(ARGS) > 0 else 100_000
    rounds = int(ARGS[1]) if len(ARGS) > 1 else 7
    window = float(ARGS[2]) if len(ARGS) > 2 else 0.3
    print(f"package {os.path.relpath(PKG, ROOT)}; library {os.environ.get('MRS_SWARM_LIB', 'in-tree')}; max_range {MAX_RANGE} m; {rounds} rounds, "
          f"windows of at least {window} s", flush=True)
    for count in (100, 10_000):
        print(f"{n} UAVs", flush=True)
        measure(n, count, rounds, window)


if __name__ == "__main__":
    main()
