#!/usr/bin/env python3
"""Time of one range scan against a static forest, legs alternating within one run (host clock around windows of back-to-back calls that
end with a device synchronise, after a warm-up; each window is sized to last at least `window` seconds):

  s16  tensors.range_scan, scan_ring(16), body frame, ground, FP32 rows
  s64  tensors.range_scan, scan_grid(16, 4, 120 deg, 40 deg), body frame, ground, FP32 rows
  h64  s64 with the hit indices as well
  c    tensors.nearest_obstacles(k = 8, radius 5 m, REL | DIST, FP32) on the same swarm: the yardstick
  o    tensors.obstacle_cost(radius 5 m, k = 8, HINGE2, accumulate)
  t    (forests of at most 1 000 obstacles) the torch expression a caller writes without the scan: the same ray tests of the 16 beams of
       a chunk of UAVs against every pillar and box ([chunk, 16, M] FP64) and the ground, the minimum below max_range; the chunk is
       sized so that the intermediates stay under 2 GiB.  It needs nothing of this feature: the yardstick, never the code under test

on the swarm and the forests of tools/obstacle_rate.py (`n` x500 UAVs, 64 m^3 per UAV; M = 100 and M = 10 000 obstacles, half pillars
without ends, half boxes).  max_range 10 m.  Besides the times it prints what the beams hit and, from the C++ grid builder's numbers in
obstacle_stats, how many grids were built.

    python tools/range_scan_rate.py [n=100000] [rounds=7] [window=0.3] [--package-root DIR]

--package-root DIR imports mrs_multirotor_simulator_amd from DIR (another checkout with a library of its own) instead of this tree: a
package without range_scan is timed on (c) and (o) alone — their kernels are the same in both, so this compares the host paths.
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
import mrs_multirotor_simulator_amd as M  # noqa: E402
import obstacle_rate as OR  # noqa: E402  (the swarm and the forests)

MAX_RANGE, RADIUS, K = 10.0, 5.0, 8
BUDGET = 2 << 30  # bytes of the FP64 intermediates of leg t
LIVE = 14         # ... of which about this many [chunk, 16, M, 3] blocks are alive at once


def torch_scan(x, R, beams, pillars, boxes, out, chunk):
    """leg t: out[i, b] = the smallest of the pillar, box and ground ranges of beam b of UAV i below MAX_RANGE, else MAX_RANGE"""
    import torch
    pc, pr = pillars
    bc, bh = boxes
    inf = float("inf")
    for a in range(0, x.shape[0], chunk):
        p = x[a:a + chunk]
        u = torch.einsum("ncj,bj->nbc", R[a:a + chunk], beams)  # [c, B, 3]
        d = (p[:, None, :2] - pc[None, :, :2])[:, None]          # [c, 1, Mp, 2]
        uu = (u[..., :2] * u[..., :2]).sum(dim=2)[..., None]     # [c, B, 1]
        b = (d * u[:, :, None, :2]).sum(dim=3)
        cc = (d * d).sum(dim=3) - (pr * pr)[None, None, :]
        disc = b * b - uu * cc
        q = -b + torch.sqrt(disc.clamp(min=0.0))
        t_p = torch.where(cc <= 0.0, 0.0, torch.where((disc >= 0.0) & (b < 0.0), cc / q, inf))
        e = (p[:, None, :] - bc[None, :, :])[:, None]            # [c, 1, Mb, 3]
        t1, t2 = (-bh[None, None] - e) / u[:, :, None, :], (bh[None, None] - e) / u[:, :, None, :]
        enter = torch.minimum(t1, t2).max(dim=3).values.clamp(min=0.0)
        exit_ = torch.maximum(t1, t2).min(dim=3).values
        t_b = torch.where(enter <= exit_, enter, inf)
        t_g = torch.where(p[:, None, 2] <= 0.0, 0.0, torch.where(u[..., 2] < 0.0, p[:, None, 2] / -u[..., 2], inf))
        best = torch.minimum(torch.minimum(t_p.min(dim=2).values, t_b.min(dim=2).values), t_g)
        out[a:a + chunk] = torch.where(best < MAX_RANGE, best, MAX_RANGE)


def measure(n, count, rounds, window):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, scene = OR.make(n, 1)
    n = g.n
    dev = torch.device("cuda", g.device())
    kinds, centres, sizes, density = OR.forest(scene, count)
    T.set_obstacles(g, kinds, centres, sizes, all_worlds=np.ones(count, bool))
    have = hasattr(T, "range_scan")
    print(f"  {count} obstacles, {density:.2f} per hectare of footprint", flush=True)
    rows = torch.empty((n, K * 4), dtype=torch.float32, device=dev)
    idx = torch.empty((n, K), dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    cost = torch.zeros(n, dtype=torch.float64, device=dev)
    paths = {}
    if have:
        ring, grid = T.scan_ring(16), T.scan_grid(16, 4, math.radians(120.0), math.radians(40.0))
        out16 = torch.empty((n, 16), dtype=torch.float32, device=dev)
        out64 = torch.empty((n, 64), dtype=torch.float32, device=dev)
        hit64 = torch.empty((n, 64), dtype=torch.int32, device=dev)

        # (one pattern per swarm: a leg sets its pattern before its windows, outside the clock)
        legs = {"s16": (ring, out16, None), "s64": (grid, out64, None), "h64": (grid, out64, hit64)}
        for name, (beams, out, hits) in legs.items():
            paths[name] = (lambda b=beams, o=out, h=hits: T.range_scan(g, MAX_RANGE, True, True, out=o, hits=h), beams)
    paths["c"] = (lambda: T.nearest_obstacles(g, K, RADIUS, T.ON_REL | T.ON_DIST, out=rows, index=idx, counts=cnt), None)
    paths["o"] = (lambda: T.obstacle_cost(g, RADIUS, K, T.PROX_HINGE2, 1.0, out=cost, accumulate=True), None)
    if have and count <= 1000:
        x = T.gather(g, T.OBS_POS, dtype=torch.float64)
        R = T.gather(g, T.OBS_ROT, dtype=torch.float64).reshape(n, 3, 3)
        pil, box = kinds == OR.CYLINDER, kinds == OR.BOX
        pillars = (torch.tensor(centres[pil], device=dev), torch.tensor(sizes[pil, 0], device=dev))
        boxes = (torch.tensor(centres[box], device=dev), torch.tensor(sizes[box], device=dev))
        tb = torch.tensor(ring, device=dev)
        chunk = max(1, min(n, BUDGET // (8 * LIVE * 16 * count * 3)))
        out_t = torch.empty((n, 16), dtype=torch.float64, device=dev)
        paths["t"] = (lambda: torch_scan(x, R, tb, pillars, boxes, out_t, chunk), None)
        print(f"  leg t in chunks of {chunk} UAVs ({math.ceil(n / chunk)} per evaluation)", flush=True)
        # one evaluation each: the same ranges up to the rounding of the torch expression and the FP32 rows
        T.set_scan_beams(g, ring)
        paths["s16"][0]()
        paths["t"][0]()
        a, b = out16.cpu().numpy().astype(np.float64), out_t.cpu().numpy()
        assert (a < MAX_RANGE).any() and np.allclose(a, b, rtol=1e-5, atol=1e-5), np.abs(a - b).max()

    def timed(fn, calls):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / calls

    if have:
        T.set_scan_beams(g, grid)
        _, h = T.range_scan(g, MAX_RANGE, True, True, hits=True)
        h = h.cpu().numpy()
        print(f"  64 beams: {np.mean(h >= 0) * 100:.1f} % end on an obstacle, {np.mean(h == T.SCAN_HIT_GROUND) * 100:.1f} % on the ground, "
              f"{np.mean(h == T.SCAN_HIT_NONE) * 100:.1f} % on nothing within {MAX_RANGE} m", flush=True)
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
    what = {"s16": "s16 range_scan 16 beams", "s64": "s64 range_scan 64 beams", "h64": "h64 range_scan 64 beams + hits",
            "c": "c nearest_obstacles k 8 REL|DIST f32", "o": "o obstacle_cost HINGE2 accumulate", "t": "t torch expression 16 beams, chunked"}
    med = {}
    for name in paths:
        t = np.array(us[name])
        med[name] = float(np.median(t))
        print(f"  {what[name]:40s} {med[name]:10.1f} us per evaluation (min {t.min():.1f}, max {t.max():.1f}, spread "
              f"{(t.max() - t.min()) / med[name] * 100:.1f} %, {calls[name]} calls per window)", flush=True)
    if have:
        print(f"  s16 / c = {med['s16'] / med['c']:.2f}   s64 / c = {med['s64'] / med['c']:.2f}   s64 / s16 = {med['s64'] / med['s16']:.2f}"
              + (f"   t / s16 = {med['t'] / med['s16']:.1f}" if "t" in med else ""), flush=True)
        print(f"  grids built: {g.obstacle_stats()['grid_builds']}", flush=True)
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
