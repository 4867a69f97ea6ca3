#!/usr/bin/env python3
"""Time of one obstacle-cost evaluation against a static forest, four legs alternating within one run (host clock around windows of
back-to-back calls that end with a device synchronise, after a warm-up; each window is sized to last at least `window` seconds):

  a  tensors.obstacle_cost, HINGE2, accumulate, into an FP64 cost vector
  b  the torch expression a caller writes without it: the signed distances of a chunk of UAVs to every obstacle ([chunk, M] FP64), the
     8 smallest below the radius by topk, weight * (radius - sd)^2 summed and added into the same kind of vector; the chunk is sized so
     that the [chunk, M] intermediates stay under 2 GiB.  It needs nothing of this feature: the yardstick, never the code under test
  c  tensors.nearest_obstacles(k, ON_DIST, float64) alone
  d  tensors.proximity_cost on the same swarm (the sibling's scale)

on the swarm of tools/nearest_rate.py (`n` x500 UAVs of bench.make_inputs(n, "position+collisions"), 64 m^3 per UAV) among forests of
M = 100 and M = 10 000 obstacles spread uniformly over the swarm's footprint — half of them pillars without ends (radius 0.3 .. 0.8 m),
half axis-aligned boxes (half-extents 1 .. 3 m) at random heights; the density is printed — and on `worlds` stacked copies of a scene
of n / worlds UAVs, one collision world per copy, sharing one all-worlds forest of 100 obstacles.  Radius 5 m, k = 8.  Besides the times
it prints, from obstacle_stats, the grid of each forest (cells, mean and longest cell list: what a query walks) and how many obstacles
the UAVs have within the radius.

    python tools/obstacle_rate.py [n=100000] [worlds=100] [rounds=7] [window=0.3] [--package-root DIR]

--package-root DIR imports mrs_multirotor_simulator_amd from DIR (another checkout with a library of its own) instead of this tree: a
package without obstacle_cost is timed on (b) and (d) alone.
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
sys.path.insert(0, ROOT)
sys.path.insert(0, PKG)
import bench  # noqa: E402
import mrs_multirotor_simulator_amd as M  # noqa: E402

RADIUS, K, WEIGHT = 5.0, 8, 1.0
CYLINDER, BOX = 2, 1
BUDGET = 2 << 30  # bytes of [chunk, M] FP64 intermediates of leg b
LIVE = 12         # ... of which about this many are alive at once


def make(n, worlds, seed=3):
    """worlds == 1: the swarm of tools/nearest_rate.py; else `worlds` copies of a scene of n // worlds UAVs, one label per copy"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    m = n // worlds
    st, _ = bench.make_inputs(m, "position+collisions", seed=seed)
    g = M.Swarm(m * worlds, arith=M.ARITH_FAST)
    g.construct(0, m * worlds, M.model_params("x500", ground_enabled=True, ground_z=0.0))
    g.set_state(0, m * worlds, *(np.concatenate([st[f]] * worlds) for f in ("x", "v", "R", "omega", "motor_rpm")))
    if worlds > 1:
        labels = torch.arange(m * worlds, dtype=torch.int32, device=torch.device("cuda", g.device())) // m
        T.set_worlds(g, labels)
    return g, np.asarray(st["x"], np.float64)


def forest(x, count, seed=11):
    """(kinds, centres, sizes) of `count` obstacles uniform over the footprint of the positions x: pillars and boxes alternating"""
    rng = np.random.default_rng(seed)
    lo, hi = x.min(axis=0), x.max(axis=0)
    kinds = np.where(np.arange(count) % 2 == 0, CYLINDER, BOX).astype(np.int32)
    centres = rng.uniform(lo, hi, (count, 3))
    sizes = rng.uniform(1.0, 3.0, (count, 3))
    pillar = kinds == CYLINDER
    sizes[pillar, 0] = rng.uniform(0.3, 0.8, pillar.sum())
    sizes[pillar, 2] = np.inf
    area = (hi[0] - lo[0]) * (hi[1] - lo[1])
    return kinds, centres, sizes, count / area * 1e4


def torch_cost(x, pillars, boxes, cost, chunk):
    """leg b: cost += sum over the K nearest obstacles with sd < RADIUS of WEIGHT (RADIUS - sd)^2, chunk by chunk"""
    import torch
    pc, pr = pillars
    bc, bh = boxes
    for a in range(0, x.shape[0], chunk):
        p = x[a:a + chunk]
        d = p[:, None, :2] - pc[None, :, :2]
        sd_p = torch.sqrt((d * d).sum(dim=2)) - pr[None, :]
        q = (p[:, None, :] - bc[None, :, :]).abs() - bh[None, :, :]
        sd_b = torch.sqrt((q.clamp(min=0.0) ** 2).sum(dim=2)) + q.max(dim=2).values.clamp(max=0.0)
        sd = torch.cat([sd_p, sd_b], dim=1)
        near = torch.topk(sd, min(K, sd.shape[1]), dim=1, largest=False).values
        gap = RADIUS - near
        cost[a:a + chunk] += torch.where(near < RADIUS, (WEIGHT * gap) * gap, 0.0).sum(dim=1)


def measure(n, worlds, count, rounds, window):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, scene = make(n, worlds)
    n = g.n
    dev = torch.device("cuda", g.device())
    kinds, centres, sizes, density = forest(scene, count)
    have = hasattr(T, "obstacle_cost")
    if have:
        T.set_obstacles(g, kinds, centres, sizes, all_worlds=np.ones(count, bool))
    x = T.gather(g, T.OBS_POS, dtype=torch.float64)
    pil, box = kinds == CYLINDER, kinds == BOX
    pillars = (torch.tensor(centres[pil], device=dev), torch.tensor(sizes[pil, 0], device=dev))
    boxes = (torch.tensor(centres[box], device=dev), torch.tensor(sizes[box], device=dev))
    chunk = max(1, min(n, BUDGET // (8 * LIVE * count)))
    rows = torch.empty((n, K), dtype=torch.float64, device=dev)
    idx = torch.empty((n, K), dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    cost = {w: torch.zeros(n, dtype=torch.float64, device=dev) for w in "abd"}
    print(f"  {count} obstacles, {density:.2f} per hectare of footprint; leg b in chunks of {chunk} UAVs ({math.ceil(n / chunk)} per evaluation)",
          flush=True)

    def path_a():
        T.obstacle_cost(g, RADIUS, K, T.PROX_HINGE2, WEIGHT, out=cost["a"], accumulate=True)

    def path_b():
        torch_cost(x, pillars, boxes, cost["b"], chunk)

    def path_c():
        T.nearest_obstacles(g, K, RADIUS, T.ON_DIST, dtype=torch.float64, out=rows, index=idx, counts=cnt)

    def path_d():
        T.proximity_cost(g, RADIUS, K, T.PROX_HINGE2, WEIGHT, out=cost["d"], accumulate=True)

    paths = {"a": path_a, "b": path_b, "c": path_c, "d": path_d} if have else {"b": path_b, "d": path_d}

    def timed(fn, calls):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / calls

    if have:  # one evaluation each into fresh vectors: the same penalty up to the rounding of the torch expression
        path_a()
        path_b()
        _, found = T.obstacle_cost(g, RADIUS, K, T.PROX_COUNT, 1.0, found=True)
        a, b, found = cost["a"].cpu().numpy(), cost["b"].cpu().numpy(), found.cpu().numpy()
        assert a.max() > 0 and np.allclose(a, b, rtol=1e-9, atol=1e-9), np.abs(a - b).max()
        st = g.obstacle_stats()
        print(f"  obstacles within the radius per UAV {found.mean():.2f} (most {found.max()}), more than k for {np.mean(found > K) * 100:.1f} %; "
              f"penalty summed over the swarm {a.sum():.6g} (leg a) {b.sum():.6g} (leg b)", flush=True)
        print(f"  grid {st['dims'][0]} x {st['dims'][1]} x {st['dims'][2]} cells of {st['cell_edge']:.1f} m, {st['list_items']} list entries: "
              f"mean list {st['list_items'] / st['cells']:.2f}, longest {st['longest_list']}, {st['grid_builds']} build(s)", flush=True)
    calls = {}
    for name, fn in paths.items():
        timed(fn, 3)  # warm-up
        calls[name] = max(3, math.ceil(window / timed(fn, 3)))
    us = {name: [] for name in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            us[name].append(timed(fn, calls[name]) * 1e6)
    med = {}
    what = {"a": "a obstacle_cost HINGE2 accumulate", "b": "b torch expression, chunked", "c": "c nearest_obstacles DIST f64 alone",
            "d": "d proximity_cost HINGE2 accumulate"}
    for name in paths:
        t = np.array(us[name])
        med[name] = float(np.median(t))
        print(f"  {what[name]:36s} {med[name]:10.1f} us per evaluation (min {t.min():.1f}, max {t.max():.1f}, spread "
              f"{(t.max() - t.min()) / med[name] * 100:.1f} %, {calls[name]} calls per window)", flush=True)
    if have:
        print(f"  b / a = {med['b'] / med['a']:.1f}   a / d = {med['a'] / med['d']:.3f}   a / c = {med['a'] / med['c']:.3f}", flush=True)
    g.close()


def main():
    n = int(ARGS[0]) if len(ARGS) > 0 else 100_000
    worlds = int(ARGS[1]) if len(ARGS) > 1 else 100
    rounds = int(ARGS[2]) if len(ARGS) > 2 else 7
    window = float(ARGS[3]) if len(ARGS) > 3 else 0.3
    print(f"package {os.path.relpath(PKG, ROOT)}; radius {RADIUS} m, k {K}; {rounds} rounds, windows of at least {window} s", flush=True)
    for count in (100, 10_000):
        print(f"one world, {n} UAVs", flush=True)
        measure(n, 1, count, rounds, window)
    if worlds > 1:
        print(f"{worlds} stacked worlds of {n // worlds} UAVs, one all-worlds forest", flush=True)
        measure(n, worlds, 100, rounds, window)


if __name__ == "__main__":
    main()
