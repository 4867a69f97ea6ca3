#!/usr/bin/env python3
"""Time of one separation-penalty evaluation, three ways, alternating within one run (host clock around windows of back-to-back calls that
end with a device synchronise, after a warm-up; each window is sized to last at least `window` seconds):

  a  tensors.proximity_cost, HINGE2, accumulate, into an FP64 cost vector
  b  the path it replaces: tensors.nearest(k, NN_DIST, float64) into preallocated tensors, then the torch hinge reduction
     (weight * (radius - d)^2 over the listed slots) added into the same kind of vector
  c  tensors.nearest(k, NN_DIST, float64) alone

on two swarms: `n` x500 UAVs of bench.make_inputs(n, "position+collisions") (64 m^3 per UAV, nearest's reference point), and `worlds`
stacked copies of a scene of n / worlds UAVs on the same coordinates, one collision world per copy.  Radius 5 m, k = 8.

    python tools/proximity_rate.py [n=100000] [worlds=100] [rounds=7] [window=0.3] [--package-root DIR]

--package-root DIR imports mrs_multirotor_simulator_amd from DIR (another checkout with a library of its own, e.g. the parent commit)
instead of this tree: a package without proximity_cost is timed on (c) alone, which is how (c) is compared across commits (alternate
the two command lines).
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
    return g


def measure(n, worlds, rounds, window):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = make(n, worlds)
    n = g.n
    dev = torch.device("cuda", g.device())
    rows = torch.empty((n, K), dtype=torch.float64, device=dev)
    idx = torch.empty((n, K), dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    slot = torch.arange(K, device=dev)[None, :]
    cost = {w: torch.zeros(n, dtype=torch.float64, device=dev) for w in "ab"}

    def path_a():
        T.proximity_cost(g, RADIUS, K, T.PROX_HINGE2, WEIGHT, out=cost["a"], accumulate=True)

    def path_b():
        T.nearest(g, K, RADIUS, T.NN_DIST, dtype=torch.float64, out=rows, index=idx, counts=cnt)
        gap = RADIUS - rows
        cost["b"].add_(torch.where(slot < cnt[:, None], (WEIGHT * gap) * gap, 0.0).sum(dim=1))

    def path_c():
        T.nearest(g, K, RADIUS, T.NN_DIST, dtype=torch.float64, out=rows, index=idx, counts=cnt)

    paths = {"c": path_c}
    if hasattr(T, "proximity_cost"):
        paths = {"a": path_a, "b": path_b, "c": path_c}

    def timed(fn, calls):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / calls

    if "a" in paths:  # one evaluation each into fresh vectors: the same penalty up to the order of the torch sum
        path_a()
        path_b()
        a, b, found = cost["a"].cpu().numpy(), cost["b"].cpu().numpy(), cnt.cpu().numpy()
        assert a.max() > 0 and np.allclose(a, b, rtol=1e-12, atol=0.0), np.abs(a - b).max()
        print(f"  neighbours listed per UAV {found.mean():.2f}, full rows {np.mean(found == K) * 100:.0f} %; penalty summed over the swarm "
              f"{a.sum():.6g} (path a) {b.sum():.6g} (path b)", flush=True)
    calls = {}
    for name, fn in paths.items():
        timed(fn, 20)  # warm-up
        calls[name] = max(20, math.ceil(window / timed(fn, 20)))
    us = {name: [] for name in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            us[name].append(timed(fn, calls[name]) * 1e6)
    med = {}
    what = {"a": "a proximity_cost HINGE2 accumulate", "b": "b nearest DIST f64 + torch hinge", "c": "c nearest DIST f64 alone"}
    for name in paths:
        t = np.array(us[name])
        med[name] = float(np.median(t))
        print(f"  {what[name]:36s} {med[name]:8.1f} us per evaluation (min {t.min():.1f}, max {t.max():.1f}, spread "
              f"{(t.max() - t.min()) / med[name] * 100:.1f} %, {calls[name]} calls per window)", flush=True)
    if "a" in paths:
        print(f"  a / b = {med['a'] / med['b']:.3f}   a / c = {med['a'] / med['c']:.3f}", flush=True)
    g.close()


def main():
    n = int(ARGS[0]) if len(ARGS) > 0 else 100_000
    worlds = int(ARGS[1]) if len(ARGS) > 1 else 100
    rounds = int(ARGS[2]) if len(ARGS) > 2 else 7
    window = float(ARGS[3]) if len(ARGS) > 3 else 0.3
    print(f"package {os.path.relpath(PKG, ROOT)}; radius {RADIUS} m, k {K}; {rounds} rounds, windows of at least {window} s", flush=True)
    print(f"one world, {n} UAVs", flush=True)
    measure(n, 1, rounds, window)
    if worlds > 1:
        print(f"{worlds} stacked worlds of {n // worlds} UAVs", flush=True)
        measure(n, worlds, rounds, window)


if __name__ == "__main__":
    main()
