#!/usr/bin/env python3
"""Time of the line-of-sight neighbours against its yardsticks, legs alternating within one run (host clock around windows of
back-to-back calls that end with a device synchronise, after a warm-up; each window is sized to last at least `window` seconds; the
spread of the rounds is printed):

  v  tensors.nearest_visible(k = 8, 5 m, NN_REL_POS | NN_DIST, float32) with index, counts, visible and hidden
  n  tensors.nearest with the same arguments on the same build: the floor — the hash build and a query without any sight line
  o  tensors.nearest_obstacles(k = 8, ON_DIST, float64) at that radius: what a walk of the obstacle grid costs per UAV

on the swarm of tools/obstacle_rate.py (`n` x500 UAVs, 64 m^3 per UAV) among its forests of M = 100 and M = 10 000 obstacles, and on
`worlds` stacked copies of a scene of n / worlds UAVs, one collision world per copy, sharing an all-worlds forest of 100 obstacles.
Besides the times it prints what the call found: the share of hidden pairs, observers that see nobody, the largest counts.

    python tools/nearest_visible_rate.py [n=100000] [worlds=100] [rounds=7] [window=0.3] [--package-root DIR]

--package-root DIR imports mrs_multirotor_simulator_amd from DIR (another checkout with a library of its own) instead of this tree: a
package without nearest_visible is timed on the yardsticks alone.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import obstacle_rate as OR  # noqa: E402  (the swarm, the forests, --package-root)
from obstacle_contact_rate import run_legs  # noqa: E402

RADIUS, K = 5.0, 8


def measure(n, worlds, count, rounds, window):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, scene = OR.make(n, worlds)
    n = g.n
    dev = torch.device("cuda", g.device())
    kinds, centres, sizes, density = OR.forest(scene, count)
    T.set_obstacles(g, kinds, centres, sizes, all_worlds=np.ones(count, bool))
    have = hasattr(T, "nearest_visible")
    fields = T.NN_REL_POS | T.NN_DIST
    rows = torch.empty((n, K * 4), dtype=torch.float32, device=dev)
    index = torch.empty((n, K), dtype=torch.int32, device=dev)
    counts, visible, hidden = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    rows_n = torch.empty((n, K * 4), dtype=torch.float32, device=dev)
    index_n = torch.empty((n, K), dtype=torch.int32, device=dev)
    counts_n = torch.empty(n, dtype=torch.int32, device=dev)
    rows_o = torch.empty((n, K), dtype=torch.float64, device=dev)
    index_o = torch.empty((n, K), dtype=torch.int32, device=dev)
    counts_o = torch.empty(n, dtype=torch.int32, device=dev)
    print(f"  {worlds} world(s), {count} obstacles, {density:.2f} per hectare of footprint", flush=True)

    def leg_v():
        T.nearest_visible(g, K, RADIUS, fields, out=rows, index=index, counts=counts, visible=visible, hidden=hidden)

    def leg_n():
        T.nearest(g, K, RADIUS, fields, out=rows_n, index=index_n, counts=counts_n)

    def leg_o():
        T.nearest_obstacles(g, K, RADIUS, T.ON_DIST, dtype=torch.float64, out=rows_o, index=index_o, counts=counts_o)

    leg_n()
    if have:
        leg_v()
        v, h, c = visible.cpu().numpy().astype(np.int64), hidden.cpu().numpy().astype(np.int64), counts_n.cpu().numpy()
        assert (np.minimum(v + h, K) == c).all()  # visible + hidden are the candidates of nearest
        same = (index.cpu().numpy() == index_n.cpu().numpy()).all(axis=1)
        assert same[h == 0].all()  # and where nothing is hidden the lists are nearest's
        print(f"  {h.sum()} of {(v + h).sum()} pairs hidden ({h.sum() / max((v + h).sum(), 1) * 100:.1f} %), {(~same).sum()} of {n} rows differ "
              f"from nearest, {((h > 0) & (v == 0)).sum()} observers see nobody, most visible {v.max()}, most hidden {h.max()}", flush=True)
    paths = {"v": leg_v, "n": leg_n, "o": leg_o} if have else {"n": leg_n, "o": leg_o}
    what = {"v": "v nearest_visible 5 m k=8 REL_POS|DIST f32, all vectors", "n": "n nearest, the same arguments", "o": "o nearest_obstacles 5 m k=8 DIST f64"}
    med = run_legs(paths, what, rounds, window, dev)
    if have:
        print(f"  v / n = {med['v'] / med['n']:.3f}   v / o = {med['v'] / med['o']:.3f}   v - n = {med['v'] - med['n']:.1f} us", flush=True)
    g.close()


def main():
    args = OR.ARGS
    n = int(args[0]) if len(args) > 0 else 100_000
    worlds = int(args[1]) if len(args) > 1 else 100
    rounds = int(args[2]) if len(args) > 2 else 7
    window = float(args[3]) if len(args) > 3 else 0.3
    print(f"package {os.path.relpath(OR.PKG, OR.ROOT)}; radius {RADIUS} m, k = {K}; {rounds} rounds, windows of at least {window} s", flush=True)
    print(f"{n} UAVs", flush=True)
    for w, count in ((1, 100), (1, 10_000), (worlds, 100)):
        measure(n, w, count, rounds, window)


if __name__ == "__main__":
    main()
