#!/usr/bin/env python3
"""Device time of the state snapshots (tensors.save / tensors.load into preallocated tensors) against a torch device-to-device copy of the
same record bytes, the floor of a call that moves them.

  save          mrs_swarm_save_device of every UAV: 480 B of state columns in, one 496-B record out per UAV
  load          mrs_swarm_load_device, no index: record k -> UAV k
  load+index    the same through a random permutation (every record read once, in random order)
  torch copy    dst.copy_(src) of n x 496 bytes

n x500 UAVs of bench.make_inputs(n, "position+collisions"); hipEvents on torch's stream around `calls` back-to-back calls after a
warm-up, `reps` rounds, the four kinds alternating within a round; median and min-max in us per call, and the ratio to the copy.
Both kernel forms (MRS_SNAP_FORM=lane / tile, read per call) are timed in the same rounds.

    python tools/state_io_rate.py [sizes=100000,1000000] [calls=20] [reps=5]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import mrs_multirotor_simulator_amd as M  # noqa: E402

FORMS = ("lane", "tile")


def make(n, seed=3):
    st, cmd = bench.make_inputs(n, "position+collisions", seed=seed)
    g = M.Swarm(n, arith=M.ARITH_FAST)
    g.construct(0, n, M.model_params("x500", ground_enabled=True, ground_z=0.0))
    g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    g.set_input(0, n, M.POSITION_CMD, cmd)
    g.step_n(0.001, 3)
    return g


def rate(n, calls, reps):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = make(n)
    dev = torch.device("cuda", g.device())
    rec = T.save(g)
    dst = torch.empty_like(rec)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5)).to(torch.int32).to(dev)
    kinds = {"torch copy": lambda: dst.copy_(rec)}
    for form in FORMS:
        def with_form(fn, form=form):
            def run():
                os.environ["MRS_SNAP_FORM"] = form
                fn()
            return run
        kinds[f"save       {form}"] = with_form(lambda: T.save(g, out=dst))
        kinds[f"load       {form}"] = with_form(lambda: T.load(g, rec, status=status))
        kinds[f"load+index {form}"] = with_form(lambda: T.load(g, rec, index=perm, status=status))
    us = {k: [] for k in kinds}
    for fn in kinds.values():  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize(dev)
    for _ in range(reps):
        for name, fn in kinds.items():
            fn()  # (sets the form before the timed calls)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    os.environ.pop("MRS_SNAP_FORM", None)
    assert (status.cpu().numpy() == T.SNAP_LOADED).all()
    floor = float(np.median(us["torch copy"]))
    mb = n * T.SNAP_BYTES / 1e6
    for name, v in us.items():
        v = np.array(v)
        med = float(np.median(v))
        print(f"  n {n:8d}  {name:16s}: {med:9.1f} us per call (min {v.min():.1f}, max {v.max():.1f})  {med / floor:5.2f}x the copy  "
              f"{2 * mb / med:6.2f} TB/s of 2 x {mb:.0f} MB", flush=True)
    g.close()


def main():
    args = dict(a.split("=", 1) for a in sys.argv[1:])
    sizes = [int(s) for s in args.get("sizes", "100000,1000000").split(",")]
    calls, reps = int(args.get("calls", 20)), int(args.get("reps", 5))
    print(f"state snapshots: {calls} calls per timing, {reps} rounds")
    for n in sizes:
        rate(n, calls, reps)


if __name__ == "__main__":
    main()
