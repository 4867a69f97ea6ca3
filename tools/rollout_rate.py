#!/usr/bin/env python3
"""A planner's rollout of T steps through the device-resident loop against one mrs_swarm_rollout_device call.  n x500 UAVs take FP32
command rows of one mode before each step and report FP32 POS | VEL | QUAT rows after it:
  loop     for t: tensors.set_input(cmd[t]); step_n(dt, 1); tensors.gather(out=obs[t])     (three dependent launches, two fences per step)
  rollout  tensors.rollout(cmd, dt, out=obs)                                                 (fused steps; one fence per call)
alternating in one process, per mode and size (a warm-up, then `reps` rounds).  Timed with hipEvents on torch's current stream; prints
us per step (median, min-max).  In LITERAL (the default) both forms must end bit-identical: the tool asserts it (rows and state).  In FAST
the rollout runs the fused kernels and the loop the single-step ones, which differ in the last bits: the tool prints the largest
relative difference of the rows instead.

    python tools/rollout_rate.py [sizes=100000,1000000] [T=64] [reps=5] [modes=ACTUATOR_CMD,ATTITUDE_RATE_CMD,VELOCITY_HDG_CMD] [forms=loop,rollout] [arith=literal] [hold] [obs_every=hold]

(`forms=rollout` runs the rollout alone, e.g. under rocprofv3 --kernel-trace --stats; the bit-identity check then has no partner.)

With a `hold` (and an `obs_every`) the tool measures a CONTROL-RATE rollout instead: each command row is held for `hold` steps and a row
block is due every `obs_every` steps (mrs_swarm_rollout_rate_device).  The same T steps three ways, alternating as above:
  plain    tensors.rollout(cmd.repeat_interleave(hold, 0), dt, out=all T row blocks)         (what a caller did before the rates existed)
  rate     tensors.rollout(cmd, dt, out=T / obs_every row blocks, hold=hold, obs_every=obs_every)
  loop     set_input(cmd[j]) every `hold` steps; step_n(dt, to the next event); gather every `obs_every` steps
and prints the bytes of rows one call of `plain` and of `rate` carries.  In both flavours rows plain[obs_every-1::obs_every] == rate and the
final states must be bit-identical; in LITERAL the loop must equal them too (in FAST its largest relative difference is printed).
`forms` then selects among plain,rate,loop (default: all three; `loop,rollout`, the default above, also means all three).

With `--force-every N` (anywhere on the command line, beside a `hold`) the tool measures the FORCE rollout: a force row block (FP32, a few
newtons per axis) is applied every N steps (mrs_swarm_rollout_force_device).  The same T steps four ways, alternating:
  rate     the rate rollout above on a swarm that has had a zero force applied (so every form reads the force columns)
  force    tensors.rollout(cmd, dt, out=, hold=hold, obs_every=obs_every, forces=frc, force_hold=N)
  force1   the same with force_hold=1 on frc.repeat_interleave(N, 0): a force row per step
  loop     set_input every `hold` steps, apply_force every N steps, step_n(dt, to the next event), gather every `obs_every` steps
`force`, `force1` and `loop` apply the same forces: in LITERAL they must end bit-identical (rows and state), and differ from `rate`.
`forms` selects among rate,force,force1,loop (default: all four).

With `--cost` (anywhere on the command line) the tool measures the COST rollout (mrs_swarm_rollout_cost_device): a quadratic tracking cost
per UAV, evaluated every `cost_every` steps against one shared FP32 target row per evaluation under one shared weight row.  Defaults:
T = 320, modes ACTUATOR_CMD,VELOCITY_HDG_CMD, arith literal,fast, hold 10, and the ninth argument is a list of cost_every (1,10).  The
same T steps three ways, alternating:
  b     tensors.rollout(cmd, dt, out=T / cost_every row blocks, hold=hold, obs_every=cost_every)   (the rows a caller needs for the cost)
  b+    b, then the torch reduction of those rows to one number per UAV: ((rows - target)**2 * weight).sum over evaluations and columns
  f     tensors.rollout_cost(cmd, dt, targets, weights, hold=hold, cost_every=cost_every)
and prints the bytes each form moves between the kernels and the caller's tensors.  A fourth swarm replays the horizon with FP64 rows, in
chunks of 40 steps, and the restatement of the ABI comment is applied to them in torch (element-wise FP64 kernels, one rounding each):
f's cost must equal it bit for bit, and the final states of b and f must agree.

With `--ticks` (anywhere on the command line) the tool measures the TICK rollout (mrs_swarm_rollout_tick_device): T ticks of timerMain —
a step of every UAV, then the collision pass in elastic mode — on the `position+collisions` inputs of bench.py, POSITION_CMD rows held for
`hold` ticks, POS | VEL | QUAT rows (FP32) every `hold` ticks, with and without crash rows.  Defaults: sizes 100000, T = 200, arith fast,
and the seventh argument is a list of holds (1,10).  The same T ticks three ways, alternating, timed with the host clock around work
that ends in a synchronisation of the device:
  tick     tensors.rollout_ticks(cmd, dt, False, 100.0, out=, hold=hold, crashed=)            (one call, one host wait)
  loop     per tick: tensors.set_input every `hold` ticks; step_n(dt, 1); every `hold` ticks tensors.gather and tensors.crashed;
           handle_collisions(True, False, 100.0)                                               (the calls the tick rollout stands for)
  bare     tick_n(dt, T, True, False, 100.0), then synchronize: no commands, no rows              (the floor)
and prints us per tick (median, min-max), the bytes of rows per tick, and whether the call beats the loop in every round.  In LITERAL
`tick` and `loop` must end bit-identical (rows, crash bytes and state): the tool asserts it.  The fifth argument selects among
tick,loop,bare,cost,rows64,feedback,torchloop (e.g. `bare` alone, with MRS_SWARM_LIB naming the library of another commit).  The last two are not in the
default; they measure the COST tick rollout (mrs_swarm_rollout_tick_cost_device) against what a caller did without it:
  cost     tensors.rollout_tick_cost(cmd, dt, False, 100.0, POS | VEL | QUAT, targets [E, 1, 10], weights [1, 10], 1000.0, hold=hold,
           cost_every=hold, out=)                                                                (one call, 8 B per UAV come back)
  rows64   tensors.rollout_ticks with FP64 rows of the same groups and crash rows every `hold` ticks (FP64 commands: one dtype serves
           both), then the torch reduction ((w * d) * d).sum over columns and evaluations + crash_cost * crashed.sum to one number per UAV
With both, the two costs of the first run must agree to 1e-9 relative (the reduction sums in another order).
Two more forms, not in the default either, measure the FEEDBACK tick rollout (mrs_swarm_rollout_tick_feedback_device) against the closed
loop through torch that it replaces:
  feedback   tensors.rollout_tick_feedback(cmd, dt, False, 100.0, POS | VEL | ROT | OMEGA, gains [1, 4, 18], refs [1, n, 18], and the
             cost of `cost`, hold=hold, out=): the command of a block is the nominal row plus G (ref - the 18-column row before the step)
  torchloop  per block: tensors.gather(POS | VEL | ROT | OMEGA) -> cmd + (ref - o) @ G^T (torch.matmul) -> tensors.set_input ->
             tick_n(dt, hold, True, False, 100.0)       (one host wait and one stream fence per block; FP32 rows, no cost)
The largest relative difference of torchloop's final positions from feedback's after the first run is printed (the loop rounds the row to
FP32 and sums in another order).

    python tools/rollout_rate.py --ticks [sizes=100000] [T=200] [reps=5] [-] [forms=tick,loop,bare] [arith=fast] [holds=1,10]

With `--feedback` (anywhere on the command line) the tool measures the FEEDBACK rollout (mrs_swarm_rollout_feedback_device): the command of
a block is the nominal FP32 row plus G (ref - observation row of POS | VEL | ROT | OMEGA, 18 columns), formed in the step kernel, with the
cost of `--cost` evaluated every `hold` steps.  Defaults: sizes 100000, T = 320, modes ACTUATOR_CMD,ATTITUDE_RATE_CMD, arith fast, and the
seventh argument is a list of holds (10,1; cost_every = hold).  The same T steps four ways, alternating:
  c     tensors.rollout_cost(cmd, dt, targets, weights, hold=hold)                              (open loop: what the feedback is added to)
  fs    tensors.rollout_feedback(cmd, dt, fb_groups, gains [1, W_c, 18], refs, ..., hold=hold)   (one gain matrix for all UAVs)
  fu    the same with gains [1, W_c, 18, n], UAV-minor: the shared matrix repeated per UAV        (a gain matrix per UAV)
  loop  per block: tensors.gather(fb_groups) -> cmd + (ref - o) @ G^T (torch.matmul) -> tensors.set_input -> step_n(dt, hold)
        (the closed loop through torch that the call replaces; FP32 rows, no cost)
`fs` and `fu` apply the same gains: cost and final state must be bit-identical, and differ from `c`; the largest relative difference of
the loop's final positions from theirs is printed (the loop rounds the row to FP32 and sums in another order).

    python tools/rollout_rate.py --feedback [sizes=100000] [T=320] [reps=5] [modes=ACTUATOR_CMD,ATTITUDE_RATE_CMD] [forms=c,fs,fu,loop] [arith=fast] [holds=10,1]
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


def commands(mode, n, steps, rng):
    if mode == M.ACTUATOR_CMD:
        return rng.uniform(0.45, 0.6, (steps, n, 4))
    if mode == M.ATTITUDE_RATE_CMD:
        return np.concatenate([rng.uniform(-0.3, 0.3, (steps, n, 3)), rng.uniform(0.5, 0.6, (steps, n, 1))], axis=2)
    return np.concatenate([rng.uniform(-1, 1, (steps, n, 3)), rng.uniform(-0.5, 0.5, (steps, n, 1))], axis=2)


def main():
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    if "--ticks" in sys.argv:
        sys.argv.remove("--ticks")
        return main_ticks([int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [100_000], int(sys.argv[2]) if len(sys.argv) > 2 else 200,
                          int(sys.argv[3]) if len(sys.argv) > 3 else 5, sys.argv[6] if len(sys.argv) > 6 else "fast",
                          [int(h) for h in (sys.argv[7] if len(sys.argv) > 7 else "1,10").split(",")],
                          sys.argv[5].split(",") if len(sys.argv) > 5 else ["tick", "loop", "bare"])
    if "--feedback" in sys.argv:
        sys.argv.remove("--feedback")
        for ar in (sys.argv[6] if len(sys.argv) > 6 else "fast").split(","):
            for hold in [int(h) for h in (sys.argv[7] if len(sys.argv) > 7 else "10,1").split(",")]:
                main_feedback([int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [100_000], int(sys.argv[2]) if len(sys.argv) > 2 else 320,
                              int(sys.argv[3]) if len(sys.argv) > 3 else 5,
                              sys.argv[4].split(",") if len(sys.argv) > 4 and sys.argv[4] != "-" else ["ACTUATOR_CMD", "ATTITUDE_RATE_CMD"],
                              sys.argv[5].split(",") if len(sys.argv) > 5 and sys.argv[5] != "-" else ["c", "fs", "fu", "loop"], ar, hold)
        return None
    cost = "--cost" in sys.argv
    if cost:
        sys.argv.remove("--cost")
    force_every = None
    if "--force-every" in sys.argv:
        k = sys.argv.index("--force-every")
        force_every = int(sys.argv[k + 1])
        del sys.argv[k:k + 2]
    sizes = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [100_000, 1_000_000]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    modes = sys.argv[4].split(",") if len(sys.argv) > 4 else ["ACTUATOR_CMD", "ATTITUDE_RATE_CMD", "VELOCITY_HDG_CMD"]
    forms = sys.argv[5].split(",") if len(sys.argv) > 5 else ["loop", "rollout"]
    arith = sys.argv[6] if len(sys.argv) > 6 else "literal"
    if cost:
        assert force_every is None, "--cost and --force-every exclude each other (no force schedule inside a cost rollout)"
        hold = int(sys.argv[7]) if len(sys.argv) > 7 else 10
        for ar in (sys.argv[6] if len(sys.argv) > 6 else "literal,fast").split(","):
            for every in [int(e) for e in (sys.argv[8] if len(sys.argv) > 8 else "1,10").split(",")]:
                main_cost(sizes, int(sys.argv[2]) if len(sys.argv) > 2 else 320, reps,
                          modes if len(sys.argv) > 4 else ["ACTUATOR_CMD", "VELOCITY_HDG_CMD"], ar, hold, every)
        return None
    if len(sys.argv) > 7:
        hold = int(sys.argv[7])
        every = int(sys.argv[8]) if len(sys.argv) > 8 else hold
        if force_every is not None:
            return main_force(sizes, steps, reps, modes, ["rate", "force", "force1", "loop"] if forms == ["loop", "rollout"] else forms, arith, hold,
                              every, force_every)
        return main_rate(sizes, steps, reps, modes, ["plain", "rate", "loop"] if forms == ["loop", "rollout"] else forms, arith, hold, every)
    assert force_every is None, "--force-every needs a hold"
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_QUAT
    rng = np.random.default_rng(5)
    print(f"rollout of T = {steps} steps, FP32 commands and POS|VEL|QUAT rows, x500, {arith.upper()}; {reps} rounds after a warm-up, alternating")
    for n in sizes:
        st, _ = bench.make_inputs(n, "position+collisions", seed=3)
        p = M.model_params("x500", ground_enabled=True, ground_z=0.0)
        for mode_name in modes:
            mode = getattr(M, mode_name)

            def make():
                g = M.Swarm(n, arith=M.ARITH_FAST if arith == "fast" else M.ARITH_LITERAL)
                g.construct(0, n, p)
                g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
                return g

            swarms = {f: make() for f in forms}
            dev = torch.device("cuda", swarms[forms[0]].device())
            cmd = torch.tensor(commands(mode, n, steps, rng), dtype=torch.float32, device=dev)
            obs = {f: torch.empty((steps, n, T.gather_width(groups)), dtype=torch.float32, device=dev) for f in forms}

            def run(form):
                g = swarms[form]
                if form == "rollout":
                    T.rollout(g, mode, cmd, DT, groups, out=obs[form])
                    return
                for t in range(steps):
                    T.set_input(g, mode, cmd[t])
                    g.step_n(DT, 1)
                    T.gather(g, groups, out=obs[form][t])

            for f in forms:  # warm-up: code objects, the type table, torch kernels
                run(f)
            torch.cuda.synchronize(dev)
            times = {f: [] for f in forms}
            for _ in range(reps):
                for f in forms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(f)
                    e1.record()
                    e1.synchronize()
                    times[f].append(e0.elapsed_time(e1) * 1e3 / steps)
            med = {f: float(np.median(times[f])) for f in forms}
            line = f"  {n:>8d} UAVs  {mode_name:18s}"
            for f in forms:
                line += f"  {f} {med[f]:7.2f} us/step ({min(times[f]):.2f}-{max(times[f]):.2f})"
            if len(forms) == 2:
                line += f"  loop / rollout {med['loop'] / med['rollout']:.2f}x"
                if arith == "fast":
                    a, b = obs["loop"].double(), obs["rollout"].double()
                    line += f"  max rel diff {float(((a - b).abs() / a.abs().clamp_min(1.0)).max()):.1e}"
                    print(line, flush=True)
                    for g in swarms.values():
                        g.close()
                    continue
                assert torch.equal(obs["loop"].view(torch.int32), obs["rollout"].view(torch.int32)), f"{n} {mode_name}: rows differ"
                a, b = swarms["loop"].get_states(), swarms["rollout"].get_states()
                for fld in a.dtype.names:
                    assert np.array_equal(a[fld].view(np.uint64) if a[fld].dtype == np.float64 else a[fld],
                                          b[fld].view(np.uint64) if b[fld].dtype == np.float64 else b[fld]), f"{n} {mode_name}: {fld} differs"
                line += "  bit-identical"
            print(line, flush=True)
            for g in swarms.values():
                g.close()


def bits_equal(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def main_rate(sizes, steps, reps, modes, forms, arith, hold, every):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    assert hold >= 1 and every >= 1 and steps % hold == 0 and steps % every == 0, "hold and obs_every must divide T"
    assert set(forms) <= {"plain", "rate", "loop"}, forms
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_QUAT
    ow = T.gather_width(groups)
    rng = np.random.default_rng(5)
    print(f"control-rate rollout of T = {steps} steps, hold {hold}, obs_every {every}, FP32 commands and POS|VEL|QUAT rows, x500, {arith.upper()}; "
          f"{reps} rounds after a warm-up, alternating")
    for n in sizes:
        st, _ = bench.make_inputs(n, "position+collisions", seed=3)
        p = M.model_params("x500", ground_enabled=True, ground_z=0.0)
        for mode_name in modes:
            mode = getattr(M, mode_name)
            swarms = {}
            for f in forms:
                g = M.Swarm(n, arith=M.ARITH_FAST if arith == "fast" else M.ARITH_LITERAL)
                g.construct(0, n, p)
                g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
                swarms[f] = g
            dev = torch.device("cuda", swarms[forms[0]].device())
            cmd = torch.tensor(commands(mode, n, steps // hold, rng), dtype=torch.float32, device=dev)
            rep = cmd.repeat_interleave(hold, 0) if "plain" in forms else None  # (made once: the caller's copy is not what is timed)
            obs = {f: torch.empty((steps if f == "plain" else steps // every, n, ow), dtype=torch.float32, device=dev) for f in forms}

            def run(form):
                g = swarms[form]
                if form == "plain":
                    T.rollout(g, mode, rep, DT, groups, out=obs[form])
                elif form == "rate":
                    T.rollout(g, mode, cmd, DT, groups, out=obs[form], hold=hold, obs_every=every)
                else:
                    t = 0
                    while t < steps:
                        if t % hold == 0:
                            T.set_input(g, mode, cmd[t // hold])
                        nxt = min((t // hold + 1) * hold, (t // every + 1) * every)
                        g.step_n(DT, nxt - t)
                        t = nxt
                        if t % every == 0:
                            T.gather(g, groups, out=obs[form][t // every - 1])

            for f in forms:  # warm-up: code objects, the type table, torch kernels
                run(f)
            torch.cuda.synchronize(dev)
            times = {f: [] for f in forms}
            for _ in range(reps):
                for f in forms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(f)
                    e1.record()
                    e1.synchronize()
                    times[f].append(e0.elapsed_time(e1) * 1e3 / steps)
            line = f"  {n:>8d} UAVs  {mode_name:18s}"
            for f in forms:
                line += f"  {f} {float(np.median(times[f])):7.2f} us/step ({min(times[f]):.2f}-{max(times[f]):.2f})"
            width = cmd.shape[2]
            if "plain" in forms:
                line += f"  rows plain {(steps * n * (width + ow) * 4) / 1e6:.1f} MB"
            if "rate" in forms:
                line += f"  rows rate {((steps // hold) * n * width + (steps // every) * n * ow) * 4 / 1e6:.1f} MB"

            def same_state(fa, fb):
                a, b = swarms[fa].get_states(), swarms[fb].get_states()
                for fld in a.dtype.names:
                    assert np.array_equal(a[fld].view(np.uint64) if a[fld].dtype == np.float64 else a[fld],
                                          b[fld].view(np.uint64) if b[fld].dtype == np.float64 else b[fld]), f"{n} {mode_name}: {fld} differs ({fa} / {fb})"

            if "plain" in forms and "rate" in forms:
                assert bits_equal(obs["plain"][every - 1::every], obs["rate"]), f"{n} {mode_name}: rows of plain[{every - 1}::{every}] and rate differ"
                same_state("plain", "rate")
                line += "  plain == rate"
            if "loop" in forms and "rate" in forms:
                if arith == "fast":
                    a, b = obs["loop"].double(), obs["rate"].double()
                    line += f"  loop vs rate max rel diff {float(((a - b).abs() / a.abs().clamp_min(1.0)).max()):.1e}"
                else:
                    assert bits_equal(obs["loop"], obs["rate"]), f"{n} {mode_name}: rows of loop and rate differ"
                    same_state("loop", "rate")
                    line += "  loop == rate"
            print(line, flush=True)
            for g in swarms.values():
                g.close()


def main_force(sizes, steps, reps, modes, forms, arith, hold, every, fhold):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    assert min(hold, every, fhold) >= 1 and steps % hold == 0 and steps % every == 0 and steps % fhold == 0, "the three rates must divide T"
    assert set(forms) <= {"rate", "force", "force1", "loop"}, forms
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_QUAT
    ow = T.gather_width(groups)
    rng = np.random.default_rng(5)
    print(f"force rollout of T = {steps} steps, hold {hold}, obs_every {every}, force_every {fhold}, FP32 commands, forces and POS|VEL|QUAT rows, "
          f"x500, {arith.upper()}; {reps} rounds after a warm-up, alternating")
    for n in sizes:
        st, _ = bench.make_inputs(n, "position+collisions", seed=3)
        p = M.model_params("x500", ground_enabled=True, ground_z=0.0)
        for mode_name in modes:
            mode = getattr(M, mode_name)
            swarms = {}
            for f in forms:
                g = M.Swarm(n, arith=M.ARITH_FAST if arith == "fast" else M.ARITH_LITERAL)
                g.construct(0, n, p)
                g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
                g.apply_force(0, n, np.zeros((n, 3)))  # every form reads the force columns from its first step on
                swarms[f] = g
            dev = torch.device("cuda", swarms[forms[0]].device())
            cmd = torch.tensor(commands(mode, n, steps // hold, rng), dtype=torch.float32, device=dev)
            frc = torch.tensor(rng.uniform(-3.0, 3.0, (steps // fhold, n, 3)), dtype=torch.float32, device=dev)
            frc1 = frc.repeat_interleave(fhold, 0) if "force1" in forms else None  # (made once: the caller's copy is not what is timed)
            obs = {f: torch.empty((steps // every, n, ow), dtype=torch.float32, device=dev) for f in forms}

            def run(form):
                g = swarms[form]
                if form == "rate":
                    T.rollout(g, mode, cmd, DT, groups, out=obs[form], hold=hold, obs_every=every)
                elif form == "force":
                    T.rollout(g, mode, cmd, DT, groups, out=obs[form], hold=hold, obs_every=every, forces=frc, force_hold=fhold)
                elif form == "force1":
                    T.rollout(g, mode, cmd, DT, groups, out=obs[form], hold=hold, obs_every=every, forces=frc1, force_hold=1)
                else:
                    t = 0
                    while t < steps:
                        if t % hold == 0:
                            T.set_input(g, mode, cmd[t // hold])
                        if t % fhold == 0:
                            T.apply_force(g, frc[t // fhold])
                        nxt = min((t // hold + 1) * hold, (t // every + 1) * every, (t // fhold + 1) * fhold)
                        g.step_n(DT, nxt - t)
                        t = nxt
                        if t % every == 0:
                            T.gather(g, groups, out=obs[form][t // every - 1])

            for f in forms:  # warm-up: code objects, the type table, torch kernels
                run(f)
            torch.cuda.synchronize(dev)
            times = {f: [] for f in forms}
            for _ in range(reps):
                for f in forms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(f)
                    e1.record()
                    e1.synchronize()
                    times[f].append(e0.elapsed_time(e1) * 1e3 / steps)
            line = f"  {n:>8d} UAVs  {mode_name:18s}"
            for f in forms:
                line += f"  {f} {float(np.median(times[f])):7.2f} us/step ({min(times[f]):.2f}-{max(times[f]):.2f})"
            if "force" in forms and "loop" in forms:
                line += "  force beats loop" if max(times["force"]) < min(times["loop"]) else "  FORCE DOES NOT BEAT LOOP"

            def same_state(fa, fb):
                a, b = swarms[fa].get_states(), swarms[fb].get_states()
                for fld in a.dtype.names:
                    assert np.array_equal(a[fld].view(np.uint64) if a[fld].dtype == np.float64 else a[fld],
                                          b[fld].view(np.uint64) if b[fld].dtype == np.float64 else b[fld]), f"{n} {mode_name}: {fld} differs ({fa} / {fb})"

            if "force" in forms and "force1" in forms:
                assert bits_equal(obs["force"], obs["force1"]), f"{n} {mode_name}: rows of force and force1 differ"
                same_state("force", "force1")
                line += "  force == force1"
            if "force" in forms and "rate" in forms:
                assert not bits_equal(obs["force"], obs["rate"]), f"{n} {mode_name}: the forces moved nothing"
            if "loop" in forms and "force" in forms:
                if arith == "fast":
                    a, b = obs["loop"].double(), obs["force"].double()
                    line += f"  loop vs force max rel diff {float(((a - b).abs() / a.abs().clamp_min(1.0)).max()):.1e}"
                else:
                    assert bits_equal(obs["loop"], obs["force"]), f"{n} {mode_name}: rows of loop and force differ"
                    same_state("loop", "force")
                    line += "  loop == force"
            print(line, flush=True)
            for g in swarms.values():
                g.close()


def main_ticks(sizes, ticks, reps, arith, holds, forms):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_QUAT
    ow = T.gather_width(groups)
    rng = np.random.default_rng(5)
    rebounce = 100.0
    assert set(forms) <= {"tick", "loop", "bare", "cost", "rows64", "feedback", "torchloop"}, forms
    crash_cost = 1000.0
    fb_groups = T.OBS_POS | T.OBS_VEL | T.OBS_ROT | T.OBS_OMEGA
    fw = T.gather_width(fb_groups)
    print(f"tick rollout of T = {ticks} ticks (step + elastic collision pass), POSITION_CMD, FP32 commands and POS|VEL|QUAT rows, x500, "
          f"{arith.upper()}; {reps} rounds after a warm-up, alternating; host clock around a device synchronisation")
    for n in sizes:
        st, goal = bench.make_inputs(n, "position+collisions", seed=3)
        p = M.model_params("x500", ground_enabled=True, ground_z=0.0)
        for hold in holds:
            assert hold >= 1 and ticks % hold == 0, "hold must divide T"
            for crash_rows in ((False, True) if {"tick", "loop"} & set(forms) else (False,)):  # (only tick and loop have optional crash rows)
                swarms = {}
                for f in forms:
                    g = M.Swarm(n, arith=M.ARITH_FAST if arith == "fast" else M.ARITH_LITERAL)
                    g.construct(0, n, p)
                    g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
                    g.set_input(0, n, M.POSITION_CMD, goal)
                    swarms[f] = g
                dev = torch.device("cuda", swarms[forms[0]].device())
                cmd = torch.tensor(goal[None] + rng.normal(0.0, 0.05, (ticks // hold, n, 4)), dtype=torch.float32, device=dev)
                rowless = ("bare", "cost", "feedback", "torchloop")
                obs = {f: torch.empty((ticks // hold, n, ow), dtype=torch.float64 if f == "rows64" else torch.float32, device=dev)
                       for f in forms if f not in rowless}
                cr = {f: torch.zeros((ticks // hold, n), dtype=torch.bool, device=dev) for f in forms if f not in rowless}
                # the cost forms: one shared target row per evaluation around the goal, one weight row; FP64 twins for the torch reduction
                tg = torch.tensor(np.concatenate([goal[:1, :3], np.zeros((1, ow - 3))], axis=1)[None] + rng.normal(0.0, 0.5, (ticks // hold, 1, ow)),
                                  dtype=torch.float32, device=dev)
                wt = torch.tensor(rng.uniform(0.1, 2.0, (1, ow)), dtype=torch.float32, device=dev)
                tg64, wt64, cmd64 = tg.double(), wt.double(), cmd.double() if "rows64" in forms else None
                cost = {f: torch.empty(n, dtype=torch.float64, device=dev) for f in forms if f in ("cost", "rows64", "feedback")}
                # the feedback forms: one small gain matrix for all UAVs, a setpoint row per UAV around its initial state (one block each)
                gain = torch.tensor(rng.normal(0.0, 1e-3, (1, 4, fw)), dtype=torch.float32, device=dev)
                fb_ref = None
                if "feedback" in forms or "torchloop" in forms:
                    fb_ref = (T.gather(swarms[forms[0]], fb_groups) + torch.tensor(rng.normal(0.0, 0.5, (n, fw)), dtype=torch.float32, device=dev))[None]
                    o_row = torch.empty((n, fw), dtype=torch.float32, device=dev)

                def run(form):
                    g = swarms[form]
                    if form == "tick":
                        T.rollout_ticks(g, M.POSITION_CMD, cmd, DT, False, rebounce, groups, out=obs[form], hold=hold,
                                        crashed=cr[form] if crash_rows else False)
                    elif form == "cost":
                        T.rollout_tick_cost(g, M.POSITION_CMD, cmd, DT, False, rebounce, groups, tg, wt, crash_cost, hold=hold, out=cost[form])
                    elif form == "rows64":  # (the crash rows are part of what the caller needs, whatever crash_rows says)
                        T.rollout_ticks(g, M.POSITION_CMD, cmd64, DT, False, rebounce, groups, out=obs[form], hold=hold, crashed=cr[form])
                        d = obs[form] - tg64
                        cost[form].copy_(((wt64 * d) * d).sum(dim=(0, 2)) + crash_cost * cr[form].sum(dim=0))
                    elif form == "feedback":
                        T.rollout_tick_feedback(g, M.POSITION_CMD, cmd, DT, False, rebounce, fb_groups, gain, fb_ref, groups, tg, wt, crash_cost,
                                                hold=hold, out=cost[form])
                    elif form == "torchloop":
                        for b in range(ticks // hold):
                            T.gather(g, fb_groups, out=o_row)
                            T.set_input(g, M.POSITION_CMD, cmd[b] + torch.matmul(fb_ref[0] - o_row, gain[0].t()))
                            g.tick_n(DT, hold, True, False, rebounce)
                    elif form == "bare":
                        g.tick_n(DT, ticks, True, False, rebounce)
                    else:
                        for t in range(ticks):
                            if t % hold == 0:
                                T.set_input(g, M.POSITION_CMD, cmd[t // hold])
                            g.step_n(DT, 1)
                            if (t + 1) % hold == 0:
                                T.gather(g, groups, out=obs[form][t // hold])
                                if crash_rows:
                                    T.crashed(g, out=cr[form][t // hold])
                            g.handle_collisions(True, False, rebounce)
                    g.synchronize()
                    torch.cuda.synchronize(dev)

                for f in forms:  # warm-up: code objects, the type table, torch kernels, the first neighbour search
                    run(f)
                if arith != "fast" and "tick" in forms and "loop" in forms:  # the first run of both forms starts from the same state
                    assert bits_equal(obs["loop"], obs["tick"]) and torch.equal(cr["loop"], cr["tick"]), f"{n} hold {hold}: rows of loop and tick differ"
                    a, b = swarms["loop"].get_states(), swarms["tick"].get_states()
                    for fld in a.dtype.names:
                        assert np.array_equal(a[fld].view(np.uint64) if a[fld].dtype == np.float64 else a[fld],
                                              b[fld].view(np.uint64) if b[fld].dtype == np.float64 else b[fld]), f"{n} hold {hold}: {fld} differs"
                if "cost" in forms and "rows64" in forms:  # (the first run of both forms starts from the same state)
                    assert torch.allclose(cost["cost"], cost["rows64"], rtol=1e-9, atol=0.0), f"{n} hold {hold}: the cost and the reduction of the rows differ"
                fb_diff = None
                if "feedback" in forms and "torchloop" in forms:  # (the first run of both forms starts from the same state)
                    xa, xb = swarms["feedback"].get_states()["x"], swarms["torchloop"].get_states()["x"]
                    fb_diff = float(np.max(np.abs(xa - xb) / np.maximum(np.abs(xa), 1.0)))
                times = {f: [] for f in forms}
                for _ in range(reps):
                    for f in forms:
                        torch.cuda.synchronize(dev)
                        t0 = time.perf_counter()
                        run(f)
                        times[f].append((time.perf_counter() - t0) * 1e6 / ticks)
                line = f"  {n:>8d} UAVs  hold {hold:3d}  crash rows {'yes' if crash_rows else 'no ':3s}"
                for f in forms:
                    line += f"  {f} {float(np.median(times[f])):7.2f} us/tick ({min(times[f]):.2f}-{max(times[f]):.2f})"
                row_bytes = (n * 4 * 4 + n * ow * 4 + (n if crash_rows else 0)) / hold
                line += f"  rows {row_bytes / 1e6:.2f} MB/tick"
                if "tick" in forms and "bare" in forms:
                    line += f"  tick - bare {float(np.median(times['tick'])) - float(np.median(times['bare'])):+.2f} us"
                if "cost" in forms and "bare" in forms:
                    line += f"  cost - bare {float(np.median(times['cost'])) - float(np.median(times['bare'])):+.2f} us"
                if "cost" in forms and "rows64" in forms:
                    line += (f"  rows64 moves {(n * ow * 8 + n) / hold / 1e6:.2f} MB/tick out and back, cost {n * 8 / ticks / 1e6:.4f}"
                             + ("  cost beats rows64" if max(times["cost"]) < min(times["rows64"]) else "  COST DOES NOT BEAT ROWS64"))
                if "feedback" in forms and "bare" in forms:
                    line += f"  feedback - bare {float(np.median(times['feedback'])) - float(np.median(times['bare'])):+.2f} us"
                if "feedback" in forms and "torchloop" in forms:
                    line += (f"  torchloop vs feedback positions {fb_diff:.1e}"
                             + ("  feedback beats torchloop" if max(times["feedback"]) < min(times["torchloop"]) else "  FEEDBACK DOES NOT BEAT TORCHLOOP"))
                if "tick" in forms and "loop" in forms:
                    line += "  tick beats loop" if max(times["tick"]) < min(times["loop"]) else "  TICK DOES NOT BEAT LOOP"
                for f in forms:
                    stats = swarms[f].fused_stats()
                    line += f"  ({f}: {stats[0]} fused launches, {stats[1]} stalls, {stats[2]} replayed, {stats[3]} searches ahead)"
                print(line, flush=True)
                for g in swarms.values():
                    g.close()


def main_cost(sizes, steps, reps, modes, arith, hold, every):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    assert hold >= 1 and every >= 1 and steps % hold == 0 and steps % every == 0, "hold and cost_every must divide T"
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_QUAT
    ow = T.gather_width(groups)
    rng = np.random.default_rng(5)
    forms = ["b", "b+", "f"]
    E = steps // every
    chunk = next(c for c in (40, 20, 10, hold * every) if c % hold == 0 and c % every == 0 and steps % c == 0)
    print(f"cost rollout of T = {steps} steps, hold {hold}, cost_every {every}, FP32 commands, shared FP32 targets and weights, POS|VEL|QUAT, x500, "
          f"{arith.upper()}; {reps} rounds after a warm-up, alternating")
    for n in sizes:
        st, _ = bench.make_inputs(n, "position+collisions", seed=3)
        p = M.model_params("x500", ground_enabled=True, ground_z=0.0)
        for mode_name in modes:
            mode = getattr(M, mode_name)
            swarms = {}
            for f in forms + ["check"]:
                g = M.Swarm(n, arith=M.ARITH_FAST if arith == "fast" else M.ARITH_LITERAL)
                g.construct(0, n, p)
                g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
                swarms[f] = g
            dev = torch.device("cuda", swarms["b"].device())
            cmd = torch.tensor(commands(mode, n, steps // hold, rng), dtype=torch.float32, device=dev)
            tgt = torch.tensor(rng.normal(0.0, 2.0, (E, 1, ow)), dtype=torch.float32, device=dev)
            wt = torch.tensor(rng.uniform(0.1, 2.0, (1, ow)), dtype=torch.float32, device=dev)
            obs = {f: torch.empty((E, n, ow), dtype=torch.float32, device=dev) for f in ("b", "b+")}
            cost = {f: torch.empty(n, dtype=torch.float64 if f == "f" else torch.float32, device=dev) for f in ("b+", "f")}

            def run(form):
                g = swarms[form]
                if form == "f":
                    T.rollout_cost(g, mode, cmd, DT, groups, tgt, wt, hold=hold, cost_every=every, out=cost["f"])
                    return
                T.rollout(g, mode, cmd, DT, groups, out=obs[form], hold=hold, obs_every=every)
                if form == "b+":
                    d = obs[form] - tgt
                    torch.sum(d * d * wt, dim=(0, 2), out=cost["b+"])

            # the reference first (the three timed forms replay this horizon again and again; the check is against their FIRST run):
            # FP64 rows in chunks, the restatement in element-wise FP64 torch kernels
            want = torch.zeros(n, dtype=torch.float64, device=dev)
            t64, w64 = tgt.double(), wt.double()
            for c0 in range(0, steps, chunk):
                rows = T.rollout(swarms["check"], mode, cmd[c0 // hold:(c0 + chunk) // hold].double(), DT, groups, hold=hold, obs_every=every)
                for j in range(chunk // every):
                    term = torch.zeros(n, dtype=torch.float64, device=dev)
                    for col in range(ow):
                        d = rows[j, :, col] - t64[c0 // every + j, 0, col]
                        term = term + (w64[0, col] * d) * d
                    want = want + term
                del rows
            for f in forms:  # warm-up: code objects, the type table, torch kernels — and the run that is checked
                run(f)
            torch.cuda.synchronize(dev)
            nan = torch.isnan(want)
            assert torch.equal(torch.isnan(cost["f"]), nan) and torch.equal(cost["f"][~nan].view(torch.int64), want[~nan].view(torch.int64)), \
                f"{n} {mode_name}: the cost is not the restatement on the FP64 rows"
            for fa, fb in (("b", "f"), ("check", "f")):
                a, b = swarms[fa].get_states(), swarms[fb].get_states()
                for fld in a.dtype.names:
                    assert np.array_equal(a[fld].view(np.uint64) if a[fld].dtype == np.float64 else a[fld],
                                          b[fld].view(np.uint64) if b[fld].dtype == np.float64 else b[fld]), f"{n} {mode_name}: {fld} differs ({fa} / {fb})"
            times = {f: [] for f in forms}
            for _ in range(reps):
                for f in forms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(f)
                    e1.record()
                    e1.synchronize()
                    times[f].append(e0.elapsed_time(e1) * 1e3 / steps)
            line = f"  {n:>8d} UAVs  {mode_name:18s}"
            for f in forms:
                line += f"  {f} {float(np.median(times[f])):7.2f} us/step ({min(times[f]):.2f}-{max(times[f]):.2f})"
            cmd_b, row_b = (steps // hold) * n * cmd.shape[2] * 4, E * n * ow * 4
            line += f"  bytes b {(cmd_b + row_b) / 1e6:.1f} MB, b+ {(cmd_b + 4 * row_b + n * 4) / 1e6:.1f} MB (rows written, read, d*d*w written and read)"
            line += f", f {(cmd_b + 2 * E * n * 8 + 2 * E * ow * 4) / 1e6:.1f} MB (cost element read and written per evaluation)"
            line += "  cost == restatement, states agree"
            line += "  f <= b" if np.median(times["f"]) <= np.median(times["b"]) else "  F SLOWER THAN B"
            print(line, flush=True)
            for g in swarms.values():
                g.close()


def main_feedback(sizes, steps, reps, modes, forms, arith, hold):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    assert hold >= 1 and steps % hold == 0, "hold must divide T"
    fb, groups = T.OBS_POS | T.OBS_VEL | T.OBS_ROT | T.OBS_OMEGA, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT
    wo, ow = T.gather_width(fb), T.gather_width(groups)
    rng = np.random.default_rng(5)
    B = E = steps // hold
    print(f"feedback rollout of T = {steps} steps, hold = cost_every = {hold}, FP32 commands, gains, setpoints, targets and weights, feedback on "
          f"POS|VEL|ROT|OMEGA ({wo} columns), x500, {arith.upper()}; {reps} rounds after a warm-up, alternating")
    for n in sizes:
        st, _ = bench.make_inputs(n, "position+collisions", seed=3)
        p = M.model_params("x500", ground_enabled=True, ground_z=0.0)
        for mode_name in modes:
            mode = getattr(M, mode_name)
            swarms = {}
            for f in forms:
                g = M.Swarm(n, arith=M.ARITH_FAST if arith == "fast" else M.ARITH_LITERAL)
                g.construct(0, n, p)
                g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
                swarms[f] = g
            dev = torch.device("cuda", next(iter(swarms.values())).device())
            cmd = torch.tensor(commands(mode, n, B, rng), dtype=torch.float32, device=dev)
            wc = cmd.shape[2]
            gs = torch.tensor(rng.normal(0.0, 1e-3, (1, wc, wo)), dtype=torch.float32, device=dev)
            gu = gs[..., None].expand(1, wc, wo, n).contiguous()  # UAV-minor
            gt = gs[0].t().contiguous()
            ref = torch.tensor(np.concatenate([[0.0, 0.0, 5.0], np.zeros(3), np.eye(3).ravel(), np.zeros(3)])[None, None, :], dtype=torch.float32, device=dev)
            tgt = torch.tensor(rng.normal(0.0, 2.0, (E, 1, ow)), dtype=torch.float32, device=dev)
            wt = torch.tensor(rng.uniform(0.1, 2.0, (1, ow)), dtype=torch.float32, device=dev)
            cost = {f: torch.empty(n, dtype=torch.float64, device=dev) for f in ("c", "fs", "fu")}
            row = torch.empty((n, wo), dtype=torch.float32, device=dev)

            def run(form):
                g = swarms[form]
                if form == "c":
                    T.rollout_cost(g, mode, cmd, DT, groups, tgt, wt, hold=hold, out=cost["c"])
                elif form in ("fs", "fu"):
                    T.rollout_feedback(g, mode, cmd, DT, fb, gs if form == "fs" else gu, ref, groups, tgt, wt, hold=hold, out=cost[form])
                else:
                    for b in range(B):
                        T.gather(g, fb, out=row)
                        T.set_input(g, mode, torch.addmm(cmd[b], ref[0] - row, gt))
                        g.step_n(DT, hold)

            for f in forms:  # warm-up: code objects, the type table, torch kernels — and the run that is checked
                run(f)
            torch.cuda.synchronize(dev)
            note = ""
            if "fs" in forms and "fu" in forms:
                a, b = swarms["fs"].get_states(), swarms["fu"].get_states()
                for fld in a.dtype.names:
                    assert np.array_equal(a[fld].view(np.uint64) if a[fld].dtype == np.float64 else a[fld],
                                          b[fld].view(np.uint64) if b[fld].dtype == np.float64 else b[fld]), f"{n} {mode_name}: {fld} differs (fs / fu)"
                assert torch.equal(cost["fs"].view(torch.int64), cost["fu"].view(torch.int64)), f"{n} {mode_name}: the costs of fs and fu differ"
                note += "  fs == fu (cost and state)"
                if "c" in forms:
                    assert not torch.equal(cost["fs"], cost["c"]), f"{n} {mode_name}: the feedback changed nothing"
                if "loop" in forms:
                    xl = swarms["loop"].get_states()["x"]
                    note += f"  loop vs fs: max rel. position difference {float(np.nanmax(np.abs(xl - a['x']) / (1.0 + np.abs(a['x'])))):.1e}"
            times = {f: [] for f in forms}
            for _ in range(reps):
                for f in forms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(f)
                    e1.record()
                    e1.synchronize()
                    times[f].append(e0.elapsed_time(e1) * 1e3 / steps)
            line = f"  {n:>8d} UAVs  {mode_name:18s}"
            for f in forms:
                line += f"  {f} {float(np.median(times[f])):7.2f} us/step ({min(times[f]):.2f}-{max(times[f]):.2f})"
            line += f"  gains fs {wc * wo * 4} B, fu {wc * wo * n * 4 / 1e6:.1f} MB read per block" + note
            for f in ("fs", "fu"):
                if f in forms and "loop" in forms and np.median(times[f]) > np.median(times["loop"]):
                    line += f"  {f.upper()} SLOWER THAN THE LOOP"
            print(line, flush=True)
            for g in swarms.values():
                g.close()


if __name__ == "__main__":
    main()
