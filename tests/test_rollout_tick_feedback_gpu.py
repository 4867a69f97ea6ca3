"""Feedback tick rollouts on the GPU (include/mrs_swarm.h, "feedback tick rollouts"; tensors.rollout_tick_feedback): a cost tick rollout
whose command rows are nominal commands — at the start of every command block the fused step + collision kernel forms
cmd_row + G (ref_row - obs_row) from the state before the step — with the evaluation of the cost tick rollout beside it, or none at all.

The reference is always a twin swarm driven through the loop the call stands for (`fb_tick_loop`: per command block gather(float64) ->
test_rollout_feedback_gpu.restate_feedback in numpy on the host -> set_input; per tick step / gather + crashed / handle_collisions) and
test_rollout_tick_cost_gpu.restate_ticks over its FP64 rows and crash bytes.  Every comparison is bit for bit (a NaN cost must be a NaN),
and the two swarms must be in the same state afterwards (assert_same_swarm: state, IMU, PID, external force, crash flags, diag
counters) — which also compares the commands, through the PID state and the motors they drive.  All in LITERAL unless a test says
FAST; FAST is compared with the FAST loop, which needs no tolerance either: the law and the evaluation are uncontracted FP64 in both
step units and the loop's steps are the same FAST steps — in the cases in which the loop and the call evaluate every collision tick's force
in the same place (test_fast says which, and why FAST bits depend on it for every call with collision ticks in it).

Sizes: the 256-UAV pair swarm of test_rollout_tick_gpu (four 64-UAV blocks, 16 head-on pairs that meet around tick 20) and the variant
swarm of test_rollout_gpu (three airframes, mixed-airframe blocks, a ragged tail, held, crashed and NaN-rollback UAVs inside the
range); horizons of at most 48 ticks.  Gains are small (1e-3 per column, 1e-7 on the rpm columns) and the pair swarm's setpoints lie
around its own state, so that the closed loops stay finite and the pairs still meet: the tests check that on the loop's crash rows.

ROLLOUT_TICK_FEEDBACK_KERNELS maps every entry point of rollout_tick_feedback_device.inc to the tests that force it
(test_rollout_tick_feedback.py keeps the table complete)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import test_rollout_gpu as R
from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_rollout_cost_gpu import cost_equal
from test_rollout_feedback_gpu import restate_feedback
from test_rollout_gpu import COUNT, DT, FIRST, REBOUNCE, commands, same, variant_swarm
from test_rollout_tick_cost_gpu import assert_cost, make_targets, restate_ticks
from test_rollout_tick_gpu import N_PAIR, PAIRS, assert_same_swarm, pair_state, pair_swarm
from test_step_variants_gpu import N_SINGLE

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 300
SENTINEL = -12345.678

# which tests force each entry point of rollout_tick_feedback_device.inc (both flavours)
ROLLOUT_TICK_FEEDBACK_KERNELS = {
    "mrs_uav_rollout_tick_feedback_buf": ("test_equals_the_loop[crash]", "test_equals_the_loop[elastic]", "test_fast", "test_accumulate_and_cutting[FAST]"),
    "mrs_uav_model_rollout_tick_feedback_buf": ("test_equals_the_loop[crash]", "test_equals_the_loop[elastic]"),
    "mrs_uav_rollout_tick_feedback": ("test_pointer_form",),
    "mrs_uav_rollout_tick_feedback_mixed": ("test_equals_the_loop[crash]", "test_equals_the_loop[elastic]", "test_pointer_form"),
}

_dead = []  # the first child process that died by a signal or timed out: nothing more is started on the GPU

RATES = ((1, 1), (4, 2), (3, 6), (48, 48))  # (hold, cost_every)


def configs():
    """n_ticks in (1, 5, 48) with every pair of rates that divides it"""
    return [(t, h, e) for t in (1, 5, 48) for h, e in RATES if t % h == 0 and t % e == 0]


def fb_forms(T):
    """(fb_groups, per-UAV gains, a gain block per command block, shared setpoints, a setpoint block per command block)"""
    return ((T.OBS_POS | T.OBS_VEL | T.OBS_ROT | T.OBS_OMEGA, True, True, False, True), (T.OBS_ALL, False, False, True, False),
            (T.OBS_POS | T.OBS_VEL, True, False, True, True), (T.OBS_VEL_BODY | T.OBS_QUAT | T.OBS_IMU | T.OBS_RPM, False, True, False, False))


def cost_forms(T):
    """(cost_groups, shared targets, one weight row, crash_cost), or None: OBS_ALL, a subset, the crash cost alone, and no cost at all"""
    return ((T.OBS_ALL, False, False, 1000.0), (T.OBS_ALL, True, True, 0.1), (0, None, None, 1000.0),
            (T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, False, True, 0.1), None)


def draw(rng, mode, form, B, count, dtype, dev, centre=None, scale=1e-3, n_cols=10):
    """gains of `form` in the layout of the call, small enough that the closed loop stays finite over a test's horizon (the rpm columns
    are thousands: smaller still), and setpoints: around `centre` ([count, W_o], the swarm's own rows) when given, else near the flight
    envelope.  Returns (gains, refs) as tensors of `dtype`"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    fb_groups, per_uav, gain_blocks, shared_refs, ref_blocks = form
    wo, wc = T.gather_width(fb_groups), T.command_width(mode, n_cols)
    col = np.full(wo, scale)
    if fb_groups & T.OBS_RPM:
        col[-T.MAX_MOTORS:] = scale * 1e-4
    g = rng.normal(0.0, 1.0, (B if gain_blocks else 1, wc, wo) + ((count,) if per_uav else ())) * (col[:, None] if per_uav else col)
    r = rng.normal(0.0, 0.5 if centre is not None else 2.0, (B if ref_blocks else 1, 1 if shared_refs else count, wo))
    if centre is not None:
        r = r + (centre.mean(axis=0)[None, None] if shared_refs else centre[None])
    return torch.tensor(g, dtype=dtype, device=dev), torch.tensor(r, dtype=dtype, device=dev)


def fb_tick_loop(g, mode, cmd, fb_groups, gains, refs, cost_groups, first, hold, every, crash, rows=True):
    """the loop of the contract, through tensors, on swarm g: (FP64 rows of cost_groups [E, count, w] as numpy or None, crash rows [E,
    count] as numpy or None).  FP32 inputs are widened, which is exact"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    dev = cmd.device
    blocks, count = cmd.shape[0], cmd.shape[1]
    ticks = blocks * hold
    cn, gn, rn = (t.double().cpu().numpy() for t in (cmd, gains, refs))
    out = torch.empty((ticks // every, count, T.gather_width(cost_groups)), dtype=torch.float64, device=dev) if cost_groups and rows else None
    cr = torch.empty((ticks // every, count), dtype=torch.bool, device=dev) if rows else None
    for t in range(ticks):
        if t % hold == 0:
            o = T.gather(g, fb_groups, first, count, dtype=torch.float64).cpu().numpy()  # the state before the step; a pending collision tick stays pending
            T.set_input(g, mode, torch.tensor(restate_feedback(o, cn, gn, rn, t // hold), device=dev), first)
        g.step_n(DT, 1)  # evaluates the collision tick pending from tick t - 1
        if rows and (t + 1) % every == 0:
            j = (t + 1) // every - 1
            if out is not None:
                T.gather(g, cost_groups, first, count, out=out[j])
            T.crashed(g, first, count, out=cr[j])
        g.handle_collisions(True, crash, REBOUNCE)  # stays pending
    return (None if out is None else out.cpu().numpy()), (None if cr is None else cr.cpu().numpy())


def loop_cost(g, mode, cmd, fb_groups, gains, refs, cost, first, hold, every, crash, tg, wt, start=None):
    """the loop on swarm g and the restatement of the evaluation: (cost or None, crash rows, FP64 rows or None).  cost: a cost form"""
    rows, cr = fb_tick_loop(g, mode, cmd, fb_groups, gains, refs, cost[0] if cost else 0, first, hold, every, crash)
    if cost is None:
        return None, cr, None
    want = restate_ticks(rows, cr, None if tg is None else tg.cpu().numpy(), None if wt is None else wt.cpu().numpy(), cost[3], start)
    return want, cr, rows


def call(T, g, mode, cmd, crash, fb_groups, gains, refs, cost, tg, wt, **kw):
    """tensors.rollout_tick_feedback with a cost form: the crash cost alone needs its `out`, no cost at all returns None"""
    if cost is None:
        got = T.rollout_tick_feedback(g, mode, cmd, DT, crash, REBOUNCE, fb_groups, gains, refs, **kw)
        assert got is None
        return None
    if cost[0] == 0 and "out" not in kw:
        import torch
        kw["out"] = torch.full((cmd.shape[1],), SENTINEL, dtype=torch.float64, device=cmd.device)
    return T.rollout_tick_feedback(g, mode, cmd, DT, crash, REBOUNCE, fb_groups, gains, refs, cost[0], tg, wt, cost[3], **kw)


def pair_inputs(T, rng, a, blocks, dtype, form, cost, evals, noise=0.01):
    """nominal POSITION_CMD rows at the pair swarm's own positions, gains and setpoints of `form` around its own rows, targets likewise"""
    import torch
    dev = torch_dev(a)
    pos, _ = pair_state()
    c = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, noise, (blocks, N_PAIR, 4))
    cmd = torch.tensor(c, dtype=dtype, device=dev)
    centre = T.gather(a, form[0], 0, N_PAIR, dtype=torch.float64).cpu().numpy()
    gains, refs = draw(rng, O.POSITION_CMD, form, blocks, N_PAIR, dtype, dev, centre, n_cols=4)
    tg = wt = None
    if cost and cost[0]:
        tc = T.gather(a, cost[0], 0, N_PAIR, dtype=torch.float64).cpu().numpy()
        tg, wt = make_targets(rng, evals, N_PAIR, T.gather_width(cost[0]), dtype, dev, cost[1], cost[2], tc)
    return cmd, gains, refs, tg, wt


@pytest.mark.parametrize("crash", [True, False], ids=["crash", "elastic"])
def test_equals_the_loop(mrs, crash):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(271)
    FB, CF = fb_forms(T), cost_forms(T)
    run, seen_fb, seen_cost = 0, set(), set()
    # ---- variant swarm: every configuration, one after the other on the same two swarms; dtypes and forms take turns
    for scen, modes in (("cascade", (O.VELOCITY_HDG_CMD, O.ACTUATOR_CMD)), ("model", (O.ACTUATOR_CMD,))):
        a, b = variant_swarm(mrs, scen, mrs.ARITH_LITERAL), variant_swarm(mrs, scen, mrs.ARITH_LITERAL)
        assert np.asarray(a.has_crashed())[FIRST:].any(), "the scenario has crashed UAVs in the range"
        dev = torch_dev(a)
        paid = False
        for mode in modes:
            for ticks, hold, every in configs():
                dtype = (torch.float64, torch.float32)[(run // 4) % 2]
                form, cost = FB[run % len(FB)], CF[run % len(CF)]
                seen_fb.add((dtype, form))
                seen_cost.add((dtype, cost))
                run += 1
                x = a.get_states(FIRST, COUNT)["x"]
                B = ticks // hold
                cmd = torch.tensor(commands(mode, rng, B, COUNT, x), dtype=dtype, device=dev)
                gains, refs = draw(rng, mode, form, B, COUNT, dtype, dev, n_cols=cmd.shape[2])
                E = ticks // every
                tg, wt = make_targets(rng, E, COUNT, T.gather_width(cost[0]), dtype, dev, cost[1], cost[2]) if cost and cost[0] else (None, None)
                want, cr, _ = loop_cost(a, mode, cmd, form[0], gains, refs, cost, FIRST, hold, every, crash, tg, wt)
                got = call(T, b, mode, cmd, crash, form[0], gains, refs, cost, tg, wt, first=FIRST, hold=hold, cost_every=every)
                what = f"variant {scen} {dtype} mode {mode} T={ticks} hold={hold} cost_every={every} fb={form} cost={cost}"
                if cost is not None:
                    assert_cost(got, want, what)
                assert_same_swarm(a, b, what)
                assert cr.any(), f"{what}: crashed UAVs in the range"
                paid = paid or cost is not None
        assert paid
        print(f"variant {scen} crash={crash}: fused_stats of the calls' swarm {b.fused_stats()}, of the loop's {a.fused_stats()}")
        for g in (a, b):
            g.tick_n(DT, 9, True, crash, REBOUNCE)
        assert_same_swarm(a, b, f"variant {scen}: 9 ticks after the calls")
    assert len(seen_fb) == 2 * len(FB) and len(seen_cost) == 2 * len(CF), "both dtypes met every feedback form and every cost form"
    # ---- pair swarm: fresh swarms per configuration (the pairs meet once), fused launches
    for mixed in (False, True):
        for ticks, hold, every in (configs() if not mixed else [(48, 4, 2), (48, 1, 1)]):
            dtype = torch.float32 if (ticks, hold, every) == (48, 4, 2) and not mixed else torch.float64
            form, cost = FB[run % len(FB)], CF[run % len(CF)] if (hold, every) != (1, 1) or ticks < 48 else CF[0]
            run += 1
            a, b = pair_swarm(mrs, mrs.ARITH_LITERAL, mixed), pair_swarm(mrs, mrs.ARITH_LITERAL, mixed)
            E = ticks // every
            cmd, gains, refs, tg, wt = pair_inputs(T, rng, a, ticks // hold, dtype, form, cost, E)
            fused0 = b.fused_stats()[0]
            want, cr, rows = loop_cost(a, O.POSITION_CMD, cmd, form[0], gains, refs, cost, 0, hold, every, crash, tg, wt)
            got = call(T, b, O.POSITION_CMD, cmd, crash, form[0], gains, refs, cost, tg, wt, hold=hold, cost_every=every)
            what = f"pair mixed={mixed} {dtype} T={ticks} hold={hold} cost_every={every} fb={form} cost={cost}"
            if cost is not None:
                assert_cost(got, want, what)
            assert_same_swarm(a, b, what)
            assert b.fused_stats()[0] - fused0 >= ticks - 1, f"{what}: the ticks after the first are fused launches"
            if ticks == 48:
                # the conditions, on the loop's own crash rows: the gains are small enough that the pairs still meet
                if crash:
                    assert cr[-1, :2 * PAIRS].all() and not cr[:, 2 * PAIRS:].any(), what
                else:
                    assert not cr.any() and np.abs(a.get_external_force()[:2 * PAIRS]).sum() > 0, what
                if crash and (hold, every) == (1, 1):
                    j0 = np.argmax(cr, axis=0)[:2 * PAIRS]
                    assert ((j0 > 0) & (j0 < E - 1)).all() and cr[j0, np.arange(2 * PAIRS)].all(), f"{what}: crash bytes go 0 -> 1 strictly inside the horizon"
                for g in (a, b):
                    g.tick_n(DT, 9, True, crash, REBOUNCE)
                assert_same_swarm(a, b, f"{what}: 9 ticks after the call")


def test_zero_gains_are_the_cost_tick_rollout_and_gains_change_the_state(mrs):
    """on the pair swarm, where all state is finite: G = 0 gives the cost and the state of rollout_tick_cost on the same commands bit for
    bit (0 * e = +-0 and c + +-0 = c for every finite c that is not -0.0: the nominal rows hold none), and the test's non-zero gains
    end in another state"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(273)
    ticks, hold, every = 48, 4, 2
    for crash, dtype, form in ((True, torch.float64, fb_forms(T)[0]), (False, torch.float32, fb_forms(T)[1])):
        a, b, c = (pair_swarm(mrs, mrs.ARITH_LITERAL) for _ in range(3))
        cost = cost_forms(T)[0]
        cmd, gains, refs, tg, wt = pair_inputs(T, rng, a, ticks // hold, dtype, form, cost, ticks // every)
        assert not (cmd == 0).any()
        want = T.rollout_tick_cost(a, O.POSITION_CMD, cmd, DT, crash, REBOUNCE, cost[0], tg, wt, cost[3], hold=hold, cost_every=every)
        zero = call(T, b, O.POSITION_CMD, cmd, crash, form[0], torch.zeros_like(gains), refs, cost, tg, wt, hold=hold, cost_every=every)
        assert_cost(zero, want.cpu().numpy(), f"G = 0, crash={crash}")
        assert_same_swarm(a, b, f"G = 0, crash={crash}")
        call(T, c, O.POSITION_CMD, cmd, crash, form[0], gains, refs, cost, tg, wt, hold=hold, cost_every=every)
        sa, sc = a.get_states(), c.get_states()
        assert np.isfinite(sc["x"]).all() and np.isfinite(sc["v"]).all()
        moved = (sa["x"] != sc["x"]).any(axis=1)
        print(f"crash={crash}: the gains moved {int(moved.sum())} of {N_PAIR} UAVs")
        assert moved.any(), f"crash={crash}: the feedback is in effect"
        assert np.asarray(c.has_crashed())[:2 * PAIRS].all() if crash else np.abs(c.get_external_force()[:2 * PAIRS]).sum() > 0


def test_stall_and_replay_inside_a_call(mrs):
    """launches queue behind a stalled one (the setup of test_rollout_tick_gpu): the replayed launches form the command from the state
    the no-ops left alone and add once, the no-ops write and add nothing"""
    import torch
    import mrs_multirotor_simulator_amd as M
    from mrs_multirotor_simulator_amd import tensors as T
    ticks, hold, every, n_fast = 48, 4, 2, 4
    a, b = (pair_swarm(mrs, mrs.ARITH_LITERAL, n_fast=n_fast) for _ in range(2))
    rng = np.random.default_rng(277)
    for g in (a, b):  # live lists: every tick of the call can be a fused launch
        g.tick_n(DT, 2, True, True, REBOUNCE)
    form, cost = fb_forms(T)[0], (T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, False, False, 1000.0)
    cmd, gains, refs, tg, wt = pair_inputs(T, rng, a, ticks // hold, torch.float64, form, cost, ticks // every)
    dev = cmd.device
    want, cr, _ = loop_cost(a, O.POSITION_CMD, cmd, form[0], gains, refs, cost, 0, hold, every, True, tg, wt)
    out = torch.full((N_PAIR,), SENTINEL, dtype=torch.float64, device=dev)
    fused0, stalls0, replayed0, _ = b.fused_stats()
    # the device is held back while the host queues its launches: the stall of the first one is seen when others are queued behind it
    assert M.load_library().mrs_debug_stream_delay(C.c_void_p(b.stream()), C.c_double(20000.0)) == 0
    got = call(T, b, O.POSITION_CMD, cmd, True, form[0], gains, refs, cost, tg, wt, hold=hold, cost_every=every, out=out)
    fused, stalls, replayed, _ = b.fused_stats()
    print(f"stall inside a call: {fused - fused0} fused launches, {stalls - stalls0} stalls, {replayed - replayed0} replayed")
    assert fused - fused0 >= 40 and stalls - stalls0 >= 1 and replayed - replayed0 >= 1, (fused - fused0, stalls - stalls0, replayed - replayed0)
    assert got.data_ptr() == out.data_ptr()
    c = got.cpu().numpy()
    assert not (c == SENTINEL).any() and (c >= 0).all(), "every element was overwritten (accumulate = 0: the sentinel is not added to)"
    assert_cost(c, want, "stall and replay: nothing added twice, nothing skipped")
    assert cr[-1, :2 * PAIRS].all()
    # the launch log is empty after the call: looking at the swarm replays nothing more and the vector stays as it is
    T.gather(b, cost[0], 0, N_PAIR, dtype=torch.float64)
    assert b.fused_stats()[1:3] == (stalls, replayed)
    assert_cost(out, want, "after looking at the swarm")
    assert_same_swarm(a, b, "after the call")


def test_unfused_paths(mrs, monkeypatch):
    """the ticks without the fused form (one step of the feedback rollout kernels, then the crash-add kernel) give the loop's bits, and
    those of a twin whose ticks are fused launches: the four cases of test_rollout_tick_gpu.test_unfused_paths"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ticks, hold, every = 48, 3, 6
    form = fb_forms(T)[1]  # OBS_ALL, shared gains and setpoints, one block
    full, alone = (T.OBS_ALL, False, False, 0.1), (0, None, None, 0.1)

    def run(make, what, crash, dirty=False, fused=None, cost=full):
        rng = np.random.default_rng(281)  # (the same inputs for every case: the twins are compared with each other)
        a, b = make(), make()
        for g in (a, b):
            g.tick_n(DT, 3, True, crash, REBOUNCE)
            if dirty:  # a host write of positions between two ticks: the pending collision tick is evaluated by a search of its own
                st = g.get_states()
                x = st["x"].copy()
                x[40:50, 1] += 0.125
                g.set_state(0, N_PAIR, x, st["v"], st["R"].reshape(N_PAIR, 9), st["omega"], st["motor_rpm"])
                g.handle_collisions(True, crash, REBOUNCE)
        cmd, gains, refs, tg, wt = pair_inputs(T, rng, pair_swarm(mrs, mrs.ARITH_LITERAL), ticks // hold, torch.float64, form, cost, ticks // every)
        fused0 = b.fused_stats()[0]
        want, cr, _ = loop_cost(a, O.POSITION_CMD, cmd, form[0], gains, refs, cost, 0, hold, every, crash, tg, wt)
        got = call(T, b, O.POSITION_CMD, cmd, crash, form[0], gains, refs, cost, tg, wt, hold=hold, cost_every=every)
        assert_cost(got, want, what)
        assert_same_swarm(a, b, what)
        n_fused = b.fused_stats()[0] - fused0
        if fused is not None:
            assert (n_fused > 0) == fused, f"{what}: {n_fused} fused launches"
        effect = cr[-1, :2 * PAIRS].all() if crash else np.abs(b.get_external_force()[:2 * PAIRS]).sum() > 0
        assert effect, f"{what}: the pairs met"
        return got.cpu().numpy()

    for crash in (True, False):
        run(lambda: pair_swarm(mrs, mrs.ARITH_LITERAL), f"dirty lists crash={crash}", crash, dirty=True, fused=True)
        run(lambda: pair_swarm(mrs, mrs.ARITH_LITERAL, dense=True), f"dense cluster crash={crash}", crash, fused=False)
    run(lambda: pair_swarm(mrs, mrs.ARITH_LITERAL, dense=True), "dense cluster, crash cost alone", True, fused=False, cost=alone)
    # the twins whose ticks are fused launches (the environment is read when a swarm is created)
    fused_crash = run(lambda: pair_swarm(mrs, mrs.ARITH_LITERAL), "fused twin crash", True, fused=True)
    fused_elastic = run(lambda: pair_swarm(mrs, mrs.ARITH_LITERAL), "fused twin elastic", False, fused=True)
    monkeypatch.setenv("MRS_FUSED_COLLISIONS", "0")
    got = run(lambda: pair_swarm(mrs, mrs.ARITH_LITERAL), "MRS_FUSED_COLLISIONS=0", True, fused=False)
    assert cost_equal(got, fused_crash), "MRS_FUSED_COLLISIONS=0: the bits of the fused twin"
    monkeypatch.delenv("MRS_FUSED_COLLISIONS")
    monkeypatch.setenv("MRS_NEIGHBOUR_LISTS", "0")
    got = run(lambda: pair_swarm(mrs, mrs.ARITH_LITERAL), "MRS_NEIGHBOUR_LISTS=0", False, fused=False)
    assert cost_equal(got, fused_elastic), "MRS_NEIGHBOUR_LISTS=0: the bits of the fused twin"


@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
def test_accumulate_and_cutting(mrs, arith):
    """one 24-tick call equals the same horizon cut at tick 12, a command-block boundary (the feedback is sampled at block starts, so a
    cut inside a block would be another law), the second half with accumulate; the pure closed-loop form is cut likewise and ends in the
    same state.  The pairs crash inside the horizon: the collision pass pending at the end of a call is charged by the next one.  FAST
    in crash mode only: one long call may search ahead where two short ones do not, and in elastic mode FAST bits depend on it
    (test_fast)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ar = getattr(mrs, "ARITH_" + arith)
    rng = np.random.default_rng(283)
    ticks, hold, cut = 24, 4, 12
    cost = (T.OBS_POS | T.OBS_VEL | T.OBS_ROT, False, False, 1000.0)
    w = T.gather_width(cost[0])
    cb = cut // hold
    for label, form in (("pair", fb_forms(T)[0]), ("variant", fb_forms(T)[3])):
        for crash in ((True, False) if arith == "LITERAL" else (True,)):
            if label == "pair":
                make, first, count, mode = (lambda: pair_swarm(mrs, ar)), 0, N_PAIR, O.POSITION_CMD
                cmd, gains, refs, _, _ = pair_inputs(T, rng, make(), ticks // hold, torch.float64, form, None, 0)
                dev = cmd.device
            else:
                make, first, count, mode = (lambda: variant_swarm(mrs, "cascade", ar)), FIRST, COUNT, O.ATTITUDE_RATE_CMD
                dev = torch_dev(make())
                cmd = torch.tensor(commands(mode, rng, ticks // hold, count, None), device=dev)
                gains, refs = draw(rng, mode, form, ticks // hold, count, torch.float64, dev)
            tg, wt = make_targets(rng, ticks, count, w, torch.float64, dev, False, False)
            one, split, pure, pure_split = make(), make(), make(), make()
            kw = dict(first=first, hold=hold, cost_every=1)
            what = f"{arith} {label} crash={crash}"
            got = call(T, one, mode, cmd, crash, form[0], gains, refs, cost, tg, wt, **kw).cpu().numpy()
            if label == "pair" and crash:
                assert np.asarray(one.has_crashed())[:2 * PAIRS].all() and (got[:2 * PAIRS] > 1000.0).all(), f"{what}: the pairs crashed and paid"
            g2 = gains[cb:] if gains.shape[0] > 1 else gains
            r2 = refs[cb:] if refs.shape[0] > 1 else refs
            acc = torch.full((count,), SENTINEL, dtype=torch.float64, device=dev)
            call(T, split, mode, cmd[:cb], crash, form[0], gains[:cb] if gains.shape[0] > 1 else gains, refs[:cb] if refs.shape[0] > 1 else refs, cost,
                 tg[:cut], wt[:cut], out=acc, **kw)
            call(T, split, mode, cmd[cb:], crash, form[0], g2, r2, cost, tg[cut:], wt[cut:], out=acc, accumulate=True, **kw)
            assert_cost(acc, got, f"{what}: one call vs two calls")
            assert_same_swarm(one, split, f"{what}: one call vs two calls")
            # without a cost: the same state, from one call and from two
            call(T, pure, mode, cmd, crash, form[0], gains, refs, None, None, None, **kw)
            assert_same_swarm(one, pure, f"{what}: the pure closed-loop run")
            call(T, pure_split, mode, cmd[:cb], crash, form[0], gains[:cb] if gains.shape[0] > 1 else gains, refs[:cb] if refs.shape[0] > 1 else refs, None,
                 None, None, **kw)
            call(T, pure_split, mode, cmd[cb:], crash, form[0], g2, r2, None, None, None, **kw)
            assert_same_swarm(one, pure_split, f"{what}: the pure closed-loop run in two calls")


def test_fast(mrs):
    """a FAST swarm against the FAST loop, bit for bit (cost and state): the law and the evaluation are uncontracted FP64 in both step
    units, and the loop's steps are FAST steps.

    What the cases are, and why.  In FAST the bits of a step depend on WHERE the force of the collision tick in front of it was
    evaluated: a fused launch consumes the force from its registers, and the FAST unit may contract the force's last operations into
    the step's; after a search ahead or a stall the force comes from a stand-alone pass through the F_FEXT columns.  Which of the two
    serves a tick depends on how far the host runs ahead of the device, for every call with collision ticks in it: on the variant
    swarm the 48-tick cost tick rollout (one search ahead) and ITS loop (none) differ in v for 7 UAVs in contact by 4e-16 relative,
    and so do this call and its loop; no arithmetic of this call is involved (LITERAL, where nothing is contracted, compares equal
    through every path: test_equals_the_loop, test_stall_and_replay_inside_a_call, test_unfused_paths).  So FAST is compared where
    the loop and the call provably take the same path:
    * crash mode, whole horizons: the evaluation sets crash flags and applies no force, whatever path evaluates it;
    * elastic mode, where the forces act: the horizon tick by tick (hold = cost_every = 1), 48 one-tick calls with accumulate against
      the loop.  Both wait for the device once per tick, in the same place relative to the step and the collision pass, so the host
      takes the same decision for every tick; the pairs meet and the forces act inside the horizon"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(293)
    FB, CF = fb_forms(T), cost_forms(T)

    def inputs(label, blocks, evals, dtype, form, cost):
        if label == "pair":
            a, b = pair_swarm(mrs, mrs.ARITH_FAST), pair_swarm(mrs, mrs.ARITH_FAST)
            return (a, b, 0, N_PAIR, O.POSITION_CMD) + pair_inputs(T, rng, a, blocks, dtype, form, cost, evals)
        a, b = variant_swarm(mrs, "cascade", mrs.ARITH_FAST), variant_swarm(mrs, "cascade", mrs.ARITH_FAST)
        mode, dev = O.ATTITUDE_RATE_CMD, torch_dev(a)
        cmd = torch.tensor(commands(mode, rng, blocks, COUNT, None), dtype=dtype, device=dev)
        gains, refs = draw(rng, mode, form, blocks, COUNT, dtype, dev)
        tg, wt = make_targets(rng, evals, COUNT, T.gather_width(cost[0]), dtype, dev, cost[1], cost[2])
        return a, b, FIRST, COUNT, mode, cmd, gains, refs, tg, wt

    for label in ("variant", "pair"):
        ticks, hold, every = 48, 4, 2
        for dtype, form, cost in ((torch.float64, FB[0], CF[0]), (torch.float32, FB[3], CF[3])):
            a, b, first, count, mode, cmd, gains, refs, tg, wt = inputs(label, ticks // hold, ticks // every, dtype, form, cost)
            want, cr, _ = loop_cost(a, mode, cmd, form[0], gains, refs, cost, first, hold, every, True, tg, wt)
            got = call(T, b, mode, cmd, True, form[0], gains, refs, cost, tg, wt, first=first, hold=hold, cost_every=every)
            what = f"FAST {label} crash mode {dtype} fb={form} cost={cost}"
            assert_cost(got, want, what)
            assert_same_swarm(a, b, what)
            assert cr.any(), what
        # elastic, tick by tick: one shared gain matrix and one setpoint block for the call, a target row per evaluation, one weight row
        dtype, form, cost = torch.float32, FB[1], CF[1]
        a, b, first, count, mode, cmd, gains, refs, tg, wt = inputs(label, ticks, ticks, dtype, form, cost)
        want, cr, _ = loop_cost(a, mode, cmd, form[0], gains, refs, cost, first, 1, 1, False, tg, wt)
        acc = torch.full((count,), SENTINEL, dtype=torch.float64, device=cmd.device)
        for t in range(ticks):
            call(T, b, mode, cmd[t:t + 1], False, form[0], gains, refs, cost, tg[t:t + 1], wt, first=first, out=acc, accumulate=t > 0)
        what = f"FAST {label} elastic, tick by tick"
        assert_cost(acc, want, what)
        assert_same_swarm(a, b, what)
        assert not cr.any() or label == "variant", what  # (the variant swarm's crashed UAVs crashed before the horizon)
        assert np.abs(a.get_external_force()).sum() > 0, f"{what}: forces act"


def test_held_crashed_and_outside(mrs):
    """UAV 0 (the partner of UAV 1) and the lone UAV 100 are on hold inside the range [0, 128): their commands are formed from their
    unchanged state and written, their terms are those of that state, UAV 1 still flies into UAV 0 and both pay the crash cost from then
    on; the UAVs outside the range own no element, keep their commands and go on exactly as under tick_n"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ticks, count, cc = 48, 128, 1000.0
    a, b, twin = (pair_swarm(mrs, mrs.ARITH_LITERAL) for _ in range(3))
    for g in (a, b, twin):
        g.set_hold(0, 1, True)
        g.set_hold(100, 1, True)
    dev = torch_dev(a)
    rng = np.random.default_rng(307)
    pos, _ = pair_state()
    form = (T.OBS_POS | T.OBS_VEL | T.OBS_OMEGA, True, True, False, True)
    cmd = torch.tensor(np.concatenate([pos[:count], np.zeros((count, 1))], axis=1)[None] + rng.normal(0, 0.01, (ticks, count, 4)), device=dev)
    fb_before = T.gather(b, form[0], 0, count, dtype=torch.float64).cpu().numpy()
    gains, refs = draw(rng, O.POSITION_CMD, form, ticks, count, torch.float64, dev, fb_before, n_cols=4)
    before = T.gather(b, T.OBS_ALL, 0, count, dtype=torch.float64).cpu().numpy()
    tg, wt = make_targets(rng, ticks, count, 36, torch.float64, dev, False, False, before)
    cost = (T.OBS_ALL, False, False, cc)
    want, cr, rows = loop_cost(a, O.POSITION_CMD, cmd, form[0], gains, refs, cost, 0, 1, 1, True, tg, wt)
    out_big = torch.full((N_PAIR,), SENTINEL, dtype=torch.float64, device=dev)
    got = call(T, b, O.POSITION_CMD, cmd, True, form[0], gains, refs, cost, tg, wt, out=out_big[:count]).cpu().numpy()
    assert_cost(got, want, "held UAVs in the range")
    assert_same_swarm(a, b, "held UAVs in the range")
    assert (out_big[count:].cpu().numpy() == SENTINEL).all(), "UAVs outside the range own no element"
    # the held UAVs: the terms of their unchanged state, and for UAV 0 the crash cost from the evaluation at which its byte first reads 1
    unchanged = np.broadcast_to(before[None], (ticks, count, 36))
    for k in (0, 100):
        assert all(same(rows[t, k], before[k]) for t in range(ticks)), f"held UAV {k}: the loop's rows are its unchanged state"
        assert cost_equal(got[k:k + 1], restate_ticks(unchanged[:, k:k + 1], cr[:, k:k + 1], tg.cpu().numpy()[:, k:k + 1], wt.cpu().numpy(), cc)), k
    assert cr[-1, 0] and cr[-1, 1] and not cr[0, :2].any() and not cr[:, 100].any(), "UAV 1 flew into the held UAV 0: both crashed inside the call"
    j0 = int(np.argmax(cr[:, 0]))
    assert 0 < j0 < ticks - 1 and got[0] > (ticks - j0) * cc * 0.999, "the held UAV crashed by a tick's evaluation pays from that evaluation on"
    assert cr[-1, 2:2 * PAIRS].all()
    # the command formed for a held UAV from its unchanged state sits in its command columns: released, the lone UAV 100 flies on it
    for g in (a, b):
        g.set_hold(100, 1, False)
        g.tick_n(DT, 5, True, True, REBOUNCE)
    assert_same_swarm(a, b, "after the release of a held UAV")
    u_last = restate_feedback(fb_before, cmd.cpu().numpy(), gains.cpu().numpy(), refs.cpu().numpy(), ticks - 1)[100]
    assert not same(u_last, cmd.cpu().numpy()[-1, 100]), "the held UAV's formed command is not its nominal row"
    # outside the range: as under tick_n
    twin.tick_n(DT, ticks, True, True, REBOUNCE)
    twin.set_hold(100, 1, False)
    twin.tick_n(DT, 5, True, True, REBOUNCE)
    sb, st = b.get_states(), twin.get_states()
    for f in ("x", "v", "omega", "motor_rpm"):
        assert same(sb[f][count:], st[f][count:]), f"outside the range: {f}"
    assert np.array_equal(b.has_crashed()[count:], twin.has_crashed()[count:])


def test_refused_calls_change_nothing(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL)
    dev = torch_dev(g)
    before = T.save(g).cpu().numpy()
    # 4 ticks, 2 command blocks x 100 UAVs x 10 FP64; POSITION_CMD: W_c = 4; fb_groups POS | VEL: W_o = 6; per-UAV gains, a block per command block
    hip, cmd = R._hip_malloc(2 * 100 * 10 * 8)
    _, gain = R._hip_malloc(2 * 4 * 6 * 100 * 8)
    _, gsmall = R._hip_malloc(2 * 4 * 6 * 100 * 8 - 8)
    _, ref = R._hip_malloc(2 * 100 * 6 * 8)
    _, rsmall = R._hip_malloc(2 * 100 * 6 * 8 - 8)
    _, tgt = R._hip_malloc(4 * 100 * 36 * 8)
    _, small = R._hip_malloc(4 * 100 * 36 * 8 - 8)
    _, wgt = R._hip_malloc(4 * 36 * 8)
    _, wsmall = R._hip_malloc(4 * 36 * 8 - 8)
    _, cost = R._hip_malloc(100 * 8)
    _, short = R._hip_malloc(100 * 8 - 8)
    host = np.zeros((4, 100, 36))
    fill = np.full(100, SENTINEL)
    assert hip.hipMemcpy(C.c_void_p(cost), fill.ctypes.data_as(C.c_void_p), fill.nbytes, 1) == 0
    for p, nbytes in ((gain, 2 * 4 * 6 * 100 * 8), (ref, 2 * 100 * 6 * 8)):  # (the accepted calls below read them)
        assert hip.hipMemset(C.c_void_p(p), 0, C.c_size_t(nbytes)) == 0
    fb = T.OBS_POS | T.OBS_VEL
    ok = dict(first=0, count=100, mode=O.POSITION_CMD, dt=DT, n_ticks=4, cmd_every=2, cost_every=1, dev_cmd=cmd, dtype=T.DTYPE_F64, cmd_stride=10,
              fb_groups=fb, dev_gain=gain, gain_per_uav=1, gain_blocks=2, dev_ref=ref, ref_stride=6, ref_blocks=2,
              cost_groups=T.OBS_ALL, dev_target=tgt, target_stride=36, dev_weight=wgt, weight_stride=36, crash_cost=1000.0, dev_cost=cost, accumulate=False,
              crash=True, rebounce=REBOUNCE, ext_stream=None)
    bad = [
        # the refusals of the tick rollout
        ({"first": N_SINGLE - 5}, 3), ({"count": -1}, 3), ({"mode": 11}, 1), ({"mode": -1}, 1), ({"dtype": 2}, 1), ({"n_ticks": 0}, 1),
        ({"dt": 0.0}, 1), ({"dt": -DT}, 1), ({"dt": float("nan")}, 1), ({"dt": float("inf")}, 1), ({"cmd_stride": 3}, 1), ({"cost_groups": 0x100}, 1),
        ({"dev_cmd": None}, 1), ({"dev_cmd": host.ctypes.data}, 1), ({"n_ticks": 5}, 1), ({"cmd_every": 0}, 1), ({"cmd_every": 3}, 1),
        ({"n_ticks": 6}, 1), ({"rebounce": float("nan")}, 1), ({"rebounce": float("inf")}, 1), ({"rebounce": float("-inf")}, 1),
        ({"mode": O.ACTUATOR_CMD, "cmd_stride": 4, "first": 1900}, 1),
        # those of the feedback rollout
        ({"mode": T.INPUT_UNKNOWN}, 1), ({"fb_groups": 0}, 1), ({"fb_groups": 0x100}, 1), ({"dev_gain": None}, 1),
        ({"dev_ref": None}, 1), ({"gain_per_uav": 2}, 1), ({"gain_per_uav": -1}, 1), ({"gain_blocks": 0}, 1), ({"gain_blocks": 4}, 1),
        ({"ref_blocks": 0}, 1), ({"ref_blocks": 3}, 1), ({"ref_stride": 5}, 1), ({"ref_stride": -1}, 1), ({"dev_gain": gsmall}, 1),
        ({"dev_gain": host.ctypes.data}, 1), ({"dev_ref": rsmall}, 1), ({"dev_ref": host.ctypes.data}, 1),
        # those of the cost tick rollout
        ({"cost_every": 0}, 1), ({"cost_every": -1}, 1), ({"cost_every": 3}, 1), ({"cost_every": 8}, 1), ({"dev_target": None}, 1),
        ({"dev_weight": None}, 1), ({"dev_cost": None}, 1), ({"dev_cost": short}, 1), ({"dev_cost": host.ctypes.data}, 1),
        ({"dev_target": small}, 1), ({"dev_target": host.ctypes.data}, 1), ({"dev_weight": wsmall}, 1), ({"dev_weight": host.ctypes.data}, 1),
        ({"target_stride": 35}, 1), ({"weight_stride": 35}, 1), ({"target_stride": -1}, 1),
        # cost_groups == 0 is refused only when a target or weight pointer comes with it; a bad cost_every is refused without a cost too
        ({"cost_groups": 0}, 1), ({"cost_groups": 0, "dev_weight": None}, 1), ({"cost_groups": 0, "dev_target": None}, 1),
        ({"cost_groups": 0, "dev_target": None, "dev_weight": None, "dev_cost": short}, 1),
        ({"cost_groups": 0, "dev_target": None, "dev_cost": None}, 1),
        ({"cost_groups": 0, "dev_target": None, "dev_weight": None, "dev_cost": None, "cost_every": 3}, 1),
    ]
    back = np.zeros(100)
    for change, code in bad:
        with pytest.raises(mrs.MrsError, match=f"error {code}:"):
            g.rollout_tick_feedback_device(**dict(ok, **change))
        assert np.array_equal(T.save(g).cpu().numpy(), before), change
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(cost), back.nbytes, 2) == 0
        assert (back == SENTINEL).all(), f"{change}: a refused call wrote dev_cost"
    with pytest.raises(ValueError):  # the tensor layer refuses before any library call
        T.rollout_tick_feedback(g, O.POSITION_CMD, torch.zeros((4, 100, 4), dtype=torch.float64), DT, True, REBOUNCE, fb, None, None)
    # the pure closed-loop run is accepted, ignores crash_cost and leaves the vector alone
    g.rollout_tick_feedback_device(**dict(ok, cost_groups=0, dev_target=None, dev_weight=None, dev_cost=None, crash_cost=float("nan")))
    torch.cuda.synchronize(dev)
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(cost), back.nbytes, 2) == 0
    assert (back == SENTINEL).all() and not np.array_equal(T.save(g).cpu().numpy(), before)
    # the unchanged arguments are accepted, and so are: shared rows and gains, one block, the crash cost alone, accumulation, non-finite
    # and negative crash costs
    g.rollout_tick_feedback_device(**ok)
    g.rollout_tick_feedback_device(**dict(ok, target_stride=0, weight_stride=0, ref_stride=0, gain_per_uav=0))
    g.rollout_tick_feedback_device(**dict(ok, gain_blocks=1, ref_blocks=1))
    g.rollout_tick_feedback_device(**dict(ok, cost_groups=0, dev_target=None, dev_weight=None, accumulate=True))
    g.rollout_tick_feedback_device(**dict(ok, crash_cost=float("inf")))
    g.rollout_tick_feedback_device(**dict(ok, crash_cost=-2.5, crash=False))
    torch.cuda.synchronize(dev)
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(cost), back.nbytes, 2) == 0
    assert not (back == SENTINEL).any()
    for p in (cmd, gain, gsmall, ref, rsmall, tgt, small, wgt, wsmall, cost, short):
        hip.hipFree(C.c_void_p(p))


def test_refused_on_a_sharded_swarm(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    group = mrs.LoopbackGroup(2)
    shards = []
    for r in range(2):
        g = mrs.Swarm(100)
        g.construct(0, 100, mrs.model_params("x500"), np.stack([np.arange(100) * 3.0 + 400 * r, np.zeros(100), np.full(100, 5.0)], axis=1))
        g.comm_init_loopback(group, r, 200)
        shards.append(g)
    dev = torch_dev(shards[0])
    cmd = torch.zeros((2, 100, 4), dtype=torch.float64, device=dev)
    gains = torch.zeros((1, 4, 3), dtype=torch.float64, device=dev)
    refs = torch.zeros((1, 1, 3), dtype=torch.float64, device=dev)
    tg = torch.zeros((2, 1, 3), dtype=torch.float64, device=dev)
    wt = torch.ones((1, 3), dtype=torch.float64, device=dev)
    out = torch.full((100,), SENTINEL, dtype=torch.float64, device=dev)
    for g in shards:
        x = g.get_states()["x"]
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.rollout_tick_feedback(g, O.POSITION_CMD, cmd, DT, True, REBOUNCE, T.OBS_POS, gains, refs, T.OBS_POS, tg, wt, 1000.0, out=out)
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.rollout_tick_feedback(g, O.POSITION_CMD, cmd, DT, True, REBOUNCE, T.OBS_POS, gains, refs)
        assert same(g.get_states()["x"], x)
    assert (out.cpu().numpy() == SENTINEL).all()
    for g in shards:
        g.close()
    group.close()


def test_caller_stream_is_fenced(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, b, c = (pair_swarm(mrs, mrs.ARITH_LITERAL) for _ in range(3))
    rng = np.random.default_rng(311)
    form, cost = fb_forms(T)[0], (T.OBS_ALL, False, False, 1000.0)
    src, gsrc, rsrc, tsrc, wsrc = pair_inputs(T, rng, a, 30, torch.float64, form, cost, 30)
    dev = src.device
    want = call(T, a, O.POSITION_CMD, src, True, form[0], gsrc, rsrc, cost, tsrc, wsrc).cpu().numpy()
    assert np.asarray(a.has_crashed())[:2 * PAIRS].all()
    for g, side in ((b, torch.cuda.Stream(dev)), (c, torch.cuda.ExternalStream(c.stream(), device=dev))):
        cmd, gains, refs, tg, wt = (torch.zeros_like(t) for t in (src, gsrc, rsrc, tsrc, wsrc))
        out = torch.full((N_PAIR,), SENTINEL, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
            for dst, s in ((cmd, src), (gains, gsrc), (refs, rsrc), (tg, tsrc), (wt, wsrc)):
                dst.copy_(s)  # written on the caller stream right before the call, no synchronisation
            call(T, g, O.POSITION_CMD, cmd, True, form[0], gains, refs, cost, tg, wt, out=out)
            copy = out.clone()  # torch work after the call sees the cost
        side.synchronize()
        assert cost_equal(copy.cpu().numpy(), want)
        assert_same_swarm(a, g, "fenced feedback tick rollout")


def child_main(out_path):
    """the pointer-addressed kernels (MRS_NO_BUFFER_ADDRESSING=1): fused ticks of the pair swarm with its mixed last block equal the
    loop in LITERAL, in both crash modes, and FAST equals the FAST loop"""
    import torch
    import mrs_multirotor_simulator_amd as M
    from mrs_multirotor_simulator_amd import tensors as T
    M.load_library()
    rng = np.random.default_rng(313)
    res = []
    for crash in (True, False):
        for arith, mixed, form in ((M.ARITH_LITERAL, True, fb_forms(T)[0]), (M.ARITH_FAST, False, fb_forms(T)[1])):
            a, b = pair_swarm(M, arith, mixed=mixed), pair_swarm(M, arith, mixed=mixed)
            cost = (T.OBS_ALL, False, False, 0.1)
            cmd, gains, refs, tg, wt = pair_inputs(T, rng, a, 12, torch.float32, form, cost, 24)
            want, cr, _ = loop_cost(a, O.POSITION_CMD, cmd, form[0], gains, refs, cost, 0, 4, 2, crash, tg, wt)
            got = call(T, b, O.POSITION_CMD, cmd, crash, form[0], gains, refs, cost, tg, wt, hold=4, cost_every=2)
            assert_cost(got, want, f"arith {arith} crash={crash}")
            assert_same_swarm(a, b, f"arith {arith} crash={crash}")
            assert b.fused_stats()[0] >= 47
            assert cr[-1, :2 * PAIRS].all() if crash else np.abs(b.get_external_force()[:2 * PAIRS]).sum() > 0
        res.append(str(crash))
    np.save(out_path, np.array(res))


def test_pointer_form(mrs, tmp_path):
    if _dead:
        pytest.fail(f"an earlier child process of this module died ({_dead[0]}): no further GPU process is started")
    out = str(tmp_path / "pointer.npy")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MRS_")}
    env["MRS_NO_BUFFER_ADDRESSING"] = "1"
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_rollout_tick_feedback_gpu as T; T.child_main({out!r})"
    try:
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _dead.append(f"pointer child timed out after {CHILD_TIMEOUT} s")
        pytest.fail(_dead[0])
    if p.returncode < 0:
        _dead.append(f"pointer child ended by signal {-p.returncode}")
        pytest.fail(f"{_dead[0]}\n{p.stderr[-3000:]}")
    assert p.returncode == 0, p.stderr[-3000:]
    assert list(np.load(out)) == ["True", "False"]


def test_cpp_facade_equals_python(mrs):
    if _dead:
        pytest.fail(f"an earlier child process of this module died ({_dead[0]}): no further GPU process is started")
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, B, hold, every, W, WO, WC = 1000, 6, 4, 2, 10, 6, 4
    E = B * hold // every
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rollout_tick_feedback.bin")
        try:
            out = subprocess.run([build_cpp("rollout_tick_feedback_test"), path], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            _dead.append(f"rollout_tick_feedback_test timed out after {CHILD_TIMEOUT} s")
            pytest.fail(_dead[0])
        if out.returncode < 0:
            _dead.append(f"rollout_tick_feedback_test ended by signal {-out.returncode}")
            pytest.fail(f"{_dead[0]}\n{out.stdout[-3000:]}")
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok cost_equals_the_loop", "ok crashed_uavs_pay", "ok state_equals_the_loop", "ok refused_call_changes_nothing",
                    "ok closed_loop_without_cost", "ok written"):
            assert tag in out.stdout, out.stdout
        cost = np.fromfile(path, np.float64)
    i = np.arange(n)
    pos = np.stack([4.0 * (i % 32), 4.0 * (i // 32), np.full(n, 5.0)], axis=1)
    odd = np.arange(1, 2 * PAIRS, 2)
    pos[odd] = np.stack([4.0 * (odd - 1) + 0.4, np.zeros(PAIRS), np.full(PAIRS, 5.0)], axis=1)
    g = mrs.Swarm(n, arith=mrs.ARITH_LITERAL)
    g.construct(0, n, mrs.default_params(), pos, 0.003 * i)
    dev = torch_dev(g)
    t = np.arange(B)[:, None]
    cmd = np.stack([np.broadcast_to(0.02 * np.sin(0.1 * t + 0.001 * i), (B, n)), np.broadcast_to(-0.01 + 0.0 * t + 0.0 * i, (B, n)),
                    np.broadcast_to(0.3 + 0.0001 * i + 0.0 * t, (B, n)), np.broadcast_to(0.55 + 0.005 * t + 0.0 * i, (B, n))], axis=2)
    gains = ((np.arange(WC)[:, None] + 1) * (np.arange(WO)[None, :] + 1) / 65536.0)[None]
    refs = (0.5 * np.arange(WO)[None, :] + 0.25 * np.arange(B)[:, None])[:, None, :]
    tg = (0.25 * np.arange(W)[None, :] + 0.125 * np.arange(E)[:, None])[:, None, :]
    wt = (0.5 + 0.0625 * np.arange(W))[None, :]
    mine = T.rollout_tick_feedback(g, O.ATTITUDE_RATE_CMD, torch.tensor(cmd, device=dev), DT, True, REBOUNCE, T.OBS_POS | T.OBS_VEL,
                                   torch.tensor(gains, device=dev), torch.tensor(refs, device=dev), T.OBS_POS | T.OBS_VEL | T.OBS_QUAT,
                                   torch.tensor(tg, device=dev), torch.tensor(wt, device=dev), 1000.0, hold=hold, cost_every=every)
    assert cost.shape == (n,) and cost_equal(cost, mine.cpu().numpy())
