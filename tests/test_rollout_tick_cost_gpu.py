"""Cost tick rollouts on the GPU (include/mrs_swarm.h, "cost tick rollouts"; tensors.rollout_tick_cost): a tick rollout that returns one
FP64 number per UAV, the weighted squared distance of its observation rows from target rows plus a crash cost at every evaluation at
which its crash flag is set, summed inside the fused step + collision kernels.

The reference is always a twin swarm driven through the loop the call stands for (test_rollout_tick_gpu.tick_loop: set_input / step /
gather + crashed / handle_collisions per tick, FP64 OBS rows and crash bytes; FP32 commands are widened, which is exact) and
`restate_ticks`, the restatement of the ABI comment in numpy: test_rollout_cost_gpu.restate evaluation by evaluation with the crash add
behind each term.  Every cost comparison is bit for bit (cost_equal: a NaN must be a NaN), and the two swarms must be in the same state
afterwards (assert_same_swarm).  All in LITERAL unless a test says FAST; FAST is compared with FAST rows, which needs no tolerance.

Sizes: the 256-UAV pair swarm of test_rollout_tick_gpu (four 64-UAV blocks, 16 head-on pairs that meet around tick 20) and the variant
swarm of test_rollout_gpu; horizons of at most 48 ticks.

The -0.0 cases: a term is never -0.0 (it starts from +0.0) and neither is a sum that had +0.0 added to it, so what can tell an
implementation that skips an add of zero from one that performs it is a vector that starts at -0.0 under accumulate: a zero weight row
makes every finite term +0.0 and the add must turn -0.0 into +0.0; with groups == 0 and crash_cost = 0.0 exactly the crashed UAVs turn.

ROLLOUT_TICK_COST_KERNELS maps every entry point of rollout_tick_cost_device.inc to the tests that force it (test_rollout_tick_cost.py
keeps the table complete)."""
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
from test_rollout_cost_gpu import cost_equal, restate
from test_rollout_gpu import COUNT, DT, FIRST, REBOUNCE, commands, same, variant_swarm
from test_rollout_tick_gpu import N_PAIR, PAIRS, assert_same_swarm, pair_state, pair_swarm, tick_loop
from test_step_variants_gpu import N_SINGLE

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 300
SENTINEL = -12345.678

# which tests force each entry point of rollout_tick_cost_device.inc (both flavours)
ROLLOUT_TICK_COST_KERNELS = {
    "mrs_uav_rollout_tick_cost_buf": ("test_equals_the_loop[crash]", "test_equals_the_loop[elastic]", "test_fast", "test_accumulate_and_cutting[FAST]"),
    "mrs_uav_model_rollout_tick_cost_buf": ("test_equals_the_loop[crash]", "test_equals_the_loop[elastic]"),
    "mrs_uav_rollout_tick_cost": ("test_pointer_form",),
    "mrs_uav_rollout_tick_cost_mixed": ("test_equals_the_loop[crash]", "test_equals_the_loop[elastic]", "test_pointer_form"),
}

_dead = []  # the first child process that died by a signal or timed out: nothing more is started on the GPU


def restate_ticks(rows, crashed, targets, weights, crash_cost, start=None):
    """the restatement of mrs_swarm_rollout_tick_cost_device: test_rollout_cost_gpu.restate evaluation by evaluation, and behind each
    term `c = c + crash_cost` where the crash byte is set.  rows [E, count, w] FP64 or None (groups == 0: no term is added), crashed
    [E, count], targets / weights as restate's or None (numpy arrays)"""
    cr = np.asarray(crashed).astype(bool)
    E, count = cr.shape
    c = np.zeros(count) if start is None else np.array(start, dtype=np.float64)
    cc = np.float64(crash_cost)
    with np.errstate(all="ignore"):
        for j in range(E):
            if rows is not None:
                wt = np.asarray(weights)
                c = restate(np.asarray(rows)[j:j + 1], np.asarray(targets)[j:j + 1], wt[j:j + 1] if wt.shape[0] > 1 else wt, c)
            c = np.where(cr[j], c + cc, c)
    return c


def assert_cost(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    if not cost_equal(got, want):
        bad = np.flatnonzero(~((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError(f"{what}: cost differs for {len(bad)} UAVs, first {bad[:6]}: got {got[bad[:6]]}, want {want[bad[:6]]}")


def make_targets(rng, E, count, w, dtype, dev, shared_targets, shared_weights, centre=None):
    """targets around `centre` ([count, w] or None: 0), positive weights with a heavier last row when there is a row per evaluation"""
    import torch
    tg = rng.normal(0.0, 2.0, (E, 1 if shared_targets else count, w))
    if centre is not None and not shared_targets:
        tg = tg + centre[None]
    wt = rng.uniform(0.1, 2.0, (1 if shared_weights else E, w))
    if not shared_weights:
        wt[-1] *= 10.0
    return torch.tensor(tg, dtype=dtype, device=dev), torch.tensor(wt, dtype=dtype, device=dev)


def loop_cost(g, mode, cmd, groups, first, hold, every, crash, tg, wt, crash_cost, start=None):
    """the loop on swarm g and the restatement: (cost, crash rows as numpy, FP64 rows as numpy or None)"""
    rows, cr = tick_loop(g, mode, cmd.double(), groups, first, hold, every, crash)
    rows = None if rows is None else rows.cpu().numpy()
    cr = cr.cpu().numpy()
    want = restate_ticks(rows, cr, None if tg is None else tg.cpu().numpy(), None if wt is None else wt.cpu().numpy(), crash_cost, start)
    return want, cr, rows


RATES = ((1, 1), (4, 2), (3, 6), (48, 48))  # (hold, cost_every)


def configs():
    """n_ticks in (1, 5, 48) with every pair of rates that divides it"""
    return [(t, h, e) for t in (1, 5, 48) for h, e in RATES if t % h == 0 and t % e == 0]


def forms(T):
    """(groups, shared targets, one weight row, crash_cost): per-UAV and shared targets, a weight row per evaluation and one row, the
    crash cost 1000.0 and 0.1, and the crash cost alone"""
    return ((T.OBS_ALL, False, False, 1000.0), (T.OBS_ALL, True, True, 0.1), (0, None, None, 1000.0),
            (T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, False, True, 0.1), (T.OBS_ALL, True, False, 1000.0))


@pytest.mark.parametrize("crash", [True, False], ids=["crash", "elastic"])
def test_equals_the_loop(mrs, crash):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(171)
    F = forms(T)
    run, seen = 0, set()
    # ---- variant swarm: every configuration, one after the other on the same two swarms; dtypes and forms take turns
    for scen, modes in (("cascade", (O.VELOCITY_HDG_CMD, O.ACTUATOR_CMD)), ("model", (O.ACTUATOR_CMD,))):
        a, b = variant_swarm(mrs, scen, mrs.ARITH_LITERAL), variant_swarm(mrs, scen, mrs.ARITH_LITERAL)
        assert np.asarray(a.has_crashed())[FIRST:].any() and np.asarray(a.has_crashed()).any(), "the scenario has crashed UAVs in the range"
        dev = torch_dev(a)
        for mode in modes:
            for ticks, hold, every in configs():
                dtype = (torch.float64, torch.float32)[run % 2]
                groups, sh_t, sh_w, cc = F[run % len(F)]
                seen.add((dtype, groups, sh_t, sh_w, cc))
                run += 1
                x = a.get_states(FIRST, COUNT)["x"]
                cmd = torch.tensor(commands(mode, rng, ticks // hold, COUNT, x), dtype=dtype, device=dev)
                E, w = ticks // every, T.gather_width(groups)
                tg, wt = make_targets(rng, E, COUNT, w, dtype, dev, sh_t, sh_w) if groups else (None, None)
                want, cr, _ = loop_cost(a, mode, cmd, groups, FIRST, hold, every, crash, tg, wt, cc)
                got = T.rollout_tick_cost(b, mode, cmd, DT, crash, REBOUNCE, groups, tg, wt, cc, first=FIRST, hold=hold, cost_every=every)
                what = f"variant {scen} {dtype} mode {mode} T={ticks} hold={hold} cost_every={every} groups={groups:#x} crash_cost={cc}"
                assert_cost(got, want, what)
                assert_same_swarm(a, b, what)
                assert cr.any(), f"{what}: crashed UAVs in the range pay"
        print(f"variant {scen} crash={crash}: fused_stats of the calls' swarm {b.fused_stats()}, of the loop's {a.fused_stats()}")
        for g in (a, b):
            g.tick_n(DT, 9, True, crash, REBOUNCE)
        assert_same_swarm(a, b, f"variant {scen}: 9 ticks after the calls")
        assert b.get_diag()["nan_rollback"] > 0
    assert len(seen) == 2 * len(F), "both dtypes met every form"
    # ---- pair swarm: fresh swarms per configuration (the pairs meet once), fused launches
    pos, _ = pair_state()
    for mixed in (False, True):
        for ticks, hold, every in (configs() if not mixed else [(48, 4, 2)]):
            dtype = torch.float32 if (ticks, hold, every) == (48, 4, 2) and not mixed else torch.float64
            groups, sh_t, sh_w, cc = F[run % len(F)] if (hold, every) != (1, 1) or ticks < 48 else F[0]
            run += 1
            a, b = pair_swarm(mrs, mrs.ARITH_LITERAL, mixed), pair_swarm(mrs, mrs.ARITH_LITERAL, mixed)
            dev = torch_dev(a)
            c = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (ticks // hold, N_PAIR, 4))
            cmd = torch.tensor(c, dtype=dtype, device=dev)
            E, w = ticks // every, T.gather_width(groups)
            centre = T.gather(a, groups, 0, N_PAIR, dtype=torch.float64).cpu().numpy() if groups else None
            tg, wt = make_targets(rng, E, N_PAIR, w, dtype, dev, sh_t, sh_w, centre) if groups else (None, None)
            fused0 = b.fused_stats()[0]
            want, cr, rows = loop_cost(a, O.POSITION_CMD, cmd, groups, 0, hold, every, crash, tg, wt, cc)
            got = T.rollout_tick_cost(b, O.POSITION_CMD, cmd, DT, crash, REBOUNCE, groups, tg, wt, cc, hold=hold, cost_every=every)
            what = f"pair mixed={mixed} {dtype} T={ticks} hold={hold} cost_every={every} groups={groups:#x} crash_cost={cc}"
            assert_cost(got, want, what)
            assert_same_swarm(a, b, what)
            assert b.fused_stats()[0] - fused0 >= ticks - 1, f"{what}: the ticks after the first are fused launches"
            if ticks == 48:
                if crash:
                    assert cr[-1, :2 * PAIRS].all() and not cr[:, 2 * PAIRS:].any(), what
                else:
                    assert not cr.any(), what
                if crash and (hold, every) == (1, 1):
                    # a pair UAV against a collision-free one: from the block in which the loop's crash byte first reads 1 the cost
                    # takes crash_cost per evaluation on top of the terms (the terms alone: restate without the crash add)
                    terms = restate(rows, tg.cpu().numpy(), wt.cpu().numpy())
                    extra = got.cpu().numpy() - terms
                    j0 = np.argmax(cr, axis=0)[:2 * PAIRS]
                    assert ((j0 > 0) & (j0 < E - 1)).all() and cr[j0, np.arange(2 * PAIRS)].all(), f"{what}: crash bytes go 0 -> 1 inside the call"
                    assert np.allclose(extra[:2 * PAIRS], (E - j0) * cc, rtol=1e-9, atol=0.0), f"{what}: {extra[:4]} vs {(E - j0[:4]) * cc}"
                    assert (extra[2 * PAIRS:] == 0.0).all(), f"{what}: a collision-free UAV pays its terms only"
                    # the crash cost alone on the same horizon: exactly (E - j0) additions of crash_cost, and nothing for the others
                    c2, d2 = pair_swarm(mrs, mrs.ARITH_LITERAL, mixed), pair_swarm(mrs, mrs.ARITH_LITERAL, mixed)
                    want2, cr2, _ = loop_cost(c2, O.POSITION_CMD, cmd, 0, 0, hold, every, crash, None, None, cc)
                    got2 = T.rollout_tick_cost(d2, O.POSITION_CMD, cmd, DT, crash, REBOUNCE, 0, None, None, cc, hold=hold, cost_every=every)
                    assert np.array_equal(cr2, cr)
                    assert_cost(got2, want2, f"{what}: crash cost alone")
                    assert np.array_equal(got2.cpu().numpy()[:2 * PAIRS], (E - j0) * cc) and not got2.cpu().numpy()[2 * PAIRS:].any()
                for g in (a, b):
                    g.tick_n(DT, 9, True, crash, REBOUNCE)
                assert_same_swarm(a, b, f"{what}: 9 ticks after the call")
    if crash:  # the -0.0 cases of the module docstring, on the pair swarm in crash mode
        for groups, label in ((T.OBS_POS | T.OBS_VEL, "zero weights"), (0, "crash cost alone")):
            a, b = pair_swarm(mrs, mrs.ARITH_LITERAL), pair_swarm(mrs, mrs.ARITH_LITERAL)
            dev = torch_dev(a)
            cmd = torch.tensor(np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (12, N_PAIR, 4)), device=dev)
            w = T.gather_width(groups)
            tg = torch.tensor(rng.normal(0.0, 2.0, (6, N_PAIR, w)), device=dev) if groups else None
            wt = torch.zeros((1, w), dtype=torch.float64, device=dev) if groups else None
            start = np.full(N_PAIR, -0.0)
            want, cr, _ = loop_cost(a, O.POSITION_CMD, cmd, groups, 0, 4, 8, True, tg, wt, 0.0, start)
            out = torch.tensor(start, device=dev)
            got = T.rollout_tick_cost(b, O.POSITION_CMD, cmd, DT, True, REBOUNCE, groups, tg, wt, 0.0, hold=4, cost_every=8, out=out, accumulate=True)
            assert_cost(got, want, f"-0.0, {label}")
            sign = np.signbit(got.cpu().numpy())
            assert cr[-1, :2 * PAIRS].all() and not sign[:2 * PAIRS].any(), f"-0.0, {label}: the crash add of 0.0 was performed"
            assert sign[2 * PAIRS:].all() == (groups == 0) and sign[2 * PAIRS:].any() == (groups == 0), f"-0.0, {label}"


def test_stall_and_replay_inside_a_call(mrs):
    """launches queue behind a stalled one (the setup of test_rollout_tick_gpu): the replayed launches add once, the no-ops nothing"""
    import torch
    import mrs_multirotor_simulator_amd as M
    from mrs_multirotor_simulator_amd import tensors as T
    ticks, hold, every, n_fast = 48, 4, 2, 4
    a, b = (pair_swarm(mrs, mrs.ARITH_LITERAL, n_fast=n_fast) for _ in range(2))
    dev = torch_dev(a)
    rng = np.random.default_rng(173)
    pos, _ = pair_state()
    cmd = torch.tensor(np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (ticks // hold, N_PAIR, 4)), device=dev)
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_QUAT
    for g in (a, b):  # live lists: every tick of the call can be a fused launch
        g.tick_n(DT, 2, True, True, REBOUNCE)
    centre = T.gather(a, groups, 0, N_PAIR, dtype=torch.float64).cpu().numpy()
    tg, wt = make_targets(rng, ticks // every, N_PAIR, T.gather_width(groups), torch.float64, dev, False, False, centre)
    want, cr, _ = loop_cost(a, O.POSITION_CMD, cmd, groups, 0, hold, every, True, tg, wt, 1000.0)
    out = torch.full((N_PAIR,), SENTINEL, dtype=torch.float64, device=dev)
    fused0, stalls0, replayed0, _ = b.fused_stats()
    # the device is held back while the host queues its launches: the stall of the first one is seen when others are queued behind it
    assert M.load_library().mrs_debug_stream_delay(C.c_void_p(b.stream()), C.c_double(20000.0)) == 0
    got = T.rollout_tick_cost(b, O.POSITION_CMD, cmd, DT, True, REBOUNCE, groups, tg, wt, 1000.0, hold=hold, cost_every=every, out=out)
    fused, stalls, replayed, _ = b.fused_stats()
    print(f"stall inside a call: {fused - fused0} fused launches, {stalls - stalls0} stalls, {replayed - replayed0} replayed")
    assert fused - fused0 >= 40 and stalls - stalls0 >= 1 and replayed - replayed0 >= 1, (fused - fused0, stalls - stalls0, replayed - replayed0)
    assert got.data_ptr() == out.data_ptr()
    c = got.cpu().numpy()
    assert not (c == SENTINEL).any() and (c >= 0).all(), "every element was overwritten (accumulate = 0: the sentinel is not added to)"
    assert_cost(c, want, "stall and replay: nothing added twice, nothing skipped")
    assert cr[-1, :2 * PAIRS].all()
    # the launch log is empty after the call: looking at the swarm replays nothing more and the vector stays as it is
    T.gather(b, groups, 0, N_PAIR, dtype=torch.float64)
    assert b.fused_stats()[1:3] == (stalls, replayed)
    assert_cost(out, want, "after looking at the swarm")
    assert_same_swarm(a, b, "after the call")


def test_unfused_paths(mrs, monkeypatch):
    """the ticks without the fused form (one step of the cost rollout kernels, then the crash-add kernel) give the loop's bits, and those
    of a twin whose ticks are fused launches: the four cases of test_rollout_tick_gpu.test_unfused_paths"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(179)
    ticks, hold, every = 48, 3, 6
    pos, v = pair_state()
    c = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (ticks // hold, N_PAIR, 4))
    tgn = rng.normal(0.0, 2.0, (ticks // every, N_PAIR, 36))
    wtn = rng.uniform(0.1, 2.0, (ticks // every, 36))
    cc = 0.1

    def run(make, what, crash, dirty=False, fused=None, groups=None):
        groups = T.OBS_ALL if groups is None else groups
        a, b = make(), make()
        dev = torch_dev(a)
        cmd = torch.tensor(c, device=dev)
        for g in (a, b):
            g.tick_n(DT, 3, True, crash, REBOUNCE)
            if dirty:  # a host write of positions between two ticks: the pending collision tick is evaluated by a search of its own
                st = g.get_states()
                x = st["x"].copy()
                x[40:50, 1] += 0.125
                g.set_state(0, N_PAIR, x, st["v"], st["R"].reshape(N_PAIR, 9), st["omega"], st["motor_rpm"])
                g.handle_collisions(True, crash, REBOUNCE)
        tg = torch.tensor(tgn, device=dev) if groups else None
        wt = torch.tensor(wtn, device=dev) if groups else None
        fused0 = b.fused_stats()[0]
        want, cr, _ = loop_cost(a, O.POSITION_CMD, cmd, groups, 0, hold, every, crash, tg, wt, cc)
        got = T.rollout_tick_cost(b, O.POSITION_CMD, cmd, DT, crash, REBOUNCE, groups, tg, wt, cc, hold=hold, cost_every=every)
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
    run(lambda: pair_swarm(mrs, mrs.ARITH_LITERAL, dense=True), "dense cluster, crash cost alone", True, fused=False, groups=0)
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
    """one 24-tick call equals 24 one-tick calls with accumulate, and two calls cut at tick 10, inside a held command block; the pairs
    crash inside the horizon (the collision pass pending at the end of a call is charged by the next one)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ar = getattr(mrs, "ARITH_" + arith)
    rng = np.random.default_rng(181)
    ticks, hold, cut = 24, 4, 10  # the cut at tick 10 falls inside command block 2 (ticks 8-11)
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_ROT
    w = T.gather_width(groups)
    for make, first, count, label in ((lambda: variant_swarm(mrs, "cascade", ar), FIRST, COUNT, "variant"), (lambda: pair_swarm(mrs, ar), 0, N_PAIR, "pair")):
        for crash in (True, False):
            one, single, split = make(), make(), make()
            dev = torch_dev(one)
            if label == "pair":  # head-on pairs that meet at tick 20 under their position commands
                pos, _ = pair_state()
                blocks = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (ticks // hold, N_PAIR, 4))
                mode = O.POSITION_CMD
            else:
                mode = O.ATTITUDE_RATE_CMD
                blocks = commands(mode, rng, ticks // hold, count, None)
            per_tick = torch.tensor(np.repeat(blocks, hold, axis=0), device=dev)  # command row of every tick
            cmd = torch.tensor(blocks, device=dev)
            tg, wt = make_targets(rng, ticks, count, w, torch.float64, dev, False, False)
            kw = dict(first=first, cost_every=1)
            what = f"{arith} {label} crash={crash}"
            got = T.rollout_tick_cost(one, mode, cmd, DT, crash, REBOUNCE, groups, tg, wt, 1000.0, hold=hold, **kw).cpu().numpy()
            if label == "pair" and crash:
                assert np.asarray(one.has_crashed())[:2 * PAIRS].all() and (got[:2 * PAIRS] > 1000.0).all(), f"{what}: the pairs crashed and paid"
            acc = torch.full((count,), SENTINEL, dtype=torch.float64, device=dev)
            for t in range(ticks):  # 24 calls of one tick; the first overwrites the sentinel
                T.rollout_tick_cost(single, mode, per_tick[t:t + 1], DT, crash, REBOUNCE, groups, tg[t:t + 1], wt[t:t + 1], 1000.0, out=acc,
                                    accumulate=t > 0, **kw)
            assert_cost(acc, got, f"{what}: one call vs single-tick calls")
            assert_same_swarm(one, single, f"{what}: one call vs single-tick calls")
            acc2 = torch.full((count,), SENTINEL, dtype=torch.float64, device=dev)
            T.rollout_tick_cost(split, mode, per_tick[:cut:2].contiguous(), DT, crash, REBOUNCE, groups, tg[:cut], wt[:cut], 1000.0, hold=2, out=acc2, **kw)
            T.rollout_tick_cost(split, mode, per_tick[cut::2].contiguous(), DT, crash, REBOUNCE, groups, tg[cut:], wt[cut:], 1000.0, hold=2, out=acc2,
                                accumulate=True, **kw)
            assert_cost(acc2, got, f"{what}: one call vs two calls")
            assert_same_swarm(one, split, f"{what}: one call vs two calls")


def test_fast(mrs):
    """one call on a FAST swarm equals the restatement over the FP64 rows and crash bytes that rollout_ticks writes on a FAST twin, bit
    for bit, and leaves the same state (how close FAST rows are to the loop: test_rollout_tick_gpu.test_fast)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(183)
    ticks, hold, every = 48, 4, 2
    pos, _ = pair_state()
    for make, first, count, mode, label in (
            (lambda: variant_swarm(mrs, "cascade", mrs.ARITH_FAST), FIRST, COUNT, O.ATTITUDE_RATE_CMD, "variant"),
            (lambda: pair_swarm(mrs, mrs.ARITH_FAST), 0, N_PAIR, O.POSITION_CMD, "pair")):
        for crash, dtype, (groups, sh_t, sh_w, cc) in ((True, torch.float64, forms(T)[0]), (False, torch.float32, forms(T)[1]), (True, torch.float32, forms(T)[3])):
            a, b = make(), make()
            dev = torch_dev(a)
            if label == "pair":
                blocks = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (ticks // hold, N_PAIR, 4))
            else:
                blocks = commands(mode, rng, ticks // hold, count, None)
            cmd = torch.tensor(blocks, dtype=dtype, device=dev)
            tg, wt = make_targets(rng, ticks // every, count, T.gather_width(groups), dtype, dev, sh_t, sh_w)
            rows, cr = T.rollout_ticks(a, mode, cmd.double(), DT, crash, REBOUNCE, groups, first=first, hold=hold, obs_every=every)
            want = restate_ticks(rows.cpu().numpy(), cr.cpu().numpy(), tg.cpu().numpy(), wt.cpu().numpy(), cc)
            got = T.rollout_tick_cost(b, mode, cmd, DT, crash, REBOUNCE, groups, tg, wt, cc, first=first, hold=hold, cost_every=every)
            what = f"FAST {label} crash={crash} {dtype} groups={groups:#x}"
            assert_cost(got, want, what)
            assert_same_swarm(a, b, what)
            assert cr.cpu().numpy().any() or not crash, what


def test_held_crashed_and_outside(mrs):
    """UAV 0 (the partner of UAV 1) and the lone UAV 100 are on hold inside the range [0, 128): their terms are those of their unchanged
    state, UAV 1 still flies into UAV 0 and both pay the crash cost from then on; the UAVs outside the range own no element and go on
    exactly as under tick_n"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ticks, count, cc = 48, 128, 1000.0
    a, b, twin = (pair_swarm(mrs, mrs.ARITH_LITERAL) for _ in range(3))
    for g in (a, b, twin):
        g.set_hold(0, 1, True)
        g.set_hold(100, 1, True)
    dev = torch_dev(a)
    rng = np.random.default_rng(189)
    pos, _ = pair_state()
    c = np.concatenate([pos[:count], np.zeros((count, 1))], axis=1)[None] + rng.normal(0, 0.01, (ticks, count, 4))
    cmd = torch.tensor(c, device=dev)
    before = T.gather(b, T.OBS_ALL, 0, count, dtype=torch.float64).cpu().numpy()
    tg, wt = make_targets(rng, ticks, count, 36, torch.float64, dev, False, False, before)
    want, cr, rows = loop_cost(a, O.POSITION_CMD, cmd, T.OBS_ALL, 0, 1, 1, True, tg, wt, cc)
    out_big = torch.full((N_PAIR,), SENTINEL, dtype=torch.float64, device=dev)
    got = T.rollout_tick_cost(b, O.POSITION_CMD, cmd, DT, True, REBOUNCE, T.OBS_ALL, tg, wt, cc, out=out_big[:count]).cpu().numpy()
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
    terms = restate(unchanged[:, :1], tg.cpu().numpy()[:, :1], wt.cpu().numpy())
    assert np.isclose(got[0] - terms[0], (ticks - j0) * cc, rtol=1e-9, atol=0.0) and 0 < j0 < ticks - 1
    assert cr[-1, 2:2 * PAIRS].all()
    # outside the range: as under tick_n
    twin.tick_n(DT, ticks, True, True, REBOUNCE)
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
    hip, cmd = R._hip_malloc(2 * 100 * 10 * 8)  # 4 ticks, 2 command blocks x 100 UAVs x 10 FP64
    _, tgt = R._hip_malloc(4 * 100 * 36 * 8)
    _, small = R._hip_malloc(4 * 100 * 36 * 8 - 8)
    _, wgt = R._hip_malloc(4 * 36 * 8)
    _, wsmall = R._hip_malloc(4 * 36 * 8 - 8)
    _, cost = R._hip_malloc(100 * 8)
    _, short = R._hip_malloc(100 * 8 - 8)
    host = np.zeros((4, 100, 36))
    fill = np.full(100, SENTINEL)
    assert hip.hipMemcpy(C.c_void_p(cost), fill.ctypes.data_as(C.c_void_p), fill.nbytes, 1) == 0
    ok = dict(first=0, count=100, mode=O.POSITION_CMD, dt=DT, n_ticks=4, cmd_every=2, cost_every=1, dev_cmd=cmd, dtype=T.DTYPE_F64, cmd_stride=10,
              groups=T.OBS_ALL, dev_target=tgt, target_stride=36, dev_weight=wgt, weight_stride=36, crash_cost=1000.0, dev_cost=cost, accumulate=False,
              crash=True, rebounce=REBOUNCE, ext_stream=None)
    bad = [
        # the refusals of the tick rollout
        ({"first": N_SINGLE - 5}, 3), ({"count": -1}, 3), ({"mode": 11}, 1), ({"mode": -1}, 1), ({"dtype": 2}, 1), ({"n_ticks": 0}, 1),
        ({"dt": 0.0}, 1), ({"dt": -DT}, 1), ({"dt": float("nan")}, 1), ({"dt": float("inf")}, 1), ({"cmd_stride": 3}, 1), ({"groups": 0x100}, 1),
        ({"dev_cmd": None}, 1), ({"dev_cmd": host.ctypes.data}, 1), ({"n_ticks": 5}, 1), ({"cmd_every": 0}, 1), ({"cmd_every": 3}, 1),
        ({"n_ticks": 6}, 1), ({"rebounce": float("nan")}, 1), ({"rebounce": float("inf")}, 1), ({"rebounce": float("-inf")}, 1),
        ({"mode": O.ACTUATOR_CMD, "cmd_stride": 4, "first": 1900}, 1),
        # those of the cost rollout
        ({"cost_every": 0}, 1), ({"cost_every": -1}, 1), ({"cost_every": 3}, 1), ({"cost_every": 8}, 1), ({"dev_target": None}, 1),
        ({"dev_weight": None}, 1), ({"dev_cost": None}, 1), ({"dev_cost": short}, 1), ({"dev_cost": host.ctypes.data}, 1),
        ({"dev_target": small}, 1), ({"dev_target": host.ctypes.data}, 1), ({"dev_weight": wsmall}, 1), ({"dev_weight": host.ctypes.data}, 1),
        ({"target_stride": 35}, 1), ({"weight_stride": 35}, 1), ({"target_stride": -1}, 1),
        # groups == 0 is refused only when a target or weight pointer comes with it
        ({"groups": 0}, 1), ({"groups": 0, "dev_weight": None}, 1), ({"groups": 0, "dev_target": None}, 1),
        ({"groups": 0, "dev_target": None, "dev_weight": None, "dev_cost": None}, 1),
        ({"groups": 0, "dev_target": None, "dev_weight": None, "dev_cost": short}, 1),
    ]
    back = np.zeros(100)
    for change, code in bad:
        with pytest.raises(mrs.MrsError, match=f"error {code}:"):
            g.rollout_tick_cost_device(**dict(ok, **change))
        assert np.array_equal(T.save(g).cpu().numpy(), before), change
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(cost), back.nbytes, 2) == 0
        assert (back == SENTINEL).all(), f"{change}: a refused call wrote dev_cost"
    with pytest.raises(ValueError):  # the tensor layer refuses before any library call
        T.rollout_tick_cost(g, O.POSITION_CMD, torch.zeros((4, 100, 4), dtype=torch.float64), DT, True, REBOUNCE, 0, None, None)
    # the unchanged arguments are accepted, and so are: shared rows, the crash cost alone, accumulation, non-finite and negative crash costs
    g.rollout_tick_cost_device(**ok)
    g.rollout_tick_cost_device(**dict(ok, target_stride=0, weight_stride=0))
    g.rollout_tick_cost_device(**dict(ok, groups=0, dev_target=None, dev_weight=None, accumulate=True))
    g.rollout_tick_cost_device(**dict(ok, crash_cost=float("inf")))
    g.rollout_tick_cost_device(**dict(ok, crash_cost=-2.5, crash=False))
    torch.cuda.synchronize(dev)
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(cost), back.nbytes, 2) == 0
    assert not (back == SENTINEL).any() and not np.array_equal(T.save(g).cpu().numpy(), before)
    for p in (cmd, tgt, small, wgt, wsmall, cost, short):
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
    tg = torch.zeros((2, 1, 3), dtype=torch.float64, device=dev)
    wt = torch.ones((1, 3), dtype=torch.float64, device=dev)
    out = torch.full((100,), SENTINEL, dtype=torch.float64, device=dev)
    for g in shards:
        x = g.get_states()["x"]
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.rollout_tick_cost(g, O.POSITION_CMD, cmd, DT, True, REBOUNCE, T.OBS_POS, tg, wt, 1000.0, out=out)
        assert same(g.get_states()["x"], x)
    assert (out.cpu().numpy() == SENTINEL).all()
    for g in shards:
        g.close()
    group.close()


def test_caller_stream_is_fenced(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, b, c = (pair_swarm(mrs, mrs.ARITH_LITERAL) for _ in range(3))
    dev = torch_dev(a)
    rng = np.random.default_rng(197)
    pos, _ = pair_state()
    src = torch.tensor(np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (30, N_PAIR, 4)), device=dev)
    tsrc, wsrc = make_targets(rng, 30, N_PAIR, 36, torch.float64, dev, False, False)
    want = T.rollout_tick_cost(a, O.POSITION_CMD, src, DT, True, REBOUNCE, T.OBS_ALL, tsrc, wsrc, 1000.0).cpu().numpy()
    assert np.asarray(a.has_crashed())[:2 * PAIRS].all()
    for g, side in ((b, torch.cuda.Stream(dev)), (c, torch.cuda.ExternalStream(c.stream(), device=dev))):
        cmd, tg, wt = torch.zeros_like(src), torch.zeros_like(tsrc), torch.zeros_like(wsrc)
        out = torch.full((N_PAIR,), SENTINEL, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
            cmd.copy_(src)  # written on the caller stream right before the call, no synchronisation
            tg.copy_(tsrc)
            wt.copy_(wsrc)
            T.rollout_tick_cost(g, O.POSITION_CMD, cmd, DT, True, REBOUNCE, T.OBS_ALL, tg, wt, 1000.0, out=out)
            copy = out.clone()  # torch work after the call sees the cost
        side.synchronize()
        assert cost_equal(copy.cpu().numpy(), want)
        assert_same_swarm(a, g, "fenced cost tick rollout")


def child_main(out_path):
    """the pointer-addressed kernels (MRS_NO_BUFFER_ADDRESSING=1): fused ticks of the pair swarm with its mixed last block equal the
    loop in LITERAL, in both crash modes, and FAST equals itself cut into single ticks"""
    import torch
    import mrs_multirotor_simulator_amd as M
    from mrs_multirotor_simulator_amd import tensors as T
    M.load_library()
    rng = np.random.default_rng(201)
    pos, _ = pair_state()
    res = []
    for crash in (True, False):
        a, b = pair_swarm(M, M.ARITH_LITERAL, mixed=True), pair_swarm(M, M.ARITH_LITERAL, mixed=True)
        dev = torch_dev(a)
        c = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (12, N_PAIR, 4))
        cmd = torch.tensor(c, dtype=torch.float32, device=dev)
        tg, wt = make_targets(rng, 24, N_PAIR, 36, torch.float32, dev, False, False)
        want, cr, _ = loop_cost(a, O.POSITION_CMD, cmd, T.OBS_ALL, 0, 4, 2, crash, tg, wt, 0.1)
        got = T.rollout_tick_cost(b, O.POSITION_CMD, cmd, DT, crash, REBOUNCE, T.OBS_ALL, tg, wt, 0.1, hold=4, cost_every=2)
        assert_cost(got, want, f"LITERAL crash={crash}")
        assert_same_swarm(a, b, f"LITERAL crash={crash}")
        assert b.fused_stats()[0] >= 47
        assert cr[-1, :2 * PAIRS].all() if crash else np.abs(b.get_external_force()[:2 * PAIRS]).sum() > 0
        f1, f2 = pair_swarm(M, M.ARITH_FAST), pair_swarm(M, M.ARITH_FAST)
        one = T.rollout_tick_cost(f1, O.POSITION_CMD, cmd[:6], DT, crash, REBOUNCE, T.OBS_ALL, tg[:6], wt[:6], 0.1, cost_every=1)
        acc = torch.zeros(N_PAIR, dtype=torch.float64, device=dev)
        for t in range(6):
            T.rollout_tick_cost(f2, O.POSITION_CMD, cmd[t:t + 1], DT, crash, REBOUNCE, T.OBS_ALL, tg[t:t + 1], wt[t:t + 1], 0.1, out=acc, accumulate=True)
        assert_cost(acc, one.cpu().numpy(), f"FAST crash={crash}")
        res.append(str(crash))
    np.save(out_path, np.array(res))


def test_pointer_form(mrs, tmp_path):
    if _dead:
        pytest.fail(f"an earlier child process of this module died ({_dead[0]}): no further GPU process is started")
    out = str(tmp_path / "pointer.npy")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MRS_")}
    env["MRS_NO_BUFFER_ADDRESSING"] = "1"
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_rollout_tick_cost_gpu as T; T.child_main({out!r})"
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
    n, B, hold, every, W = 1000, 6, 4, 2, 10
    E = B * hold // every
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rollout_tick_cost.bin")
        try:
            out = subprocess.run([build_cpp("rollout_tick_cost_test"), path], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            _dead.append(f"rollout_tick_cost_test timed out after {CHILD_TIMEOUT} s")
            pytest.fail(_dead[0])
        if out.returncode < 0:
            _dead.append(f"rollout_tick_cost_test ended by signal {-out.returncode}")
            pytest.fail(f"{_dead[0]}\n{out.stdout[-3000:]}")
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok cost_equals_the_loop", "ok crashed_uavs_pay", "ok state_equals_the_loop", "ok refused_call_changes_nothing",
                    "ok crash_only_accumulates", "ok written"):
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
    tg = (0.25 * np.arange(W)[None, :] + 0.125 * np.arange(E)[:, None])[:, None, :]
    wt = (0.5 + 0.0625 * np.arange(W))[None, :]
    mine = T.rollout_tick_cost(g, O.ATTITUDE_RATE_CMD, torch.tensor(cmd, device=dev), DT, True, REBOUNCE, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT,
                               torch.tensor(tg, device=dev), torch.tensor(wt, device=dev), 1000.0, hold=hold, cost_every=every)
    assert cost.shape == (n,) and cost_equal(cost, mine.cpu().numpy())
