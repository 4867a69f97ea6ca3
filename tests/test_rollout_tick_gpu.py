"""Tick rollouts on the GPU (include/mrs_swarm.h, "tick rollouts"; mrs_multirotor_simulator_amd.tensors.rollout_ticks): in LITERAL one
call over T ticks equals the loop it stands for — set_input / step / gather + crashed / handle_collisions per tick — bit for bit: every
observation row, every crash byte, and afterwards the state, PID, IMU, external force, crash flags and diag counters, also after 9 more
tick_n ticks on both.  Two swarms: the variant-test swarm of test_rollout_gpu (three airframes, mixed blocks, ragged tail, held, crashed
and NaN-rollback UAVs, contacts already present; whichever path its dense neighbourhoods let a tick take) and the pair swarm below,
whose ticks after the first are fused launches (asserted).  Stalls and replays inside a call write into the caller's rows;
the paths without the fused form give the same rows; FAST is bit-identical to itself in any split of the call and close to the loop.

ROLLOUT_TICK_KERNELS maps every entry point of rollout_tick_device.inc to the test that forces it (test_rollout_tick.py keeps the table
complete)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import helpers
import test_rollout_gpu as R
from helpers import RTOL_FAST
from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_rollout_gpu import COUNT, DT, FIRST, REBOUNCE, assert_same_state, commands, same, variant_swarm
from test_step_variants_gpu import N_SINGLE

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 300

# which test forces each entry point of rollout_tick_device.inc (both flavours)
ROLLOUT_TICK_KERNELS = {
    "mrs_uav_rollout_tick_buf": ("test_literal_equals_the_loop[crash]", "test_literal_equals_the_loop[elastic]", "test_fast"),
    "mrs_uav_model_rollout_tick_buf": ("test_literal_equals_the_loop[crash]", "test_literal_equals_the_loop[elastic]"),
    "mrs_uav_rollout_tick": ("test_pointer_form",),
    "mrs_uav_rollout_tick_mixed": ("test_literal_equals_the_loop[crash]", "test_literal_equals_the_loop[elastic]"),
}

_dead = []  # the first child process that died by a signal or timed out: nothing more is started on the GPU

N_PAIR = 256
PAIRS = 16


def pair_state(n=N_PAIR, n_fast=0):
    """n UAVs 10 m apart on a line at z = 5 m; the first 16 pairs (2k, 2k + 1) 1.5 m apart, flying at each other at 15 m/s each.  On the
    CPU oracle (dt 1 ms, rebounce 100) the first crash / the first non-zero external force comes with the collision pass of tick 20,
    for all 32 UAVs.  n_fast lone UAVs at the end of the line fly at 300 m/s: 0.3 m per tick, more than half the skin of the
    neighbour lists, so they leave it within one step, before any warning."""
    pos = np.stack([10.0 * np.arange(n), np.zeros(n), np.full(n, 5.0)], axis=1)
    v = np.zeros((n, 3))
    for k in range(PAIRS):
        pos[2 * k + 1, 0] = pos[2 * k, 0] + 1.5
        v[2 * k, 0], v[2 * k + 1, 0] = 15.0, -15.0
    if n_fast:
        v[n - n_fast:, 1] = 300.0
    return pos, v


def pair_swarm(mrs, arith, mixed=False, n_fast=0, dense=False):
    """the pair swarm under POSITION_CMD to its own positions.  mixed: the last 64-UAV block alternates x500 and f550 in runs of 5 (a
    mixed-airframe block).  dense: the last 100 UAVs stand in a 5 x 5 x 4 grid 1 m apart instead — more neighbours within the list
    radius than a list holds, so no tick of the swarm can take the fused form."""
    pos, v = pair_state(n_fast=n_fast)
    n = len(pos)
    if dense:
        k = np.arange(100)
        pos[n - 100:] = np.stack([3000.0 + 1.0 * (k % 5), 1.0 * (k // 5 % 5), 5.0 + 1.0 * (k // 25)], axis=1)
    g = mrs.Swarm(n, arith=arith)
    g.construct(0, n, mrs.model_params("x500"), pos)
    if mixed:
        for a in range(192, n, 10):
            g.construct(a, min(5, n - a), mrs.model_params("f550"), pos[a:a + 5])
    st = g.get_states()
    g.set_state(0, n, pos, v, st["R"].reshape(n, 9), st["omega"], st["motor_rpm"])
    g.set_input(0, n, mrs.POSITION_CMD, np.concatenate([pos, np.zeros((n, 1))], axis=1))
    return g


def tick_loop(g, mode, cmd, groups, first, hold, every, crash, crash_rows=True):
    """the loop of the contract, through tensors: (observation row blocks or None, crash row blocks or None)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    blocks, count = cmd.shape[0], cmd.shape[1]
    ticks = blocks * hold
    out = torch.empty((ticks // every, count, T.gather_width(groups)), dtype=cmd.dtype, device=cmd.device) if groups else None
    cr = torch.empty((ticks // every, count), dtype=torch.bool, device=cmd.device) if crash_rows else None
    for t in range(ticks):
        if t % hold == 0:
            T.set_input(g, mode, cmd[t // hold], first)
        g.step_n(DT, 1)  # evaluates the collision tick pending from tick t - 1
        if (t + 1) % every == 0:
            j = (t + 1) // every - 1
            if groups:
                T.gather(g, groups, first, count, out=out[j])
            if crash_rows:
                T.crashed(g, first, count, out=cr[j])
        g.handle_collisions(True, crash, REBOUNCE)  # stays pending
    return out, cr


def assert_rows(want, got, what):
    (wo, wc), (go, gc) = want, got
    if wo is not None:
        w, g = wo.cpu().numpy(), go.cpu().numpy()
        assert np.array_equal(w.view(np.uint8), g.view(np.uint8)), f"{what}: observation rows differ at {np.argwhere(w != g)[:5]}"
    if wc is not None:
        w, g = wc.cpu().numpy().view(np.uint8), gc.cpu().numpy().view(np.uint8)
        assert np.array_equal(w, g), f"{what}: crash bytes differ at {np.argwhere(w != g)[:5]}"


def assert_same_swarm(a, b, what):
    assert_same_state(a, b, what)  # state, IMU, PID, external force, crash flags
    assert a.get_diag() == b.get_diag(), f"{what}: diag counters"


RATES = ((1, 1), (4, 2), (3, 6), (48, 48))  # (hold, obs_every)


def configs():
    """n_ticks in (1, 5, 48) with every pair of rates that divides it"""
    return [(t, h, e) for t in (1, 5, 48) for h, e in RATES if t % h == 0 and t % e == 0]


@pytest.mark.parametrize("crash", [True, False], ids=["crash", "elastic"])
def test_literal_equals_the_loop(mrs, crash):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(71)
    # ---- variant swarm: every configuration, one after the other on the same two swarms
    for scen, modes in (("cascade", (O.VELOCITY_HDG_CMD, O.ACTUATOR_CMD)), ("model", (O.ACTUATOR_CMD,))):
        a, b = variant_swarm(mrs, scen, mrs.ARITH_LITERAL), variant_swarm(mrs, scen, mrs.ARITH_LITERAL)
        assert np.asarray(a.has_crashed()).any(), "the scenario has crashed UAVs"
        dev = torch_dev(a)
        for dtype in (torch.float64, torch.float32):
            for mode in modes:
                for ticks, hold, every in configs():
                    x = a.get_states(FIRST, COUNT)["x"]
                    cmd = torch.tensor(commands(mode, rng, ticks // hold, COUNT, x), dtype=dtype, device=dev)
                    want = tick_loop(a, mode, cmd, T.OBS_ALL, FIRST, hold, every, crash)
                    got = T.rollout_ticks(b, mode, cmd, DT, crash, REBOUNCE, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every)
                    what = f"variant {scen} {dtype} mode {mode} T={ticks} hold={hold} obs_every={every}"
                    assert_rows(want, got, what)
                    assert_same_swarm(a, b, what)
        print(f"variant {scen} crash={crash}: fused_stats of the calls' swarm {b.fused_stats()}, of the loop's {a.fused_stats()}")
        for g in (a, b):
            g.tick_n(DT, 9, True, crash, REBOUNCE)
        assert_same_swarm(a, b, f"variant {scen}: 9 ticks after the calls")
        assert b.get_diag()["nan_rollback"] > 0
    # ---- pair swarm: fresh swarms per configuration (the pairs meet once), fused launches
    for mode, mixed in ((O.POSITION_CMD, False), (O.ACTUATOR_CMD, False), (O.POSITION_CMD, True)):
        for dtype in (torch.float64, torch.float32):
            for ticks, hold, every in (configs() if not mixed else [(48, 4, 2)]):
                if ticks < 48 and dtype == torch.float32:
                    continue
                a, b = pair_swarm(mrs, mrs.ARITH_LITERAL, mixed), pair_swarm(mrs, mrs.ARITH_LITERAL, mixed)
                dev = torch_dev(a)
                pos, _ = pair_state()
                if mode == O.POSITION_CMD:  # the own positions, moved a little per block
                    c = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (ticks // hold, N_PAIR, 4))
                else:  # near hover, dense rows of 8 throttles (f550 has 6 motors)
                    c = 0.45 + rng.uniform(-0.02, 0.02, (ticks // hold, N_PAIR, 8))
                cmd = torch.tensor(c, dtype=dtype, device=dev)
                fused0 = b.fused_stats()[0]
                want = tick_loop(a, mode, cmd, T.OBS_ALL, 0, hold, every, crash)
                got = T.rollout_ticks(b, mode, cmd, DT, crash, REBOUNCE, T.OBS_ALL, first=0, hold=hold, obs_every=every)
                what = f"pair mode {mode} mixed={mixed} {dtype} T={ticks} hold={hold} obs_every={every}"
                assert_rows(want, got, what)
                assert_same_swarm(a, b, what)
                assert b.fused_stats()[0] - fused0 >= ticks - 1, f"{what}: the ticks after the first are fused launches"
                if ticks == 48:
                    cr = got[1].cpu().numpy()
                    if crash:  # some crash byte goes 0 -> 1 strictly inside the call
                        assert cr[-1, :2 * PAIRS].all() and not cr[-1, 2 * PAIRS:].any(), what
                        assert every == 48 or not cr[0].any(), what
                        if every == 1 and mode == O.POSITION_CMD:
                            assert int(np.argmax(cr.any(axis=1))) == 21, f"{what}: first crash byte in block {np.argmax(cr.any(axis=1))}"
                    else:  # the pairs' velocities differ from a collision-free twin's
                        assert not cr.any(), what
                        twin = pair_swarm(mrs, mrs.ARITH_LITERAL, mixed)
                        T.rollout(twin, mode, cmd, DT, 0, first=0, hold=hold)
                        v, vt = b.get_states()["v"], twin.get_states()["v"]
                        assert (np.abs(v[:2 * PAIRS] - vt[:2 * PAIRS]).max(axis=1) > 0).all(), f"{what}: the pairs felt no force"
                        assert same(v[2 * PAIRS:], vt[2 * PAIRS:]), what
                    for g in (a, b):
                        g.tick_n(DT, 9, True, crash, REBOUNCE)
                    assert_same_swarm(a, b, f"{what}: 9 ticks after the call")


def test_stall_and_replay_inside_a_call(mrs):
    import torch
    import mrs_multirotor_simulator_amd as M
    from mrs_multirotor_simulator_amd import tensors as T
    ticks, hold, every, n_fast = 48, 4, 2, 4
    a, b = (pair_swarm(mrs, mrs.ARITH_LITERAL, n_fast=n_fast) for _ in range(2))
    dev = torch_dev(a)
    rng = np.random.default_rng(73)
    pos, _ = pair_state()
    cmd = torch.tensor(np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (ticks // hold, N_PAIR, 4)), device=dev)
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_QUAT
    for g in (a, b):  # live lists: every tick of the call can be a fused launch
        g.tick_n(DT, 2, True, True, REBOUNCE)
    want = tick_loop(a, O.POSITION_CMD, cmd, groups, 0, hold, every, True)
    out = torch.full((ticks // every, N_PAIR, T.gather_width(groups)), -12345.678, dtype=torch.float64, device=dev)
    cr = torch.full((ticks // every, N_PAIR), 7, dtype=torch.uint8, device=dev)
    fused0, stalls0, replayed0, _ = b.fused_stats()
    # the device is held back while the host queues its launches: the stall of the first one is seen when others are queued behind it
    assert M.load_library().mrs_debug_stream_delay(C.c_void_p(b.stream()), C.c_double(20000.0)) == 0
    got = T.rollout_ticks(b, O.POSITION_CMD, cmd, DT, True, REBOUNCE, groups, first=0, out=out, hold=hold, obs_every=every, crashed=cr)
    fused, stalls, replayed, _ = b.fused_stats()
    print(f"stall inside a call: {fused - fused0} fused launches, {stalls - stalls0} stalls, {replayed - replayed0} replayed")
    assert fused - fused0 >= 40 and stalls - stalls0 >= 1 and replayed - replayed0 >= 1, (fused - fused0, stalls - stalls0, replayed - replayed0)
    o, c = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert not (o == -12345.678).any() and not (c == 7).any(), "every row was written"
    assert np.array_equal(want[0].cpu().numpy().view(np.uint8), o.view(np.uint8)), "observation rows"
    assert np.array_equal(want[1].cpu().numpy().view(np.uint8), c), "crash bytes"
    assert c[-1, :2 * PAIRS].all()
    # the launch log is empty after the call: looking at the swarm replays nothing more
    T.gather(b, groups, 0, N_PAIR, dtype=torch.float64)
    assert b.fused_stats()[1:3] == (stalls, replayed)
    assert_same_swarm(a, b, "after the call")


def test_unfused_paths(mrs, monkeypatch):
    """the paths of a tick without the fused form give the loop's rows: the first tick after a host write of positions (lists dirty,
    the collision pass on its own, then a launch without evaluation), neighbourhoods denser than the list capacity (lists incomplete:
    every tick on its own), MRS_FUSED_COLLISIONS=0 (every collision tick evaluated when it is requested) and MRS_NEIGHBOUR_LISTS=0"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(79)
    ticks, hold, every = 48, 3, 6
    pos, v = pair_state()
    c = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (ticks // hold, N_PAIR, 4))

    def run(make, what, crash, dirty=False, fused=None):
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
        fused0 = b.fused_stats()[0]
        want = tick_loop(a, O.POSITION_CMD, cmd, T.OBS_ALL, 0, hold, every, crash)
        got = T.rollout_ticks(b, O.POSITION_CMD, cmd, DT, crash, REBOUNCE, T.OBS_ALL, first=0, hold=hold, obs_every=every)
        assert_rows(want, got, what)
        assert_same_swarm(a, b, what)
        n_fused = b.fused_stats()[0] - fused0
        if fused is not None:
            assert (n_fused > 0) == fused, f"{what}: {n_fused} fused launches"
        effect = got[1].cpu().numpy()[-1, :2 * PAIRS].all() if crash else np.abs(b.get_external_force()[:2 * PAIRS]).sum() > 0
        assert effect, f"{what}: the pairs met"

    for crash in (True, False):
        run(lambda: pair_swarm(mrs, mrs.ARITH_LITERAL), f"dirty lists crash={crash}", crash, dirty=True, fused=True)
        run(lambda: pair_swarm(mrs, mrs.ARITH_LITERAL, dense=True), f"dense cluster crash={crash}", crash, fused=False)
    monkeypatch.setenv("MRS_FUSED_COLLISIONS", "0")  # (read when a swarm is created)
    run(lambda: pair_swarm(mrs, mrs.ARITH_LITERAL), "MRS_FUSED_COLLISIONS=0", True, fused=False)
    monkeypatch.delenv("MRS_FUSED_COLLISIONS")
    monkeypatch.setenv("MRS_NEIGHBOUR_LISTS", "0")
    run(lambda: pair_swarm(mrs, mrs.ARITH_LITERAL), "MRS_NEIGHBOUR_LISTS=0", False, fused=False)


def test_fast(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(83)
    ticks, hold, every, cut = 24, 4, 2, 10  # the cut at tick 10 falls inside command block 2 (ticks 8-11)
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_ROT
    for make, first, count, mode, label in (
            (lambda: variant_swarm(mrs, "cascade", mrs.ARITH_FAST), FIRST, COUNT, O.ATTITUDE_RATE_CMD, "variant"),
            (lambda: pair_swarm(mrs, mrs.ARITH_FAST), 0, N_PAIR, O.ATTITUDE_RATE_CMD, "pair")):
        for crash in (True, False):
            loop_g, one, single, split = make(), make(), make(), make()
            dev = torch_dev(one)
            blocks = commands(mode, rng, ticks // hold, count, None)
            per_tick = torch.tensor(np.repeat(blocks, hold, axis=0), device=dev)  # command row of every tick
            cmd = torch.tensor(blocks, device=dev)
            what = f"FAST {label} crash={crash}"
            got = T.rollout_ticks(one, mode, cmd, DT, crash, REBOUNCE, groups, first=first, hold=hold, obs_every=every)
            # 24 calls of one tick
            rows = [T.rollout_ticks(single, mode, per_tick[t:t + 1], DT, crash, REBOUNCE, groups, first=first) for t in range(ticks)]
            o1 = torch.cat([r[0] for r in rows])[every - 1::every]
            c1 = torch.cat([r[1] for r in rows])[every - 1::every]
            assert_rows(got, (o1, c1), f"{what}: one call vs single-tick calls")
            assert_same_swarm(one, single, f"{what}: one call vs single-tick calls")
            # two calls, cut inside a held command block (the second call starts with the rest of that block)
            r1 = T.rollout_ticks(split, mode, per_tick[:cut:2].contiguous(), DT, crash, REBOUNCE, groups, first=first, hold=2, obs_every=every)
            r2 = T.rollout_ticks(split, mode, per_tick[cut::2].contiguous(), DT, crash, REBOUNCE, groups, first=first, hold=2, obs_every=every)
            assert_rows(got, (torch.cat([r1[0], r2[0]]), torch.cat([r1[1], r2[1]])), f"{what}: one call vs two calls")
            assert_same_swarm(one, split, f"{what}: one call vs two calls")
            # close to the loop after one tick, on the finite rows
            want = tick_loop(loop_g, mode, per_tick[:1], groups, first, 1, 1, crash)[0].cpu().numpy()[0]
            near = rows[0][0].cpu().numpy()[0]
            ok = np.isfinite(want).all(axis=1)
            if label == "variant":  # v[2400] = NaN by construction (single_scenario): the one UAV of the range with non-finite rows
                assert list(np.flatnonzero(~ok)) == [2400 - FIRST] and (~ok).sum() <= 0.01 * count, np.flatnonzero(~ok)
            else:
                assert ok.all()
            assert np.array_equal(np.isfinite(near).all(axis=1), ok), what
            helpers.assert_close(near[ok], want[ok], RTOL_FAST, f"{what}: rows after one tick vs the loop")


def test_held_crashed_and_outside(mrs):
    """UAV 0 (the partner of UAV 1) and the lone UAV 100 are on hold inside the range [0, 128): their rows show their unchanged state,
    UAV 1 still flies into UAV 0 and both crash; the UAVs outside the range go on exactly as under tick_n"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ticks = 48
    a, b, twin = (pair_swarm(mrs, mrs.ARITH_LITERAL) for _ in range(3))
    for g in (a, b, twin):
        g.set_hold(0, 1, True)
        g.set_hold(100, 1, True)
    dev = torch_dev(a)
    rng = np.random.default_rng(89)
    pos, _ = pair_state()
    count = 128
    c = np.concatenate([pos[:count], np.zeros((count, 1))], axis=1)[None] + rng.normal(0, 0.01, (ticks, count, 4))
    cmd = torch.tensor(c, device=dev)
    before = T.gather(b, T.OBS_ALL, 0, count, dtype=torch.float64).cpu().numpy()
    want = tick_loop(a, O.POSITION_CMD, cmd, T.OBS_ALL, 0, 1, 1, True)
    got = T.rollout_ticks(b, O.POSITION_CMD, cmd, DT, True, REBOUNCE, T.OBS_ALL, first=0)
    assert_rows(want, got, "held UAVs in the range")
    assert_same_swarm(a, b, "held UAVs in the range")
    o, cr = got[0].cpu().numpy(), got[1].cpu().numpy()
    for k in (0, 100):
        assert all(same(o[t, k], before[k]) for t in range(ticks)), f"held UAV {k}: rows of its unchanged state"
    assert cr[-1, 0] and cr[-1, 1] and not cr[0, :2].any(), "UAV 1 flew into the held UAV 0: both crashed inside the call"
    assert not cr[:, 100].any()
    assert cr[-1, 2:2 * PAIRS].all()
    # the held UAVs took the command rows: the last one is in their command columns (they fly to it once released)
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
    _, obs = R._hip_malloc(4 * 100 * 36 * 8)
    _, small = R._hip_malloc(3 * 100 * 36 * 8)
    _, crashed = R._hip_malloc(4 * 100)
    _, short = R._hip_malloc(4 * 100 - 1)
    host = np.zeros((4, 100, 36))
    ok = dict(first=0, count=100, mode=O.POSITION_CMD, dt=DT, n_ticks=4, cmd_every=2, obs_every=1, dev_cmd=cmd, dtype=T.DTYPE_F64,
              cmd_stride=10, groups=T.OBS_ALL, dev_obs=obs, obs_stride=36, dev_crashed=crashed, crash=True, rebounce=REBOUNCE, ext_stream=None)
    bad = [({"first": N_SINGLE - 5}, 3), ({"count": -1}, 3), ({"mode": 11}, 1), ({"mode": -1}, 1), ({"dtype": 2}, 1), ({"n_ticks": 0}, 1),
           ({"dt": 0.0}, 1), ({"dt": -DT}, 1), ({"dt": float("nan")}, 1), ({"dt": float("inf")}, 1), ({"cmd_stride": 3}, 1),
           ({"groups": 0x100}, 1), ({"obs_stride": 35}, 1), ({"dev_obs": None}, 1), ({"dev_cmd": None}, 1), ({"dev_cmd": host.ctypes.data}, 1),
           ({"dev_obs": small}, 1), ({"n_ticks": 5}, 1), ({"cmd_every": 0}, 1), ({"cmd_every": 3}, 1), ({"obs_every": 0}, 1),
           ({"obs_every": 3}, 1), ({"n_ticks": 6}, 1), ({"dev_crashed": short}, 1), ({"dev_crashed": host.ctypes.data}, 1),
           ({"rebounce": float("nan")}, 1), ({"rebounce": float("inf")}, 1), ({"mode": O.ACTUATOR_CMD, "cmd_stride": 4, "first": 1900}, 1)]
    for change, code in bad:
        with pytest.raises(mrs.MrsError, match=f"error {code}:"):
            g.rollout_tick_device(**dict(ok, **change))
        assert np.array_equal(T.save(g).cpu().numpy(), before), change
    back, cb = np.zeros(4 * 100 * 36), np.zeros(4 * 100, dtype=np.uint8)
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(obs), back.nbytes, 2) == 0
    assert hip.hipMemcpy(cb.ctypes.data_as(C.c_void_p), C.c_void_p(crashed), cb.nbytes, 2) == 0
    assert not back.any() and not cb.any(), "a refused call wrote rows"
    with pytest.raises(ValueError):  # the tensor layer refuses before any library call
        T.rollout_ticks(g, O.POSITION_CMD, torch.zeros((4, 100, 4), dtype=torch.float64), DT, True, REBOUNCE)
    # the unchanged arguments are accepted, and so are: no crash rows, no observation rows, neither
    g.rollout_tick_device(**ok)
    g.rollout_tick_device(**dict(ok, dev_crashed=None))
    g.rollout_tick_device(**dict(ok, groups=0, dev_obs=None))
    g.rollout_tick_device(**dict(ok, groups=0, dev_obs=None, dev_crashed=None))
    torch.cuda.synchronize(dev)
    assert not np.array_equal(T.save(g).cpu().numpy(), before)
    for p in (cmd, obs, small, crashed, short):
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
    out = torch.zeros((2, 100, 10), dtype=torch.float64, device=dev)
    cr = torch.zeros((2, 100), dtype=torch.uint8, device=dev)
    for g in shards:
        x = g.get_states()["x"]
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.rollout_ticks(g, O.POSITION_CMD, cmd, DT, True, REBOUNCE, out=out, crashed=cr)
        assert same(g.get_states()["x"], x)
    assert not out.any() and not cr.any()
    for g in shards:
        g.close()
    group.close()


def test_caller_stream_is_fenced(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, b, c = (pair_swarm(mrs, mrs.ARITH_LITERAL) for _ in range(3))
    dev = torch_dev(a)
    rng = np.random.default_rng(97)
    pos, _ = pair_state()
    src = torch.tensor(np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (30, N_PAIR, 4)), device=dev)
    want = T.rollout_ticks(a, O.POSITION_CMD, src, DT, True, REBOUNCE, T.OBS_ALL)
    wo, wc = want[0].cpu().numpy(), want[1].cpu().numpy()
    assert wc[-1, :2 * PAIRS].all()
    for g, side in ((b, torch.cuda.Stream(dev)), (c, torch.cuda.ExternalStream(c.stream(), device=dev))):
        cmd = torch.zeros_like(src)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
            cmd.copy_(src)  # written on the caller stream right before the call, no synchronisation
            out, cr = T.rollout_ticks(g, O.POSITION_CMD, cmd, DT, True, REBOUNCE, T.OBS_ALL)
            copy, ccopy = out.clone(), cr.clone()  # torch work after the call sees the rows
        side.synchronize()
        assert same(copy.cpu().numpy(), wo) and np.array_equal(ccopy.cpu().numpy(), wc)
        assert_same_swarm(a, g, "fenced tick rollout")


def child_main(out_path):
    """the pointer-addressed kernel (MRS_NO_BUFFER_ADDRESSING=1): fused ticks of the pair swarm equal the loop in LITERAL, in both crash
    modes, and FAST equals itself split into single ticks"""
    import torch
    import mrs_multirotor_simulator_amd as M
    from mrs_multirotor_simulator_amd import tensors as T
    M.load_library()
    rng = np.random.default_rng(101)
    pos, _ = pair_state()
    res = []
    for crash in (True, False):
        a, b = pair_swarm(M, M.ARITH_LITERAL, mixed=True), pair_swarm(M, M.ARITH_LITERAL, mixed=True)
        dev = torch_dev(a)
        c = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (12, N_PAIR, 4))
        cmd = torch.tensor(c, dtype=torch.float32, device=dev)
        want = tick_loop(a, O.POSITION_CMD, cmd, T.OBS_ALL, 0, 4, 2, crash)
        got = T.rollout_ticks(b, O.POSITION_CMD, cmd, DT, crash, REBOUNCE, T.OBS_ALL, hold=4, obs_every=2)
        assert_rows(want, got, f"LITERAL crash={crash}")
        assert_same_swarm(a, b, f"LITERAL crash={crash}")
        assert b.fused_stats()[0] >= 47
        assert got[1][-1, :2 * PAIRS].all() if crash else np.abs(b.get_external_force()[:2 * PAIRS]).sum() > 0
        f1, f2 = pair_swarm(M, M.ARITH_FAST), pair_swarm(M, M.ARITH_FAST)
        one = T.rollout_ticks(f1, O.POSITION_CMD, cmd[:6], DT, crash, REBOUNCE, T.OBS_ALL)
        parts = [T.rollout_ticks(f2, O.POSITION_CMD, cmd[t:t + 1], DT, crash, REBOUNCE, T.OBS_ALL) for t in range(6)]
        assert_rows(one, (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])), f"FAST crash={crash}")
        res.append(str(crash))
    np.save(out_path, np.array(res))


def test_pointer_form(mrs, tmp_path):
    if _dead:
        pytest.fail(f"an earlier child process of this module died ({_dead[0]}): no further GPU process is started")
    out = str(tmp_path / "pointer.npy")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MRS_")}
    env["MRS_NO_BUFFER_ADDRESSING"] = "1"
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_rollout_tick_gpu as T; T.child_main({out!r})"
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
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, B, hold, every, W = 1000, 6, 4, 2, 10
    rows = B * hold // every
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rollout_tick.bin")
        out = subprocess.run([build_cpp("rollout_tick_test"), path], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok rows_equal_the_loop", "ok crash_bytes", "ok last_row_equals_pose_array", "ok refused_call_changes_nothing", "ok written"):
            assert tag in out.stdout, out.stdout
        raw = np.fromfile(path, np.uint8)
    obs, cr = raw[:rows * n * W * 8].view(np.float64), raw[rows * n * W * 8:]
    i = np.arange(n)
    pos = np.stack([4.0 * (i % 32), 4.0 * (i // 32), np.full(n, 5.0)], axis=1)
    odd = np.arange(1, 2 * PAIRS, 2)
    pos[odd] = np.stack([4.0 * (odd - 1) + 0.4, np.zeros(PAIRS), np.full(PAIRS, 5.0)], axis=1)
    g = mrs.Swarm(n, arith=mrs.ARITH_LITERAL)
    g.construct(0, n, mrs.default_params(), pos, 0.003 * i)
    t = np.arange(B)[:, None]
    cmd = np.stack([np.broadcast_to(0.02 * np.sin(0.1 * t + 0.001 * i), (B, n)), np.broadcast_to(-0.01 + 0.0 * t + 0.0 * i, (B, n)),
                    np.broadcast_to(0.3 + 0.0001 * i + 0.0 * t, (B, n)), np.broadcast_to(0.55 + 0.005 * t + 0.0 * i, (B, n))], axis=2)
    mine, mc = T.rollout_ticks(g, O.ATTITUDE_RATE_CMD, torch.tensor(cmd, device=torch_dev(g)), DT, True, REBOUNCE,
                               T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, hold=hold, obs_every=every)
    assert obs.shape == (rows * n * W,) and same(obs, mine.cpu().numpy().reshape(-1))
    assert np.array_equal(cr, mc.cpu().numpy().view(np.uint8).reshape(-1))
