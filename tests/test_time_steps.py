"""The yardstick of test_time_steps_gpu.py, without a GPU.  (1) The oracle against the independent restatement (independent_model.Uav)
at the shipped rates 0.01 s and 0.004 s and across dt changes: every GPU test there compares with the oracle, which so far had a
second opinion at 1 ms only.  (2) A condition on every dt-change scene of the GPU tests: an oracle run that keeps dt_a where dt_b belongs must end with
other motor speeds on at least 90 % of the UAVs — a scene that a stale motor-filter table would not move proves nothing.  (3) The
runners of the stall scene cross half the skin where the recipe says, by the oracle's own trajectory."""
import numpy as np
import pytest

import helpers
import independent_model as IM
import time_steps as TS
from test_independent_restatement import compare, make_pair, payload


def start(O, rng, mode, airframe="x500"):
    """an oracle UAV and its restatement in a perturbed flying state with a command of `mode`"""
    o, u, po = make_pair(O, airframe, rng, ground_enabled=True, ground_z=0.0)
    nm = int(po.n_motors)
    st = helpers.random_state(rng, 1, nm, tilted=True)
    o.set_state(0, 1, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    u.x, u.v, u.R, u.omega, u.motor_rpm = st["x"][0].copy(), st["v"][0].copy(), st["R"][0].copy(), st["omega"][0].copy(), st["motor_rpm"][0][:nm].copy()
    pl = payload(O, mode, rng, nm, st["x"][0])
    o.set_input(0, 1, mode, None if pl is None else pl[None, :])
    u.set_input(mode, pl)
    return o, u


@pytest.mark.parametrize("dt", [0.01, 0.004])
@pytest.mark.parametrize("mode", list(range(0, 11)))
def test_oracle_against_the_restatement_at_the_shipped_rates(oracle, mode, dt):
    """mode 0 is free fall (no input ever arrived), 1 the actuators, 2-10 the controller cascade from the mixer up; 1 s of flight"""
    o, u = start(oracle, np.random.default_rng(2000 + mode), mode, ("x500", "f550", "naki")[mode % 3])
    steps = int(round(1.0 / dt))
    for k in range(steps):
        o.step(dt)
        u.make_step(dt)
        if (k + 1) % (steps // 4) == 0:
            compare(o, u, f"mode {mode} dt {dt} step {k + 1}")


@pytest.mark.parametrize("mode", [0, 1, 4, 8, 10])
def test_oracle_against_the_restatement_across_dt_changes(oracle, mode):
    """dt changes every 25 steps through the suite's value, the shipped rates, the inexact reciprocal and the small one: the PID
    derivative divides by the dt of the call, the motor filter uses exp(-dt / tau) of the call"""
    o, u = start(oracle, np.random.default_rng(3000 + mode), mode)
    for block, dt in enumerate((0.001, 0.01, 0.004, 0.001, 1.0 / 300.0, 0.0005, 0.01, 0.004)):
        for _ in range(25):
            o.step(dt)
            u.make_step(dt)
        compare(o, u, f"mode {mode}, block {block} (dt {dt})")


# ---- sensitivity of the scenes ------------------------------------------------------------------------------------------------------
def run(O, scene, ops, **kw):
    o = TS.build_oracle(O, helpers, scene, **kw)
    for op in ops:
        TS.oracle_call(o, scene["n"], op)
    return o.get_state()["motor_rpm"]


@pytest.mark.parametrize("a,b", TS.DT_PAIRS)
def test_the_plain_scene_feels_a_missed_dt_change(oracle, a, b):
    scene = TS.plain_scene()
    moved = TS.rpm_moved(run(oracle, scene, TS.plain_ops(a, b)), run(oracle, scene, TS.wrong_ops(a, b)))
    assert moved >= 0.9, f"only {moved:.0%} of the UAVs end with other motor speeds"


def block_scenes():
    two = TS.sample_of(TS.two_stream_scene())[0]
    coll, coll_blocks = TS.collision_scene()
    shard, shard_blocks = TS.sharded_scene()
    return {"two_stream": (two, TS.two_stream_blocks(), dict(ground_enabled=True, ground_z=0.0)),
            "collision_ticks": (coll, coll_blocks, {}),
            "sharded": (shard, shard_blocks, dict(ground_enabled=True, ground_z=0.0)),
            "three_steps": (TS.stall_scene(TS.THREE_DTS[0]), TS.three_step_blocks(), dict(ground_enabled=True, ground_z=0.0))}


@pytest.mark.parametrize("name,changes", [("two_stream", 1), ("collision_ticks", 2), ("sharded", 2), ("three_steps", 3)])
def test_the_block_sequences_feel_every_missed_dt_change(oracle, name, changes):
    """the two-stream runs (on the sample the GPU test compares), the collision ticks at the shipped rates, the sharded ticks and the
    three-time-step sequence: behind every change of dt, the block that kept the old dt ends with other motor speeds"""
    scene, blocks, kw = block_scenes()[name]
    moved = TS.missed_changes(lambda: TS.build_oracle(oracle, helpers, scene, **kw), scene["n"], blocks)
    assert len(moved) == changes, moved
    for i, frac in moved:
        assert frac >= 0.9, f"{name}, block {i} (dt {blocks[i]['dt']}): only {frac:.0%} of the UAVs end with other motor speeds"


_first_call = {}


def after_first_call(O, a, crash):
    """the stall scene through tick_n(dt_a, STALL_TICKS), once per (dt_a, crash): (scene, oracle, runner positions after every tick)"""
    if (a, crash) not in _first_call:
        scene = TS.stall_scene(a)
        o = TS.build_oracle(O, helpers, scene, ground_enabled=True, ground_z=0.0)
        track = []
        for _ in range(TS.STALL_TICKS):
            o.step(a)
            o.handle_collisions(True, crash, TS.REBOUNCE)
            track.append(o.get_state(0, TS.N_RUNNERS)["x"].copy())
        _first_call[(a, crash)] = (scene, o, track)
    return _first_call[(a, crash)]


@pytest.mark.parametrize("a", sorted({p[0] for p in TS.DT_PAIRS}))
def test_the_runners_cross_half_the_skin_two_ticks_before_the_end(oracle, a):
    """displacement since the search (behind step 1): under the warning fraction up to step ticks - 3, over half the skin at step ticks - 2"""
    _, _, track = after_first_call(oracle, a, False)
    d = [np.linalg.norm(x - track[0], axis=1) for x in track]
    k = TS.STALL_TICKS
    assert all((d[j] < TS.WARN_FRACTION * TS.SKIN_HALF).all() for j in range(k - 3)), [x.max() for x in d]
    assert (d[k - 3] > TS.SKIN_HALF).all(), d[k - 3]


@pytest.mark.parametrize("kind", ["step_n_2", "step", "tick_n", "step_range"])  # (the other second calls are one of these to the oracle)
@pytest.mark.parametrize("a,b", TS.DT_PAIRS)
def test_the_stall_scene_feels_a_missed_dt_change(oracle, a, b, kind):
    """the second call at dt_b against the same call at dt_a, from the state the first call left: the motor speeds of (nearly) every UAV
    it stepped must differ, so a second call that ran with dt_a's motor-filter constants cannot pass the GPU comparison"""
    O = oracle
    scene = TS.stall_scene(a)
    n = scene["n"]
    got = []
    for dt in (b, a):
        o = TS.build_oracle(O, helpers, scene, ground_enabled=True, ground_z=0.0)
        for _ in range(TS.STALL_TICKS):
            o.step(a)
            o.handle_collisions(True, False, TS.REBOUNCE)
        for op in TS.second_call_ops(kind, dt, n, False):
            TS.oracle_call(o, n, op)
        got.append(o.get_state()["motor_rpm"])
    stepped = slice(0, n // 2) if kind == "step_range" else slice(0, n)
    moved = TS.rpm_moved(got[0][stepped], got[1][stepped])
    assert moved >= 0.9, f"only {moved:.0%} of the UAVs end with other motor speeds"
