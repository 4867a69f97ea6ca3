"""What the time-step tests share (test_time_steps.py without a GPU, test_time_steps_gpu.py with one): the time steps, the scenes in
which dt changes between two calls, and the call sequences, written once so that the CPU tests judge exactly the scenes the GPU tests
run.  A "target" below is an oracle swarm or a product swarm: both take the same calls; what the oracle lacks (step_range, tick_n) is
spelled out for it here."""
import numpy as np

from mrs_multirotor_simulator_amd import synthetic

DTS = (0.01, 0.004, 1.0 / 300.0, 0.0005)  # the two shipped rates, an inexact reciprocal, below the suite's own 1 ms
DT_PAIRS = ((0.001, 0.01), (0.01, 0.001), (0.01, 0.004), (0.004, 0.01))
DT_C = 1.0 / 300.0
REBOUNCE = 100.0
SKIN_HALF = 0.25        # a UAV that moved further than this since the last neighbour search stalls the launch log (collide_work.h)
WARN_FRACTION = 0.75    # ... and from this fraction of it on the host is asked to search ahead of time
POSITION_CMD, ACTUATOR_CMD = 10, 1

# ---- plain paths (no collisions) -------------------------------------------------------------------------------------------------
PLAIN_N = 512


def plain_scene():
    """512 x500: the first half in the position cascade, the second half on actuator commands.  The motors start at 3000-5000 rpm and
    the actuator commands ask for 15-30 % or 75-90 % throttle, far from where the motors are: a motor filter of the wrong dt shows."""
    rng = np.random.default_rng(2024)
    n, h = PLAIN_N, PLAIN_N // 2
    st = synthetic.random_state(rng, n, 4, tilted=True)
    goal = np.concatenate([st["x"][:h] + rng.uniform(-5, 5, (h, 3)), rng.uniform(-3.14, 3.14, (h, 1))], axis=1)
    act = np.where(rng.uniform(size=(n - h, 1)) < 0.5, rng.uniform(0.15, 0.30, (n - h, 4)), rng.uniform(0.75, 0.90, (n - h, 4)))
    return dict(n=n, st=st, inputs=[(0, h, POSITION_CMD, goal), (h, n - h, ACTUATOR_CMD, act)])


def plain_ops(a, b, c=DT_C):
    """the call sequence of the plain dt-change test; [0] is the call's name, the rest its arguments"""
    return [("step_n", a, 7, 1), ("step", b), ("step_n", b, 9, 3), ("step_range", 100, 200, c), ("step_n", a, 5, 1)]


def wrong_ops(a, b, c=DT_C):
    """the same sequence with dt_a where dt_b belongs: what a library that missed the change would compute"""
    return plain_ops(a, a, c)


def oracle_call(o, n, op):
    """one call of a sequence on an oracle swarm of n UAVs"""
    name, args = op[0], op[1:]
    if name == "step_n":
        o.step_n(args[0], args[1])  # (substeps_per_launch is a launch shape: the oracle has none)
    elif name == "step":
        o.step(args[0])
    elif name == "step_range":  # everybody else on hold, as tests/test_pool_primitives_gpu.py does it
        first, count, dt = args
        if first > 0:
            o.set_hold(0, first, True)
        if first + count < n:
            o.set_hold(first + count, n - first - count, True)
        o.step(dt)
        o.set_hold(0, n, False)
    elif name == "tick_n":
        dt, k, crash = args
        for _ in range(k):
            o.step(dt)
            o.handle_collisions(True, crash, REBOUNCE)
    else:
        raise ValueError(name)


def rpm_moved(a, b):
    """fraction of the UAVs whose motor speeds differ by more than 1e-4 relative between two runs"""
    d = np.abs(a - b).max(axis=1) / np.maximum(np.abs(a).max(axis=1), 1e-300)
    return float((d > 1e-4).mean())


# ---- a non-empty launch log (collision ticks, a stall) -----------------------------------------------------------------------------
STALL_N = 4096
STALL_TICKS = 6     # ticks of the first call
N_RUNNERS = 8
SECOND_CALLS = ("step_n_2", "step_n_1", "step", "tick_n", "step_range", "rollout", "rollout_ticks", "get_states+step_n_2")


def runner_speed(dt_a, ticks=STALL_TICKS):
    """The first collision tick (behind step 1) searches; steps 2 .. ticks are launches of the log, measured against the positions of
    that search.  A runner is over half the skin after step `ticks - 2`, i.e. after ticks - 3 steps of the log, and two launches are
    queued behind that one; 6 % over, so that it is still under WARN_FRACTION of it one step earlier ((ticks - 4) / (ticks - 3) * 1.06
    = 0.71 for 6 ticks) and no search is queued ahead of time."""
    return 1.06 * SKIN_HALF / ((ticks - 3) * dt_a)


def stall_scene(dt_a, seed=11):
    """The stall recipe of tests/test_pose_payload_gpu.py scaled down: 4096 x500 at 16 m^3 per UAV holding positions up to 5 m away,
    collisions on; 8 runners, lifted 40 m above the cloud so that they meet nobody, at the speed of runner_speed(dt_a)."""
    import bench
    st, cmd = bench.make_inputs(STALL_N, "position+collisions", seed=seed, volume_per_uav=16.0)
    side = (16.0 * STALL_N) ** (1.0 / 3.0)
    st["x"][:N_RUNNERS, 2] = side / 4 + 45.0 + 8.0 * np.arange(N_RUNNERS)
    st["v"][:N_RUNNERS] = [0.0, runner_speed(dt_a), 0.0]
    st["R"][:N_RUNNERS] = np.eye(3)
    st["omega"][:N_RUNNERS] = 0.0
    # the runners are asked to go on where they are going: the velocity limit of the cascade brakes them, but slowly
    cmd[:N_RUNNERS, :3] = st["x"][:N_RUNNERS] + [0.0, 500.0, 0.0]
    cmd[:N_RUNNERS, 3] = 0.0
    return dict(n=STALL_N, st=st, cmd=cmd)


def second_call_ops(kind, dt_b, n, crash):
    """what the oracle does for the second call `kind` at dt_b (a rollout repeats the standing commands: the plain steps or ticks)"""
    if kind in ("step_n_2", "step_n_1", "get_states+step_n_2", "rollout"):
        return [("step_n", dt_b, 10, 1)]
    if kind == "step":
        return [("step", dt_b)]
    if kind in ("tick_n", "rollout_ticks"):
        return [("tick_n", dt_b, 10, crash)]
    if kind == "step_range":
        return [("step_range", 0, n // 2, dt_b)]
    raise ValueError(kind)


def build_oracle(O, helpers, scene, airframe="x500", **kw):
    n = scene["n"]
    o = O.OracleSwarm(n)
    if "pos" in scene:  # (spawned at positions, heading 0, as the GPU test constructs its swarms)
        o.construct(0, n, helpers.oracle_params(airframe, **kw), scene["pos"], scene.get("heading", np.zeros(n)))
    else:
        o.construct(0, n, helpers.oracle_params(airframe, **kw))
    for nm in ("set_mixer_params", "set_rate_params", "set_attitude_params", "set_velocity_params", "set_position_params"):
        getattr(o, nm)(0, n)
    st = scene["st"]
    o.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    for first, count, mode, rows in scene.get("inputs", [(0, n, POSITION_CMD, scene.get("cmd"))]):
        o.set_input(first, count, mode, rows)
    return o


# ---- sequences of blocks, each at its own dt ---------------------------------------------------------------------------------------
def far_throttles(rng, n, k):
    """k + 1 sets of actuator commands, each far from the motor speeds the one before leaves behind: every UAV alternates between
    15-30 % and 75-90 % throttle (the motors start at 3000-5000 rpm, about half throttle).  A motor filter of the wrong dt shows in
    the block behind each of them, however long the block before it ran."""
    low_first = rng.uniform(size=(n, 1)) < 0.5
    out = []
    for j in range(k + 1):
        low, high = rng.uniform(0.15, 0.30, (n, 4)), rng.uniform(0.75, 0.90, (n, 4))
        out.append(np.where(low_first ^ bool(j % 2), low, high))
    return out


def oracle_block(o, n, blk):
    """one block of a sequence on an oracle swarm: {dt, and any of cmd (new actuator commands first), spin (new body rates first),
    ticks / steps}"""
    if blk.get("spin") is not None:
        s = o.get_state()
        o.set_state(0, n, s["x"], s["v"], s["R"], blk["spin"], s["motor_rpm"])
    if blk.get("cmd") is not None:
        o.set_input(0, n, ACTUATOR_CMD, blk["cmd"])
    if "ticks" in blk:
        oracle_call(o, n, ("tick_n", blk["dt"], blk["ticks"], False))
    if "steps" in blk:
        o.step_n(blk["dt"], blk["steps"])


def missed_changes(build, n, blocks):
    """For every block that runs at another dt than the block before it: the fraction of UAVs whose motor speeds after that block
    differ between the sequence as it is and the sequence in which that block keeps the dt of the block before (rpm_moved).
    build(): a fresh oracle swarm of the scene.  Returns [(block index, fraction)]."""
    out = []
    for i in range(1, len(blocks)):
        if blocks[i]["dt"] == blocks[i - 1]["dt"]:
            continue
        got = []
        for dt in (blocks[i]["dt"], blocks[i - 1]["dt"]):
            o = build()
            for blk in blocks[:i]:
                oracle_block(o, n, blk)
            oracle_block(o, n, dict(blocks[i], dt=dt))
            got.append(o.get_state()["motor_rpm"])
        out.append((i, rpm_moved(got[0], got[1])))
    return out


# two-stream runs: 1024 blocks, the smallest swarm whose runs are split over two streams; 16 steps are four launches of the fused run,
# the fewest that split, and leave the motors 0.16 s after their command: not yet converged when the second run starts
TWO_STREAM_N = 65_536
TWO_STREAM_STEPS = 16


def two_stream_scene():
    rng = np.random.default_rng(72)
    n = TWO_STREAM_N
    st = synthetic.random_state(rng, n, 4)
    return dict(n=n, st=st, pos=st["x"], inputs=[(0, n, ACTUATOR_CMD, far_throttles(rng, n, 0)[0])])


def two_stream_blocks():
    return [dict(dt=0.01, steps=TWO_STREAM_STEPS), dict(dt=0.004, steps=TWO_STREAM_STEPS)]


def sample_of(scene, count=256, seed=73):
    """(the scene of a random sample of UAVs with the first, the 64th and the last among them, their indices): the sampling of
    test_full_size_100k_sample_against_oracle.  One actuator input block over the whole swarm is assumed."""
    n = scene["n"]
    pick = np.sort(np.random.default_rng(seed).choice(n, count, replace=False))
    pick[:3] = [0, 63, n - 1]
    pick = np.unique(pick)
    (first, cnt, mode, rows), = scene["inputs"]
    sub = dict(n=len(pick), st={k: v[pick] for k, v in scene["st"].items()}, inputs=[(0, len(pick), mode, rows[pick])])
    if "pos" in scene:
        sub["pos"] = scene["pos"][pick]
    return sub, pick


# collision ticks at the shipped rates
def collision_scene():
    """1024 x500 at 64 m^3 per UAV, 100 touching pairs, velocities N(0, 6) m/s as in the neighbour-list parity test of
    tests/test_parity_gpu.py; new far throttles where the dt changes"""
    rng = np.random.default_rng(79)
    n = 1024
    side = (64.0 * n) ** (1.0 / 3.0)
    pos = rng.uniform(0, side, (n, 3)) + [0, 0, 50]
    pos[:100] = pos[100:200] + rng.normal(0, 0.35, (100, 3))
    st = synthetic.random_state(rng, n, 4, tilted=True)
    st["x"] = pos
    st["v"] = rng.normal(0, 6.0, (n, 3))
    cmds = far_throttles(rng, n, 2)
    # every body rate above 0.8 / (4 * 0.01) = 20 rad/s: the other side of the attitude condition of the displacement bound
    spin = rng.choice([-1.0, 1.0], (n, 3)) * rng.uniform(21.0, 30.0, (n, 3))
    blocks = []
    for j, dt in enumerate((0.01, 0.004)):
        blocks += [dict(dt=dt, ticks=25, cmd=cmds[j] if c == 0 else None) for c in range(4)]
    blocks.append(dict(dt=0.01, ticks=25, cmd=cmds[2], spin=spin))
    return dict(n=n, st=st, pos=pos, heading=rng.uniform(-3, 3, n), inputs=[(0, n, ACTUATOR_CMD, cmds[0])]), blocks


# sharded ticks
def sharded_scene():
    """2 x 512 UAVs in index shards at 64 m^3 per UAV, 5 m/s, with 100 touching pairs across the boundary; new far throttles at every dt"""
    rng = np.random.default_rng(1007)
    n = 1024
    side = (64.0 * n) ** (1.0 / 3.0)
    pos = rng.uniform(0, side, (n, 3)) + [0, 0, 30]
    pos[:100] = pos[512:612] + rng.normal(0, 0.3, (100, 3))
    st = synthetic.random_state(rng, n, 4, tilted=True)
    st["x"] = pos
    st["v"] = rng.normal(0, 5.0, (n, 3))
    cmds = far_throttles(rng, n, 2)
    blocks = [dict(dt=dt, ticks=20, cmd=cmds[j]) for j, dt in enumerate((0.001, 0.01, 0.004))]
    return dict(n=n, st=st, pos=pos, inputs=[(0, n, ACTUATOR_CMD, cmds[0])]), blocks


# three time steps behind one another, a stall in each call
THREE_DTS = (0.001, 0.01, 0.001, 0.01)


def three_step_blocks():
    """tick_n(0.001, 6), tick_n(0.01, 6), tick_n(0.001, 8), step_n(0.01, 4, 2) on stall_scene(0.001).  The runners cross half the skin in
    three ticks of 1 ms without passing the warning fraction first (runner_speed), and in every single tick of 10 ms: each call leaves a
    stall in the log whatever the timing of host and device, no search can be queued ahead of it."""
    return [dict(dt=0.001, ticks=STALL_TICKS), dict(dt=0.01, ticks=6), dict(dt=0.001, ticks=8), dict(dt=0.01, steps=4)]
