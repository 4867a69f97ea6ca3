"""Every stepping path at other time steps than the suite's 1 ms, and across dt changes (scenes and sequences: tests/time_steps.py;
their yardstick: tests/test_time_steps.py).  What depends on dt in the library: the motor-filter constants exp(-dt / tau) of the device
type table (re-uploaded when a call arrives with another dt, and when a stalled collision tick of an earlier dt is replayed), the PID
derivative (FAST multiplies by 1 / dt), the IMU's (v - v_prev) / dt, and dt as a launch argument of every kernel family.

Tolerances are the suite's own: LITERAL performs the reference's operations in the reference's order whatever dt is (RTOL_LITERAL),
FAST keeps RTOL_FAST after one step and RTOL_NORTH_STAR over a horizon.  The worst deviations seen are in MEASUREMENTS.md."""
import numpy as np
import pytest

import helpers
import time_steps as TS
from helpers import RTOL_FAST, RTOL_LITERAL, RTOL_NORTH_STAR, Pair, random_state
from test_components_gpu import rows_close
from test_parity_gpu import M, payload_for  # noqa: F401  (M: the fixture of the parity tests)
from test_run_fusion_gpu import assert_same

pytestmark = pytest.mark.gpu
DTS = TS.DTS
FLAVOURS = ["literal", "fast"]
OUT_FIELDS = ("position", "orientation", "velocity_body", "angular_velocity", "linear_acceleration", "range")


def arith_of(M, flavour):
    return M.ARITH_FAST if flavour == "fast" else M.ARITH_LITERAL


def tol1(flavour):
    return RTOL_FAST if flavour == "fast" else RTOL_LITERAL


def tolN(flavour):
    return RTOL_NORTH_STAR if flavour == "fast" else RTOL_LITERAL


def dt_id(dt):
    return f"{dt:.6g}"


def compare_outputs(p, rtol, what):
    """the publisher payload (the IMU's linear_acceleration divides by dt) against the oracle's: LITERAL at the 1e-12 of
    tests/test_outputs.py, FAST, whose payload is a function of a FAST state, at the state's own tolerance"""
    a, b = p.g.get_outputs(), p.o.get_outputs()
    worst = 0.0
    for k in OUT_FIELDS:
        worst = max(worst, helpers.assert_close(a[k], b[k], rtol, f"{what}: payload {k}"))
    return worst


# ---- 1. every input mode at every dt ------------------------------------------------------------------------------------------------
def mode_pair(M, O, mode, flavour, fleet, seed):
    """fleet: (airframe, count) runs; random near-upright states, payload_for per run"""
    rng = np.random.default_rng(seed)
    n = sum(c for _, c in fleet)
    p = Pair(M, n, arith=arith_of(M, flavour))
    first = 0
    for airframe, count in fleet:
        nm = M.AIRFRAMES[airframe]["n_motors"]
        p.construct(first, count, airframe)
        st = random_state(rng, count, nm, tilted=True)
        p.set_state(first, count, st)
        p.both("set_input", first, count, mode, payload_for(O, mode, rng, count, nm, st))
        first += count
    return p


def run_mode(p, mode, dt, flavour):
    what = f"mode {mode} dt {dt_id(dt)} {flavour}"
    p.step(dt)
    w1 = p.compare(tol1(flavour), what + " step 1")
    o1 = compare_outputs(p, 1e-12 if flavour == "literal" else tol1(flavour), what + " step 1")
    p.step(dt, 39)
    w40 = p.compare(tolN(flavour), what + " step 40")
    o40 = compare_outputs(p, 1e-12 if flavour == "literal" else tolN(flavour), what + " step 40")
    print(f"{what}: worst deviation from the oracle {w1:.2e} after 1 step, {w40:.2e} after 40; payload {o1:.2e}, {o40:.2e}")
    assert p.g.get_diag() == p.o.get_diag()


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("dt", DTS, ids=dt_id)
@pytest.mark.parametrize("mode", list(range(0, 11)))
def test_every_input_mode_at_every_dt(M, oracle, mode, dt, flavour):
    """128 each of x500, f550 and naki (two wavefronts per airframe, no mixed block): state, PID state, IMU, publisher payload and the
    diagnostics counters against the oracle after one step and after 40, at the constants test_every_input_mode and
    test_every_input_mode_fast_arithmetic use at 1 ms."""
    run_mode(mode_pair(M, oracle, mode, flavour, (("x500", 128), ("f550", 128), ("naki", 128)), 500 + mode), mode, dt, flavour)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("mode", list(range(0, 11)))
def test_every_input_mode_in_a_ragged_wavefront_with_an_inexact_reciprocal(M, oracle, mode, flavour):
    """67 UAVs at dt = 1/300: a wavefront of three lanes, and in FAST an inv_dt that is not the reciprocal's exact value"""
    run_mode(mode_pair(M, oracle, mode, flavour, (("x500", 67),), 600 + mode), mode, 1.0 / 300.0, flavour)


# ---- 2. plain runs at every dt ------------------------------------------------------------------------------------------------------
def model_swarms(M, O, n, flavour, seed, count):
    """`count` identical model-only swarms on actuator commands, with their start state and commands"""
    rng = np.random.default_rng(seed)
    st = random_state(rng, n, 4)
    act = rng.uniform(0.35, 0.60, (n, 4))
    out = []
    for _ in range(count):
        g = M.Swarm(n, arith=arith_of(M, flavour))
        g.construct(0, n, M.model_params("x500", ground_enabled=True, ground_z=0.0), st["x"], np.zeros(n))
        g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
        g.set_input(0, n, M.ACTUATOR_CMD, act)
        out.append(g)
    return out, st, act


def oracle_of(O, st, act, pick=None):
    pick = slice(None) if pick is None else pick
    n = len(st["x"][pick])
    o = O.OracleSwarm(n)
    o.construct(0, n, helpers.oracle_params("x500", ground_enabled=True, ground_z=0.0), st["x"][pick], np.zeros(n))
    o.set_state(0, n, st["x"][pick], st["v"][pick], st["R"][pick], st["omega"][pick], st["motor_rpm"][pick])
    o.set_input(0, n, O.ACTUATOR_CMD, act[pick])
    return o


def assert_follows(g, o, rtol, what, pick=None):
    a, b = g.get_state(), o.get_state()
    a["imu"], b["imu"] = g.get_imu(), o.get_imu()
    if pick is not None:
        a = {k: v[pick] for k, v in a.items()}
    worst = max(helpers.assert_close(a[k], b[k], rtol, f"{what}: {k}") for k in b)
    helpers.assert_close_per_uav(a, b, rtol, what)
    return worst


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("dt", DTS, ids=dt_id)
def test_plain_runs_at_every_dt(M, oracle, dt, flavour):
    """step_n(dt, 37, 1) — the fused-run family and its remainder launch — gives the bits of 37 step(dt) calls; step_n(dt, 36, 4) — the
    caller's own sub-steps — the bits of the first 36 of them; both follow the oracle"""
    n = 2048
    (run, singles, multi), st, act = model_swarms(M, oracle, n, flavour, 71, 3)
    multi.step_n(dt, 36, 4)
    for _ in range(36):
        singles.step(dt)
    if flavour == "literal":  # (test_substep_fusion_is_bit_identical demands bits of LITERAL)
        assert_same(multi, singles, f"36 steps in launches of 4, dt {dt_id(dt)} {flavour}")
    else:  # FAST: the compiler contracts each kernel instantiation as it likes, the *_multi kernels are another one (as in
        # test_pointer_addressed_kernels_match_buffer_addressed_ones: RTOL_FAST between two FAST instantiations)
        sa, sb = multi.get_state(), singles.get_state()
        for k in sa:
            helpers.assert_close(sa[k], sb[k], RTOL_FAST, f"36 steps in launches of 4, dt {dt_id(dt)}: {k}")
    singles.step(dt)
    run.step_n(dt, 37, 1)
    assert_same(run, singles, f"a run of 37 steps, dt {dt_id(dt)} {flavour}")
    o = oracle_of(oracle, st, act)
    o.step_n(dt, 36)
    w36 = assert_follows(multi, o, tolN(flavour), "36 steps in launches of 4")
    o.step(dt)
    w37 = assert_follows(run, o, tolN(flavour), "a run of 37 steps")
    print(f"plain runs dt {dt_id(dt)} {flavour}: worst deviation from the oracle {max(w36, w37):.2e}")


def scene_swarm(M, scene, flavour, **kw):
    """a product swarm of a scene of tests/time_steps.py, spawned where the scene says"""
    n = scene["n"]
    g = M.Swarm(n, arith=arith_of(M, flavour))
    g.construct(0, n, M.model_params("x500", **kw), scene.get("pos"), None if "pos" not in scene else scene.get("heading", np.zeros(n)))
    st = scene["st"]
    g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    for first, count, mode, rows in scene["inputs"]:
        g.set_input(first, count, mode, rows)
    return g


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_two_stream_runs_at_two_dt_back_to_back(M, oracle, flavour):
    """1024 blocks: the smallest swarm whose runs are split over two streams (split_stats counts the steps that were).  A run at 0.01
    directly followed by one at 0.004 — the second stream of the first run may still be at work when the table of the second is
    uploaded — gives the bits of a twin that synchronises in between, and follows the oracle on a 256-UAV sample (the sampling of
    test_full_size_100k_sample_against_oracle).  16 steps per run: the motors are still on their way to the far throttles of the scene
    when the dt changes (tests/test_time_steps.py holds the scene to that)."""
    scene = TS.two_stream_scene()
    k = TS.TWO_STREAM_STEPS
    (b0, b1) = TS.two_stream_blocks()
    assert (b0["dt"], b1["dt"], b0["steps"], b1["steps"]) == (0.01, 0.004, k, k)
    a, b = (scene_swarm(M, scene, flavour, ground_enabled=True, ground_z=0.0) for _ in range(2))
    a.step_n(0.01, k)
    assert a.split_stats()[0] == k, a.split_stats()
    a.step_n(0.004, k)
    assert a.split_stats()[0] == 2 * k, a.split_stats()
    b.step_n(0.01, k)
    b.synchronize()
    b.step_n(0.004, k)
    assert b.split_stats()[0] == 2 * k, b.split_stats()
    assert_same(a, b, f"two runs back to back, {flavour}")
    sub, pick = TS.sample_of(scene)
    o = TS.build_oracle(oracle, helpers, sub, ground_enabled=True, ground_z=0.0)
    for blk in (b0, b1):
        TS.oracle_block(o, sub["n"], blk)
    worst = assert_follows(a, o, tolN(flavour), "two-stream runs", pick)
    print(f"two-stream runs 0.01 -> 0.004 {flavour}: worst deviation from the oracle {worst:.2e}")


# ---- 3. dt changes on plain paths ---------------------------------------------------------------------------------------------------
def scene_pair(M, scene, flavour, **kw):
    n = scene["n"]
    p = Pair(M, n, arith=arith_of(M, flavour))
    p.construct(0, n, "x500", **kw)
    p.set_state(0, n, scene["st"])
    for first, count, mode, rows in scene.get("inputs", [(0, n, TS.POSITION_CMD, scene.get("cmd"))]):
        p.both("set_input", first, count, mode, rows)
    return p


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("a,b", TS.DT_PAIRS, ids=lambda v: dt_id(v))
def test_dt_changes_on_plain_paths(M, oracle, a, b, flavour):
    """step_n(a, 7), step(b), step_n(b, 9, 3), step_range(100, 200, 1/300), step_n(a, 5): every call with another dt than the one
    before it, through the fused run, the single step, the caller's sub-steps and the partial step"""
    scene = TS.plain_scene()
    p = scene_pair(M, scene, flavour)
    worst = 0.0
    for k, op in enumerate(TS.plain_ops(a, b)):
        TS.oracle_call(p.o, scene["n"], op)
        getattr(p.g, op[0])(*op[1:])
        worst = max(worst, p.compare(tolN(flavour), f"call {k} {op}"))
    assert p.g.get_diag() == p.o.get_diag()
    print(f"plain dt changes {dt_id(a)} -> {dt_id(b)} {flavour}: worst deviation from the oracle {worst:.2e}")


# ---- 4. dt changes with a non-empty launch log --------------------------------------------------------------------------------------
def second_call(M, g, kind, dt_b, scene, crash):
    n = scene["n"]
    if kind == "step_n_2":
        g.step_n(dt_b, 10, 2)
    elif kind == "step_n_1":
        g.step_n(dt_b, 10, 1)
    elif kind == "step":
        g.step(dt_b)
    elif kind == "tick_n":
        g.tick_n(dt_b, 10, True, crash, TS.REBOUNCE)
    elif kind == "step_range":
        g.step_range(0, n // 2, dt_b)
    elif kind == "get_states+step_n_2":
        g.get_states()
        g.step_n(dt_b, 10, 2)
    else:
        import torch
        from mrs_multirotor_simulator_amd import tensors as T
        cmd = torch.tensor(np.broadcast_to(scene["cmd"], (10, n, 4)).copy(), dtype=torch.float64, device=torch.device("cuda", g.device()))
        if kind == "rollout":
            T.rollout(g, M.POSITION_CMD, cmd, dt_b, groups=T.OBS_POS)
        else:
            T.rollout_ticks(g, M.POSITION_CMD, cmd, dt_b, crash, TS.REBOUNCE, groups=T.OBS_POS, crashed=False)


def compare_after_ticks(p, flavour, what):
    worst = p.compare(tolN(flavour), what)
    helpers.assert_close(p.g.get_external_force(), p.o.get_external_force(), 1e-12 if flavour == "literal" else RTOL_NORTH_STAR, f"{what}: forces")
    assert np.array_equal(p.g.has_crashed(), p.o.has_crashed()), f"{what}: crash flags"
    return worst


@pytest.mark.parametrize("crash", [False, True], ids=["elastic", "crash"])
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("kind", TS.SECOND_CALLS)
@pytest.mark.parametrize("a,b", TS.DT_PAIRS, ids=lambda v: dt_id(v))
def test_dt_changes_behind_a_stalled_launch_log(M, oracle, a, b, kind, flavour, crash):
    """tick_n(dt_a, 6) leaves a launch log in which the runners crossed half the skin two ticks before the end: the launches behind that
    one were no-ops, and it is the NEXT call — with dt_b — that finds the stall and replays them with dt_a, which sets the type table
    back to dt_a's motor-filter constants.  Whatever that call is, it must then step with dt_b's.  State, PID state, forces and crash
    flags against the oracle (step + handle_collisions per tick) after the second call; the counters, read only then, must show a stall
    and a replay.  (Whether the host saw the stall before the first call returned is a matter of timing: then the replay happened
    inside the first call, and the counters say the same.)"""
    scene = TS.stall_scene(a)
    p = scene_pair(M, scene, flavour, ground_enabled=True, ground_z=0.0)
    n = scene["n"]
    p.g.tick_n(a, TS.STALL_TICKS, True, crash, TS.REBOUNCE)
    second_call(M, p.g, kind, b, scene, crash)
    TS.oracle_call(p.o, n, ("tick_n", a, TS.STALL_TICKS, crash))
    for op in TS.second_call_ops(kind, b, n, crash):
        TS.oracle_call(p.o, n, op)
    worst = compare_after_ticks(p, flavour, f"{kind} at {dt_id(b)} behind ticks at {dt_id(a)}")
    fused, stalls, replayed, ahead = p.g.fused_stats()
    print(f"{kind} {dt_id(a)} -> {dt_id(b)} {flavour}: worst deviation {worst:.2e}; {fused} fused launches, {stalls} stalls, {replayed} replayed, {ahead} searches ahead")
    assert stalls >= 1 and replayed >= 1, (fused, stalls, replayed, ahead)


def gpu_block(g, n, blk):
    """one block of a sequence of tests/time_steps.py on a product swarm (TS.oracle_block is the oracle's side); the body rates of a
    `spin` block are set by the caller, on both sides from the oracle's state"""
    if blk.get("cmd") is not None:
        g.set_input(0, n, TS.ACTUATOR_CMD, blk["cmd"])
    if "ticks" in blk:
        g.tick_n(blk["dt"], blk["ticks"], True, False, TS.REBOUNCE)
    if "steps" in blk:
        g.step_n(blk["dt"], blk["steps"], 2)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_three_time_steps_with_a_stall_in_each_call(M, oracle, flavour):
    """0.001 -> 0.01 -> 0.001 in three tick_n calls, then step_n(0.01, 4, 2) (TS.three_step_blocks).  The runners cross half the skin in
    three ticks of 1 ms, under the warning fraction until they do, and in every tick of 10 ms: each call ends with a stall in its log
    that no search queued ahead can prevent, and the call behind it, at another dt, finds it."""
    scene = TS.stall_scene(TS.THREE_DTS[0])
    blocks = TS.three_step_blocks()
    assert tuple(b["dt"] for b in blocks) == TS.THREE_DTS
    p = scene_pair(M, scene, flavour, ground_enabled=True, ground_z=0.0)
    n = scene["n"]
    for blk in blocks:
        gpu_block(p.g, n, blk)
        TS.oracle_block(p.o, n, blk)
    worst = compare_after_ticks(p, flavour, "0.001 -> 0.01 -> 0.001 -> 0.01")
    fused, stalls, replayed, ahead = p.g.fused_stats()
    print(f"three time steps {flavour}: worst deviation {worst:.2e}; {fused} fused launches, {stalls} stalls, {replayed} replayed, {ahead} searches ahead")
    assert stalls >= 3 and replayed >= 1, (fused, stalls, replayed, ahead)


# ---- 5. collision ticks at the shipped rates ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_collision_ticks_at_the_shipped_rates(M, oracle, flavour):
    """TS.collision_scene: 1024 UAVs at 64 m^3 per UAV, 100 touching pairs, velocities N(0, 6) m/s as in the neighbour-list parity
    test: at 6 cm per tick the lists go stale every few ticks.  100 ticks at 0.01 s and 100 at 0.004 s in chunks of 25, new far throttles
    with each dt, forces and state against the oracle after every chunk; then a chunk at 0.01 s in which every UAV spins faster than
    0.8 / (4 * 0.01) = 20 rad/s, the other side of the attitude condition of the displacement bound."""
    scene, blocks = TS.collision_scene()
    n = scene["n"]
    p = Pair(M, n, arith=arith_of(M, flavour))
    p.construct(0, n, "x500", pos=scene["pos"], heading=scene["heading"])
    p.set_state(0, n, scene["st"])
    p.both("set_input", 0, n, oracle.ACTUATOR_CMD, scene["inputs"][0][3])
    touched, worst, ticks = 0, 0.0, 0
    for j, blk in enumerate(blocks):
        if blk.get("spin") is not None:
            s = p.o.get_state()
            p.g.set_state(0, n, s["x"], s["v"], s["R"], blk["spin"], s["motor_rpm"])
        TS.oracle_block(p.o, n, blk)
        gpu_block(p.g, n, blk)
        ticks += blk["ticks"]
        worst = max(worst, compare_after_ticks(p, flavour, f"chunk {j} (dt {dt_id(blk['dt'])}), {ticks} ticks"))
        touched = max(touched, int((np.abs(p.o.get_external_force()).sum(axis=1) > 0).sum()))
    assert touched >= 20, touched  # (of the 100 pairs set 0.35 m apart per axis, about a third are inside the 0.8 collision criterion)
    got_ticks, rebuilds = p.g.collision_stats()
    fused, stalls, replayed, ahead = p.g.fused_stats()
    print(f"collision ticks at the shipped rates {flavour}: worst deviation {worst:.2e}; {got_ticks} ticks, {rebuilds} searches, {fused} fused launches, "
          f"{stalls} stalls, {replayed} replayed, {ahead} searches ahead")
    assert got_ticks == ticks == 225 and rebuilds >= 10 and fused >= 1, (got_ticks, rebuilds, fused)


# ---- 6. rollouts at other dt ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("dt", DTS, ids=dt_id)
def test_rollouts_equal_the_host_loop_at_every_dt(M, oracle, dt, flavour):
    """24 steps with a command block held for 4: tensors.rollout against set_input / step_n(dt, 4) / gather, tensors.rollout_ticks against
    set_input / tick_n(dt, 1) with the rows taken between step and collision pass.  LITERAL: bit for bit, as the rollout tests demand at
    1 ms; FAST: RTOL_FAST against the loop, as test_fast_tracks_the_loop_and_itself allows."""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, blocks, hold = 256, 6, 4
    rng = np.random.default_rng(91)
    st = random_state(rng, n, 4, box=6.0, zlo=20.0, zhi=30.0, tilted=True)  # 256 UAVs in 12 x 12 x 10 m: some touch
    goal = np.concatenate([st["x"][None] + rng.uniform(-3, 3, (blocks, n, 3)), rng.uniform(-3, 3, (blocks, n, 1))], axis=2)

    def make():
        g = M.Swarm(n, arith=arith_of(M, flavour))
        g.construct(0, n, M.model_params("x500", ground_enabled=True, ground_z=0.0), st["x"], np.zeros(n))
        g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
        g.set_input(0, n, M.POSITION_CMD, goal[0])
        return g

    def close(got, want, what):
        if flavour == "literal":
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"{what}: rows differ"
        else:
            helpers.assert_close(got, want, RTOL_FAST, what)

    def same_state(a, b, what):
        if flavour == "literal":
            assert_same(a, b, what)
        else:
            sa, sb = a.get_state(), b.get_state()
            for k in sa:
                helpers.assert_close(sa[k], sb[k], RTOL_FAST, f"{what}: {k}")

    a, b = make(), make()
    dev = torch.device("cuda", a.device())
    cmd = torch.tensor(goal, dtype=torch.float64, device=dev)
    want = torch.empty((blocks, n, T.gather_width(T.OBS_ALL)), dtype=torch.float64, device=dev)
    for j in range(blocks):
        T.set_input(a, M.POSITION_CMD, cmd[j])
        a.step_n(dt, hold)
        T.gather(a, T.OBS_ALL, 0, n, out=want[j])
    got = T.rollout(b, M.POSITION_CMD, cmd, dt, T.OBS_ALL, hold=hold)
    close(got.cpu().numpy(), want.cpu().numpy(), f"rollout dt {dt_id(dt)}")
    same_state(b, a, f"rollout dt {dt_id(dt)}")

    # rollout_cost: the restatement of its sum on the rollout's own FP64 rows, bit for bit in both flavours (test_rollout_cost_gpu.py)
    from test_rollout_cost_gpu import assert_cost, restate
    c = make()
    w = T.gather_width(T.OBS_ALL)
    tg = torch.tensor(rng.normal(0.0, 2.0, (blocks, n, w)), dtype=torch.float64, device=dev)
    wt = rng.uniform(0.1, 2.0, (blocks, w))
    wt[-1] *= 10.0
    wt = torch.tensor(wt, dtype=torch.float64, device=dev)
    cost = T.rollout_cost(c, M.POSITION_CMD, cmd, dt, T.OBS_ALL, tg, wt, hold=hold)
    assert_cost(cost, restate(got.cpu().numpy(), tg.cpu().numpy(), wt.cpu().numpy()), f"rollout_cost dt {dt_id(dt)}")
    assert_same(c, b, f"rollout_cost dt {dt_id(dt)}: state")

    a, b = make(), make()
    wantc = torch.empty((blocks, n), dtype=torch.bool, device=dev)
    for j in range(blocks):
        T.set_input(a, M.POSITION_CMD, cmd[j])
        for t in range(hold):
            a.step_n(dt, 1)
            if t == hold - 1:
                T.gather(a, T.OBS_ALL, 0, n, out=want[j])
                T.crashed(a, out=wantc[j])
            a.handle_collisions(True, True, TS.REBOUNCE)
    got, gotc = T.rollout_ticks(b, M.POSITION_CMD, cmd, dt, True, TS.REBOUNCE, T.OBS_ALL, hold=hold)
    close(got.cpu().numpy(), want.cpu().numpy(), f"rollout_ticks dt {dt_id(dt)}")
    assert np.array_equal(gotc.cpu().numpy(), wantc.cpu().numpy()) and wantc.any().item(), "crash rows"
    same_state(b, a, f"rollout_ticks dt {dt_id(dt)}")


# ---- 8. refusals and the edge of the domain -----------------------------------------------------------------------------------------
def small_pair(M, O, n, flavour="literal", seed=5):
    rng = np.random.default_rng(seed)
    p = Pair(M, n, arith=arith_of(M, flavour))
    p.construct(0, n, "x500", ground_enabled=True, ground_z=0.0)
    st = random_state(rng, n, 4, tilted=True)
    p.set_state(0, n, st)
    p.cmd = payload_for(O, O.POSITION_CMD, rng, n, 4, st)
    p.both("set_input", 0, n, O.POSITION_CMD, p.cmd)
    return p, st, rng


def every_column(g):
    a = g.get_states()
    out = {f: a[f].copy() for f in a.dtype.names}
    out["pid"], out["imu"], out["fext"], out["crashed"] = g.get_pid(), g.get_imu(), g.get_external_force(), g.has_crashed()
    return out


BAD_DT = [0.0, -0.001, float("nan")]
REFUSED_CALLS = {
    "step": lambda g, dt: g.step(dt),
    "step_n": lambda g, dt: g.step_n(dt, 3, 1),
    "tick_n": lambda g, dt: g.tick_n(dt, 3, True, False, TS.REBOUNCE),
    "step_range": lambda g, dt: g.step_range(10, 30, dt),
    "debug_component": lambda g, dt: g.debug_component(10, 0, 64, np.zeros((64, 4)), dt),  # COMP_RATE
}


@pytest.mark.parametrize("dt", BAD_DT, ids=["zero", "negative", "nan"])
@pytest.mark.parametrize("call", sorted(REFUSED_CALLS))
def test_a_dt_outside_the_domain_is_refused_and_changes_nothing(M, oracle, call, dt):
    """MRS_ERR_ARG ("error 1") and every state column byte for byte what it was"""
    p, _, _ = small_pair(M, oracle, 64)
    assert M.swarm.COMP_RATE == 10
    p.g.step_n(0.01, 2)
    before = every_column(p.g)
    with pytest.raises(M.MrsError, match="error 1"):
        REFUSED_CALLS[call](p.g, dt)
    after = every_column(p.g)
    for k in before:
        assert np.array_equal(np.ascontiguousarray(before[k]).view(np.uint8), np.ascontiguousarray(after[k]).view(np.uint8)), k


def test_an_infinite_dt_steps_like_the_oracle(M, oracle):
    """dt = +inf passes the `dt > 0` check of the step calls.  One plain step of 64 UAVs against the oracle: exp(-inf / tau) = 0 puts
    the motors on their commands at once, the integrator's non-finite state is rolled back like any other."""
    p, _, _ = small_pair(M, oracle, 64)
    p.step(float("inf"))
    p.compare(RTOL_LITERAL, "one step of dt = +inf")
    assert p.g.get_diag() == p.o.get_diag()


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_component_probe_at_another_dt_and_behind_a_run_at_a_third(M, oracle, flavour):
    """debug_component of the rate and position controllers at dt = 0.01 (the PID derivative and integral use the probe's own dt), with
    the tolerances of test_position_velocity_and_rate_controllers_keep_their_pid_state; then the same right behind a run at 0.004, whose
    type table the probe keeps: no probed component reads the motor-filter constants."""
    n = 256
    p, st, rng = small_pair(M, oracle, n, flavour, seed=6)
    tol = 1e-9 if flavour == "fast" else 1e-13

    def probe(what):
        for call in range(3):
            rows = st["x"] + rng.normal(0, 50.0 if call % 2 else 1.0, (n, 3))
            rows_close(p.g.debug_component(M.swarm.COMP_POSITION, 0, n, rows, 0.01), p.o.debug_component(M.swarm.COMP_POSITION, 0, n, rows, 0.01), tol,
                       f"{what}: position controller call {call}")
            rows = np.concatenate([rng.normal(0, 5.0, (n, 3)), rng.uniform(0, 1, (n, 1))], axis=1)
            rows_close(p.g.debug_component(M.swarm.COMP_RATE, 0, n, rows, 0.01), p.o.debug_component(M.swarm.COMP_RATE, 0, n, rows, 0.01), tol,
                       f"{what}: rate controller call {call}")
            helpers.assert_close(p.g.get_pid(), p.o.get_pid(), tol, f"{what}: PID state after call {call}")

    probe("fresh swarm")
    # (the oracle's probe leaves its input rows behind as the UAV's reference, the library's does not: the command once more, to both)
    p.both("set_input", 0, n, oracle.POSITION_CMD, p.cmd)
    p.step(0.004, 5)
    p.compare(tolN(flavour), "the run at 0.004")
    # (the probes compare at 1e-13 / 1e-9: both sides start them from the same bits, the oracle's)
    p.set_state(0, n, p.o.get_state())
    p.both("set_pid", 0, n, p.o.get_pid())
    probe("behind a run at 0.004")
    p.both("set_input", 0, n, oracle.POSITION_CMD, p.cmd)
    p.step(0.004, 1)  # ... and the probe left the table to the run: one more step of it
    p.compare(tolN(flavour), "a step behind the probes")


# ---- 7. sharded tick across a dt change ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_sharded_ticks_across_dt_changes(M, oracle, flavour):
    """TS.sharded_scene: two loopback ranks in one process (index shards of 512 UAVs, 100 touching pairs across the boundary), 20 sharded
    ticks at 0.001, 20 at 0.01, 20 at 0.004, new far throttles with each dt, against one unsharded swarm and the oracle at the
    constants of test_export_sets_gpu.py.  The announcements of a call's last launches assumed its dt, so the first tick of a call with
    another dt must take the search path: every rank's search counter (comm_info) goes up by one in the first tick of each block.  The
    control is in the first block: a second call of one tick at the same 1 ms, one tick behind that search, must leave the counters
    alone, so a call boundary by itself is not what searches.  The later blocks cannot hold that control: over the horizon of four ticks
    of 10 or 4 ms the displacement bound (mrs_may_leave: 21 m/s, 100 m/s^2 per listed partner) announces the fastest UAVs as about to
    leave their skin, and a search one tick behind a search is the library's ordinary answer there.  Shards of eight blocks stay in
    the serial form of the tick: the split form, whose announcements the rule protects, needs swarms far beyond a quick test, so
    split_stats has nothing to show here."""
    from test_export_sets_gpu import VirtualShards, run_ranks
    scene, blocks = TS.sharded_scene()
    n, st, pos = scene["n"], scene["st"], scene["pos"]
    cmd0 = scene["inputs"][0][3]
    pp = helpers.to_product_params(M, helpers.oracle_params("x500", ground_enabled=True, ground_z=0.0))
    o = TS.build_oracle(oracle, helpers, scene, ground_enabled=True, ground_z=0.0)
    one = scene_swarm(M, scene, flavour, ground_enabled=True, ground_z=0.0)
    vs = VirtualShards(M, 2, np.arange(n), pp, pos, np.zeros(n), st, M.ACTUATOR_CMD, cmd0, arith_of(M, flavour), M.EXCHANGE_EXPORT_SETS)
    tol, ftol = tolN(flavour), (1e-11 if flavour == "literal" else RTOL_NORTH_STAR)

    def sharded(dt, k):
        run_ranks([(lambda g=g: g.tick_sharded_n(dt, k, True, False, TS.REBOUNCE)) for g, _ in vs.shards])

    def searches():
        return [ci["searches"] for ci in vs.info()]

    worst, touched = 0.0, 0
    for blk in blocks:
        dt = blk["dt"]
        for g, idx in vs.shards:
            g.set_input(0, len(idx), M.ACTUATOR_CMD, blk["cmd"][idx])
        s0 = searches()
        sharded(dt, 1)
        s1 = searches()
        assert s1 == [x + 1 for x in s0], f"dt {dt_id(dt)}: searches {s0} -> {s1}: the first tick behind the change did not search"
        rest = blk["ticks"] - 1
        if dt == 0.001:
            sharded(dt, 1)
            assert searches() == s1, f"dt {dt_id(dt)}: searches {s1} -> {searches()}: a new call at the same dt searched"
            rest -= 1
        sharded(dt, rest)
        gpu_block(one, n, blk)
        TS.oracle_block(o, n, blk)
        a, so, fo = vs.gather(), o.get_state(), o.get_external_force()
        sg, fg = one.get_state(), one.get_external_force()
        assert np.array_equal(a["crashed"], o.has_crashed())
        helpers.assert_close(a["f"], fo, ftol, f"forces after the ticks at {dt_id(dt)}")
        helpers.assert_close(a["f"], fg, ftol, f"forces, shards against one swarm, after the ticks at {dt_id(dt)}")
        for k in ("x", "v", "R", "omega", "motor_rpm"):
            worst = max(worst, helpers.assert_close(a[k], so[k], tol, f"{k} after the ticks at {dt_id(dt)}"))
            helpers.assert_close(a[k], sg[k], tol, f"{k}: shards against one swarm after the ticks at {dt_id(dt)}")
        helpers.assert_close_per_uav(a, so, tol, f"after the ticks at {dt_id(dt)}")
        touched = max(touched, int((np.abs(fo).sum(axis=1) > 0).sum()))
    assert touched >= 20, touched
    print(f"sharded ticks 0.001 -> 0.01 -> 0.004 {flavour}: worst deviation from the oracle {worst:.2e}; rank 0: {vs.info()[0]}")
    vs.close()
