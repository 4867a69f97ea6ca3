"""Control-rate rollouts on the GPU (include/mrs_swarm.h, "control-rate rollouts"; tensors.rollout(hold=, obs_every=)): command row block j
is held for `hold` steps and an observation row block is written every `obs_every` steps.  On the variant-test swarm of
test_rollout_gpu.py (three airframes, mixed-airframe blocks, a ragged tail, held, crashed and NaN-rollback UAVs):

* nothing but the due rows is written (sentinel-filled slack behind and between the rows) — checked before any test hands the library an
  exactly sized buffer;
* in LITERAL a rate rollout equals the decimated set_input / step_n / gather loop of the ABI comment bit for bit (rows, state, PID, IMU,
  external force, crash flags, diag) in all 11 modes, FP64 and FP32, with block boundaries inside and across launches, a launch that reads
  no command row, and one terminal row block;
* in both flavours it equals the plain rollout on repeat_interleave'd commands, decimated, bit for bit; FAST tracks the FAST loop within
  the tolerances of test_rollout_gpu.test_fast_tracks_the_loop_and_itself and is bit-identical to itself split into single blocks;
* held UAVs report their unchanged state once per observation block and the command columns are left holding the last row block;
* refused calls change nothing, and the exactly sized decimated buffers are accepted;
* it follows the CPU oracle with each command held; an MPPI fork at hold = 10 reproduces the source UAV's own continuation; the
  pointer-addressed kernels (child process), the caller-stream fence and the C++ facade (tests/cpp/rollout_rate_test.cpp) agree.

All comparisons are bit for bit except the two against other arithmetic (the oracle: RTOL_LITERAL; the FAST loop: RTOL_FAST after one
step, RTOL_NORTH_STAR after the run), which sit exactly where test_rollout_gpu uses them."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import helpers
import test_rollout_gpu as R
from helpers import RTOL_FAST, RTOL_LITERAL, RTOL_NORTH_STAR
from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_rollout_gpu import COUNT, FIRST, LAUNCH_CAP, _hip_malloc, assert_same_state, commands, loop, same, variant_swarm
from test_step_variants_gpu import N_SINGLE

pytestmark = pytest.mark.gpu
DT = R.DT
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 300
SENTINEL = -1234.5  # (exact in FP32 and FP64)

# (hold, obs_every, steps).  132 = 2 * LAUNCH_CAP + 4: command and observation blocks straddle both launch boundaries; hold 70 >
# LAUNCH_CAP: the second launch reads no command row; (5, 130, 130): one terminal row block
RATES = ((1, 1, 5), (4, 4, 8), (3, 6, 132), (10, 5, 70), (70, 140, 140), (5, 130, 130))
assert all(s % h == 0 and s % o == 0 for h, o, s in RATES) and 70 > LAUNCH_CAP and 132 == 2 * LAUNCH_CAP + 4

# which test forces each entry point of rollout_rate_device.inc (both flavours; test_rollout_rate.py keeps the table complete).  A call with
# hold == obs_every == 1 runs the kernels of rollout_device.inc (test_rollout_gpu.ROLLOUT_KERNELS)
ROLLOUT_RATE_KERNELS = {
    "mrs_uav_rollout_rate": ("test_pointer_form",),
    "mrs_uav_rollout_rate_buf": ("test_literal_equals_the_decimated_loop[cascade]", "test_equals_the_plain_rollout[cascade-FAST]"),
    "mrs_uav_model_rollout_rate": ("test_pointer_form",),
    "mrs_uav_model_rollout_rate_buf": ("test_literal_equals_the_decimated_loop[model]", "test_mppi_fork_at_a_control_rate[ACTUATOR_CMD]"),
    "mrs_uav_rollout_rate_mixed": ("test_literal_equals_the_decimated_loop[cascade]",),
}

_sentinel = []  # the outcome of sentinel_check(), once: None (passed) or the failure


def rate_loop(g, mode, cmd, groups, first, out_dtype, hold, every):
    """the loop of the ABI comment of mrs_swarm_rollout_rate_device, through tensors"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    steps, count = cmd.shape[0] * hold, cmd.shape[1]
    out = torch.empty((steps // every, count, T.gather_width(groups)), dtype=out_dtype, device=cmd.device) if groups else None
    for t in range(steps):
        if t % hold == 0:
            T.set_input(g, mode, cmd[t // hold], first)
        g.step_n(DT, 1)
        if groups and (t + 1) % every == 0:
            T.gather(g, groups, first, count, out=out[(t + 1) // every - 1])
    return out


def raw_equal(a, b):
    """two tensors / arrays of one dtype hold the same bits"""
    a, b = (np.ascontiguousarray(v.cpu().numpy() if hasattr(v, "cpu") else v) for v in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def sentinel_check(mrs):
    """rows and commands are views into larger sentinel-filled tensors: padded row strides, and behind the last due row block as many
    blocks as a kernel that still wrote (or read) a row per step would touch.  Every sentinel element is unchanged afterwards, the due
    rows are the loop's."""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(71)
    for scen, mode, dtype, pad in (("cascade", O.VELOCITY_HDG_CMD, torch.float32, 3), ("cascade", O.ATTITUDE_CMD, torch.float64, 2),
                                   ("model", O.ACTUATOR_CMD, torch.float32, 0)):  # (ACTUATOR rows are dense: no column padding)
        for hold, every, steps in ((4, 4, 8), (3, 6, 132), (10, 5, 70), (5, 130, 130)):
            a, b = variant_swarm(mrs, scen, mrs.ARITH_LITERAL), variant_swarm(mrs, scen, mrs.ARITH_LITERAL)
            dev = torch_dev(a)
            B, due, ow = steps // hold, steps // every, T.gather_width(T.OBS_ALL)
            c = torch.tensor(commands(mode, rng, B, COUNT, a.get_states(FIRST, COUNT)["x"]), dtype=dtype, device=dev)
            # commands: B due blocks, then the blocks a per-step reader would run into; `pad` sentinel columns in every row
            cmd_big = torch.full((steps + 1, COUNT, c.shape[2] + pad), SENTINEL, dtype=dtype, device=dev)
            cmd_big[:B, :, :c.shape[2]] = c
            cmd_ref = cmd_big.clone()
            # rows: `due` blocks, then (every - 1) * due blocks of slack and one more; sentinel columns behind every row's width
            obs_big = torch.full((steps + 1, COUNT, ow + 5), SENTINEL, dtype=dtype, device=dev)
            want = rate_loop(a, mode, c, T.OBS_ALL, FIRST, dtype, hold, every)
            got = T.rollout(b, mode, cmd_big[:B], DT, T.OBS_ALL, first=FIRST, out=obs_big[:due], hold=hold, obs_every=every)
            torch.cuda.synchronize(dev)
            what = f"{scen} mode {mode} {dtype} hold {hold} obs_every {every} steps {steps}"
            assert got.shape == (due, COUNT, ow) and got.data_ptr() == obs_big.data_ptr()
            assert raw_equal(cmd_big, cmd_ref), f"{what}: the command tensor was written"
            assert bool((obs_big[due:] == SENTINEL).all()), f"{what}: rows behind the last due row block were written"
            assert bool((obs_big[:due, :, ow:] == SENTINEL).all()), f"{what}: elements past a row's width were written"
            assert raw_equal(got, want), f"{what}: the due rows are not the loop's"
            assert_same_state(a, b, what)


def require_sentinel(mrs):
    """before the library is handed an exactly sized buffer: the sentinel check has run (here, if no test ran it yet) and passed"""
    if not _sentinel:
        try:
            sentinel_check(mrs)
            _sentinel.append(None)
        except BaseException as e:  # noqa: B902 (the outcome is kept for every later caller)
            _sentinel.append(e)
            raise
    if _sentinel[0] is not None:
        pytest.fail(f"the sentinel check failed ({_sentinel[0]!r}): no exactly sized buffer is handed to the library")


def test_nothing_outside_the_rows_is_written(mrs):
    require_sentinel(mrs)


@pytest.mark.parametrize("scen", ["cascade", "model"])
def test_literal_equals_the_decimated_loop(mrs, scen):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, b = variant_swarm(mrs, scen, mrs.ARITH_LITERAL), variant_swarm(mrs, scen, mrs.ARITH_LITERAL)
    assert np.asarray(a.has_crashed()).any(), "the scenario has crashed UAVs"
    dev = torch_dev(a)
    rng = np.random.default_rng(73)
    modes = range(11) if scen == "cascade" else (O.ACTUATOR_CMD, O.INPUT_UNKNOWN, O.ACTUATOR_CMD)
    for dtype in (torch.float64, torch.float32):
        for mode in modes:
            for hold, every, steps in RATES:
                x = a.get_states(FIRST, COUNT)["x"]
                cmd = torch.tensor(commands(mode, rng, steps // hold, COUNT, x), dtype=dtype, device=dev)
                want = rate_loop(a, mode, cmd, T.OBS_ALL, FIRST, dtype, hold, every)
                got = T.rollout(b, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every)
                what = f"{dtype} mode {mode} hold {hold} obs_every {every} steps {steps}"
                assert got.shape == (steps // every, COUNT, T.gather_width(T.OBS_ALL)), what
                w, gt = want.cpu().numpy(), got.cpu().numpy()
                assert np.array_equal(w.view(np.uint8), gt.view(np.uint8)), f"{what}: observation rows differ at {np.argwhere(w != gt)[:5]}"
                assert_same_state(a, b, what)
    # the non-finite velocities of the scenario took the NaN-rollback path in both, as often; the other counters agree too
    assert b.get_diag() == a.get_diag() and b.get_diag()["nan_rollback"] > 0


@pytest.mark.parametrize("arith", ["FAST", "LITERAL"])
@pytest.mark.parametrize("scen", ["cascade", "model"])
def test_equals_the_plain_rollout(mrs, scen, arith):
    """rollout(cmd, hold=C, obs_every=O) == rollout(cmd.repeat_interleave(C, 0))[O-1::O] on a twin, rows and final state, bit for bit"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ar = getattr(mrs, "ARITH_" + arith)
    a, b = variant_swarm(mrs, scen, ar), variant_swarm(mrs, scen, ar)
    dev = torch_dev(a)
    rng = np.random.default_rng(79)
    modes = (O.ATTITUDE_RATE_CMD, O.POSITION_CMD, O.ACTUATOR_CMD) if scen == "cascade" else (O.ACTUATOR_CMD,)
    for dtype in (torch.float64, torch.float32):
        for mode in modes:
            for hold, every, steps in RATES[1:]:
                x = a.get_states(FIRST, COUNT)["x"]
                cmd = torch.tensor(commands(mode, rng, steps // hold, COUNT, x), dtype=dtype, device=dev)
                want = T.rollout(a, mode, cmd.repeat_interleave(hold, 0), DT, T.OBS_ALL, first=FIRST)[every - 1::every]
                got = T.rollout(b, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every)
                what = f"{arith} {scen} {dtype} mode {mode} hold {hold} obs_every {every} steps {steps}"
                assert raw_equal(got, want), f"{what}: rows differ from the plain rollout's"
                assert_same_state(a, b, what)


def test_fast_tracks_the_loop_and_its_splits(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    loop_g = variant_swarm(mrs, "cascade", mrs.ARITH_FAST)
    one, split = variant_swarm(mrs, "cascade", mrs.ARITH_FAST), variant_swarm(mrs, "cascade", mrs.ARITH_FAST)
    dev = torch_dev(one)
    rng = np.random.default_rng(83)
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_ROT
    # against the FAST loop: 6 commands held for 4 steps, a row per step — the first row is the state after ONE step (RTOL_FAST), the
    # last after the run of 24 steps (RTOL_NORTH_STAR), over the UAVs whose rows are finite in the loop
    hold, B = 4, 6
    cmd = torch.tensor(commands(O.ATTITUDE_RATE_CMD, rng, B, COUNT, None), dtype=torch.float64, device=dev)
    want = rate_loop(loop_g, O.ATTITUDE_RATE_CMD, cmd, groups, FIRST, torch.float64, hold, 1).cpu().numpy()
    got = T.rollout(one, O.ATTITUDE_RATE_CMD, cmd, DT, groups, first=FIRST, hold=hold, obs_every=1).cpu().numpy()
    assert got.shape == want.shape == (24, COUNT, 15)
    ok = np.isfinite(want).all(axis=(0, 2))
    helpers.assert_close(got[0][ok], want[0][ok], RTOL_FAST, "FAST rate rollout vs loop after one step")
    helpers.assert_close(got[-1][ok], want[-1][ok], RTOL_NORTH_STAR, "FAST rate rollout vs loop after the run")
    T.rollout(split, O.ATTITUDE_RATE_CMD, cmd, DT, groups, first=FIRST, hold=hold, obs_every=1)
    # one call of B blocks == B calls of one block each, bit for bit (blocks of 10 steps, two row blocks each; 70 steps: two launches)
    hold, every, B = 10, 5, 7
    cmd = torch.tensor(commands(O.ATTITUDE_RATE_CMD, rng, B, COUNT, None), dtype=torch.float64, device=dev)
    whole = T.rollout(one, O.ATTITUDE_RATE_CMD, cmd, DT, groups, first=FIRST, hold=hold, obs_every=every)
    parts = [T.rollout(split, O.ATTITUDE_RATE_CMD, cmd[j:j + 1], DT, groups, first=FIRST, hold=hold, obs_every=every) for j in range(B)]
    assert whole.shape == (14, COUNT, 15) and all(p.shape == (2, COUNT, 15) for p in parts)
    assert raw_equal(torch.cat(parts), whole), "FAST: one call of B blocks vs B calls of one block"
    assert_same_state(one, split, "FAST: one call of B blocks vs B calls of one block")
    # the last row block is gather_device of the final state
    last = T.rollout(one, O.ATTITUDE_RATE_CMD, cmd[:2], DT, T.OBS_ALL, first=FIRST, hold=3, obs_every=6)
    assert last.shape[0] == 1 and same(last[0].cpu().numpy(), T.gather(one, T.OBS_ALL, FIRST, COUNT, dtype=torch.float64).cpu().numpy())


def test_held_uavs_and_the_command_left_behind(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, b = variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL), variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL)
    dev = torch_dev(a)
    rng = np.random.default_rng(89)
    held = slice(1950 - FIRST, 1953 - FIRST)  # variant_swarm: set_hold(1950, 3) inside the range, set_hold(100, 2) outside
    for mode, hold, every, steps in ((O.VELOCITY_HDG_CMD, 3, 6, 132), (O.ATTITUDE_RATE_CMD, 70, 35, 140), (O.POSITION_CMD, 10, 5, 70)):
        before = T.gather(b, T.OBS_ALL, 1950, 3, dtype=torch.float64).cpu().numpy()
        outside = T.gather(b, T.OBS_ALL, 100, 2, dtype=torch.float64).cpu().numpy()
        cmd = torch.tensor(commands(mode, rng, steps // hold, COUNT, a.get_states(FIRST, COUNT)["x"]), device=dev)
        want = rate_loop(a, mode, cmd, T.OBS_ALL, FIRST, torch.float64, hold, every).cpu().numpy()
        got = T.rollout(b, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every).cpu().numpy()
        assert got.shape[0] == steps // every and same(got, want)
        for j in range(steps // every):
            assert same(got[j, held], before), f"mode {mode}: row block {j} of the held UAVs is not their unchanged state"
        assert same(T.gather(b, T.OBS_ALL, 100, 2, dtype=torch.float64).cpu().numpy(), outside), "a held UAV outside the range moved"
        # the moving UAVs did move between two row blocks
        assert not same(got[0], got[-1])
    # released, the held UAVs fly on the LAST command row block in both
    for g in (a, b):
        g.set_hold(1950, 3, False)
        g.set_hold(100, 2, False)
        g.step_n(DT, 3)
    assert_same_state(a, b, "after the hold was released")
    assert not same(T.gather(b, T.OBS_ALL, 1950, 3, dtype=torch.float64).cpu().numpy(), before), "the released UAVs moved"


def test_refused_calls_change_nothing(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL)
    dev = torch_dev(g)
    before = T.save(g).cpu().numpy()
    # 12 steps of 100 UAVs: 4 command row blocks of 10 FP64 (held for 3 steps), 3 observation row blocks of 36 FP64 (every 4 steps)
    hip, cmd = _hip_malloc(4 * 100 * 10 * 8)
    _, obs = _hip_malloc(3 * 100 * 36 * 8)
    _, obs_short = _hip_malloc((3 * 100 - 1) * 36 * 8)  # one row short of the decimated size
    _, cmd_short = _hip_malloc((4 * 100 - 1) * 10 * 8)
    bufs = (cmd, obs, obs_short, cmd_short)
    ok = dict(first=0, count=100, mode=O.POSITION_CMD, dt=DT, n_steps=12, cmd_every=3, obs_every=4, dev_cmd=cmd, dtype=T.DTYPE_F64, cmd_stride=10,
              groups=T.OBS_ALL, dev_obs=obs, obs_stride=36, ext_stream=None)
    bad = [({"cmd_every": 0}, 1), ({"cmd_every": -1}, 1), ({"obs_every": 0}, 1), ({"obs_every": -1}, 1), ({"cmd_every": 5}, 1), ({"obs_every": 5}, 1),
           ({"cmd_every": 24}, 1), ({"obs_every": 24}, 1), ({"dev_obs": obs_short}, 1), ({"dev_cmd": cmd_short}, 1), ({"dev_obs": None}, 1),
           ({"dev_cmd": None}, 1), ({"cmd_every": 2}, 1), ({"obs_every": 3}, 1), ({"obs_every": 1}, 1), ({"n_steps": 24}, 1), ({"n_steps": 0}, 1),
           ({"first": N_SINGLE - 5}, 3), ({"count": -1}, 3), ({"mode": 11}, 1), ({"dtype": 2}, 1), ({"dt": 0.0}, 1), ({"cmd_stride": 3}, 1),
           ({"groups": 0x100}, 1), ({"obs_stride": 35}, 1)]  # (cmd_every 2 / obs_every 3 or 1 / n_steps 24: more row blocks than the buffers hold)
    for change, code in bad:
        with pytest.raises(mrs.MrsError, match=f"error {code}:"):
            g.rollout_rate_device(**dict(ok, **change))
        assert np.array_equal(T.save(g).cpu().numpy(), before), change
    back = np.zeros(3 * 100 * 36)
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(obs), back.nbytes, 2) == 0
    assert not back.any(), "a refused call wrote observation rows"
    # a sharded swarm refuses the call, state and rows untouched
    group = mrs.LoopbackGroup(2)
    shards = []
    for r in range(2):
        s = mrs.Swarm(100)
        s.construct(0, 100, mrs.model_params("x500"), np.stack([np.arange(100) * 3.0 + 400 * r, np.zeros(100), np.full(100, 5.0)], axis=1))
        s.comm_init_loopback(group, r, 200)
        shards.append(s)
    tc = torch.zeros((2, 100, 4), dtype=torch.float64, device=dev)
    to = torch.zeros((1, 100, 10), dtype=torch.float64, device=dev)
    for s in shards:
        x = s.get_states()["x"]
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.rollout(s, O.POSITION_CMD, tc, DT, out=to, hold=4, obs_every=8)
        assert same(s.get_states()["x"], x)
    assert not to.any()
    for s in shards:
        s.close()
    group.close()
    # the exactly sized buffers are accepted — once the sentinel check has shown that nothing is written outside the due rows
    require_sentinel(mrs)
    g.rollout_rate_device(**ok)
    torch.cuda.synchronize(dev)
    assert not np.array_equal(T.save(g).cpu().numpy(), before)
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(obs), back.nbytes, 2) == 0
    assert back.reshape(3, 100, 36)[:, :, 9:18].any(axis=2).all(), "every due row was written (its rotation matrix is not zero)"
    for p in bufs:
        hip.hipFree(C.c_void_p(p))


def test_follows_the_oracle_at_a_control_rate(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(97)
    n = 700
    p = helpers.Pair(mrs, n, arith=mrs.ARITH_LITERAL)
    p.construct(0, 400, "x500")
    p.construct(400, 300, "f550")
    st = helpers.random_state(rng, n, 6, tilted=True)
    st["motor_rpm"][:400, 4:] = 0.0
    p.set_state(0, n, st)
    p.both("set_input", 0, n, O.VELOCITY_HDG_CMD, np.tile([0.5, 0.0, 0.2, 0.1], (n, 1)))
    dev = torch_dev(p.g)
    for mode, first, count, blocks, hold in ((O.POSITION_CMD, 0, 350, 6, 5), (O.ATTITUDE_RATE_CMD, 350, 100, 2, 10), (O.ACTUATOR_CMD, 450, 250, 6, 4),
                                             (O.ACCELERATION_HDG_CMD, 100, 500, 5, 3)):
        nm = 6 if first + count > 400 else 4
        c = commands(mode, rng, blocks, count, p.g.get_states(first, count)["x"], n_motors=nm)
        T.rollout(p.g, mode, torch.tensor(c, device=dev), DT, 0, first=first, hold=hold)
        for j in range(blocks):
            p.o.set_input(first, count, mode, c[j])
            for _ in range(hold):
                p.o.step(DT)
        p.compare(RTOL_LITERAL, f"mode {mode} held for {hold} steps")


@pytest.mark.parametrize("mode", ["ATTITUDE_RATE_CMD", "ACTUATOR_CMD"])
def test_mppi_fork_at_a_control_rate(mrs, mode):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    m = getattr(O, mode)
    rng = np.random.default_rng(101)
    src = mrs.Swarm(10, arith=mrs.ARITH_LITERAL)
    src.construct(0, 10, mrs.model_params("x500"), np.stack([np.arange(10) * 5.0, np.zeros(10), np.full(10, 8.0)], axis=1))
    src.set_input(0, 10, O.ATTITUDE_RATE_CMD, np.tile([0.1, -0.2, 0.05, 0.6], (10, 1)))
    src.step_n(DT, 50)
    S, H, hold, j = 256, 8, 10, 3  # 80 steps: two launches
    plan = mrs.Swarm(S, arith=mrs.ARITH_LITERAL)
    plan.construct(0, S, mrs.model_params("x500"))
    dev = torch_dev(src)
    rec = T.save(src, j, 1)
    T.load(plan, rec, index=torch.zeros(S, dtype=torch.int32, device=dev))
    nominal = commands(m, rng, H, 1, None, n_motors=4, width=4)
    u = np.repeat(nominal, S, axis=1) + np.concatenate([np.zeros((H, 1, nominal.shape[2])), rng.normal(0, 0.05, (H, S - 1, nominal.shape[2]))], axis=1)
    obs = T.rollout(plan, m, torch.tensor(u, device=dev), DT, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, first=0, hold=hold)
    assert obs.shape == (H, S, 10)
    cost = obs[:, :, 2].sum(0)  # a cost in torch: the samples are ranked without leaving the device
    assert cost.shape == (S,)
    own = []
    for t in range(H):
        src.set_input(j, 1, m, nominal[t])
        src.step_n(DT, hold)
        own.append(T.gather(src, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, j, 1, dtype=torch.float64)[0])
    o = obs.cpu().numpy()
    assert same(o[:, 0, :], torch.stack(own).cpu().numpy()), "sample 0 is the source UAV's own continuation"
    assert (np.abs(o[-1, 1:, :3] - o[-1, :1, :3]).max(axis=1) > 0).all(), "perturbed samples differ"


def test_caller_stream_is_fenced(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, b, c = (variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL) for _ in range(3))
    dev = torch_dev(a)
    rng = np.random.default_rng(103)
    src = torch.tensor(commands(O.ATTITUDE_RATE_CMD, rng, 9, COUNT, None), device=dev)
    want = T.rollout(a, O.ATTITUDE_RATE_CMD, src, DT, T.OBS_ALL, first=FIRST, hold=4).cpu().numpy()
    assert want.shape[0] == 9
    for g, side in ((b, torch.cuda.Stream(dev)), (c, torch.cuda.ExternalStream(c.stream(), device=dev))):
        cmd = torch.zeros_like(src)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
            cmd.copy_(src)  # written on the caller stream right before the call, no synchronisation
            out = T.rollout(g, O.ATTITUDE_RATE_CMD, cmd, DT, T.OBS_ALL, first=FIRST, hold=4)
            copy = out.clone()  # torch work after the call sees the rows
        side.synchronize()
        assert same(copy.cpu().numpy(), want)
        assert_same_state(a, g, "fenced rate rollout")


def child_main(out_path):
    """the pointer-addressed kernels (MRS_NO_BUFFER_ADDRESSING=1): cascade, model-only and mixed-block rate rollouts equal the decimated
    loop in LITERAL, and FAST equals the plain rollout on repeated commands, decimated"""
    import torch
    import mrs_multirotor_simulator_amd as M
    from mrs_multirotor_simulator_amd import tensors as T
    M.load_library()
    rng = np.random.default_rng(107)
    res = []
    for scen, mode in (("cascade", O.VELOCITY_HDG_CMD), ("model", O.ACTUATOR_CMD)):
        for hold, every, steps in ((3, 6, 132), (70, 35, 140)):
            a, b = variant_swarm(M, scen, M.ARITH_LITERAL), variant_swarm(M, scen, M.ARITH_LITERAL)
            dev = torch_dev(a)
            cmd = torch.tensor(commands(mode, rng, steps // hold, COUNT, a.get_states(FIRST, COUNT)["x"]), dtype=torch.float32, device=dev)
            want = rate_loop(a, mode, cmd, T.OBS_ALL, FIRST, torch.float32, hold, every)
            got = T.rollout(b, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every)
            assert raw_equal(got, want), f"LITERAL {scen} hold {hold}"
            assert_same_state(a, b, f"LITERAL {scen} hold {hold}")
            f1, f2 = variant_swarm(M, scen, M.ARITH_FAST), variant_swarm(M, scen, M.ARITH_FAST)
            one = T.rollout(f1, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every)
            plain = T.rollout(f2, mode, cmd.repeat_interleave(hold, 0), DT, T.OBS_ALL, first=FIRST)[every - 1::every]
            assert raw_equal(one, plain), f"FAST {scen} hold {hold}"
            assert_same_state(f1, f2, f"FAST {scen} hold {hold}")
        res.append(scen)
    np.save(out_path, np.array(res))


def test_pointer_form(mrs, tmp_path):
    if R._dead:
        pytest.fail(f"an earlier child process died ({R._dead[0]}): no further GPU process is started")
    out = str(tmp_path / "pointer.npy")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MRS_")}
    env["MRS_NO_BUFFER_ADDRESSING"] = "1"
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_rollout_rate_gpu as T; T.child_main({out!r})"
    try:
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        R._dead.append(f"pointer child timed out after {CHILD_TIMEOUT} s")
        pytest.fail(R._dead[0])
    if p.returncode < 0:
        R._dead.append(f"pointer child ended by signal {-p.returncode}")
        pytest.fail(f"{R._dead[0]}\n{p.stderr[-3000:]}")
    assert p.returncode == 0, p.stderr[-3000:]
    assert list(np.load(out)) == ["cascade", "model"]


def test_cpp_facade_equals_python(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    if R._dead:
        pytest.fail(f"an earlier child process died ({R._dead[0]}): no further GPU process is started")
    require_sentinel(mrs)  # (the C++ test hands the library rows of exactly the decimated size)
    n, B, hold, every = 1000, 6, 10, 20
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rollout_rate.bin")
        try:
            out = subprocess.run([build_cpp("rollout_rate_test"), path], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            R._dead.append(f"rollout_rate_test timed out after {CHILD_TIMEOUT} s")
            pytest.fail(R._dead[0])
        print(out.stdout)
        if out.returncode < 0:
            R._dead.append(f"rollout_rate_test ended by signal {-out.returncode}")
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok rows_equal_the_plain_rollout", "ok last_row_equals_pose_array", "ok rows_finite_and_moving", "ok refused_call_changes_nothing",
                    "ok written"):
            assert tag in out.stdout, out.stdout
        raw = np.fromfile(path, np.float64)
    i = np.arange(n)
    pos = np.stack([4.0 * (i % 32), 4.0 * (i // 32), np.full(n, 5.0)], axis=1)
    g = mrs.Swarm(n, arith=mrs.ARITH_FAST)  # (the facade's default)
    g.construct(0, n, mrs.default_params(), pos, 0.003 * i)
    t = np.arange(B)[:, None]
    cmd = np.stack([np.broadcast_to(0.02 * np.sin(0.1 * t + 0.001 * i), (B, n)), np.broadcast_to(-0.01 + 0.0 * t + 0.0 * i, (B, n)),
                    np.broadcast_to(0.3 + 0.0001 * i + 0.0 * t, (B, n)), np.broadcast_to(0.55 + 0.005 * t + 0.0 * i, (B, n))], axis=2)
    mine = T.rollout(g, O.ATTITUDE_RATE_CMD, torch.tensor(cmd, device=torch_dev(g)), DT, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, hold=hold,
                     obs_every=every).cpu().numpy()
    assert mine.shape == (B * hold // every, n, 10)
    assert raw.shape == (mine.size,) and same(raw, mine.reshape(-1))
