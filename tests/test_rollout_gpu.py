"""Device-resident rollouts on the GPU (include/mrs_swarm.h, "device-resident rollouts"; mrs_multirotor_simulator_amd.tensors.rollout):
in LITERAL a rollout equals the set_input / step_n / gather loop bit for bit (every observation row, the final state, PID and IMU) in all
11 modes, FP64 and FP32 rows and runs longer than one launch, on the variant-test swarm (three airframes, mixed-airframe blocks, a ragged
tail, held, crashed and NaN-rollback UAVs); FAST stays close to the loop and is bit-identical to itself in any split of the run; a rollout
follows the CPU oracle; collision ticks before and after a rollout continue as in the loop; an MPPI fork reproduces the source UAV's own
continuation; the caller's stream is fenced; refused calls change nothing; the pointer-addressed kernels (child process) and the C++
facade (tests/cpp/rollout_test.cpp) give the same rows.

ROLLOUT_KERNELS maps every entry point of rollout_device.inc to the test that forces it (test_rollout.py keeps the table complete)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import helpers
from helpers import RTOL_FAST, RTOL_LITERAL, RTOL_NORTH_STAR
from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_parity_gpu import payload_for
from test_step_variants_gpu import N_SINGLE, build_single, oracle_params, single_scenario

pytestmark = pytest.mark.gpu
DT = 0.001
REBOUNCE = 100.0
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
LAUNCH_CAP = 64  # kRolloutMaxSteps of rollout_device.inc
CHILD_TIMEOUT = 300

# which test forces each entry point of rollout_device.inc (both flavours)
ROLLOUT_KERNELS = {
    "mrs_uav_rollout": ("test_pointer_form",),
    "mrs_uav_rollout_buf": ("test_literal_equals_the_loop[cascade]",),
    "mrs_uav_model_rollout": ("test_pointer_form",),
    "mrs_uav_model_rollout_buf": ("test_literal_equals_the_loop[model]", "test_mppi_fork[ACTUATOR_CMD]"),
    "mrs_uav_rollout_mixed": ("test_literal_equals_the_loop[cascade]",),
}

_dead = []  # the first child process that died by a signal or timed out: nothing more is started on the GPU


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def full_state(g):
    a = g.get_states()
    s = {f: a[f] for f in a.dtype.names}
    s["pid"], s["f"], s["crashed"] = g.get_pid(), g.get_external_force(), np.asarray(g.has_crashed(), dtype=np.float64)
    return s


def assert_same_state(a, b, what):
    sa, sb = full_state(a), full_state(b)
    for k in sa:
        da, db = bits(sa[k]).reshape(len(sa[k]), -1), bits(sb[k]).reshape(len(sb[k]), -1)
        bad = np.flatnonzero((da != db).any(axis=1))
        assert len(bad) == 0, f"{what}: {k} differs for {len(bad)} UAVs, first {bad[:8]}"


def loop(g, mode, cmd, groups, first, out_dtype):
    """what rollout stands for: set_input / step_n / gather per step, through tensors"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    steps, count = cmd.shape[0], cmd.shape[1]
    out = torch.empty((steps, count, T.gather_width(groups)), dtype=out_dtype, device=cmd.device) if groups else None
    for t in range(steps):
        T.set_input(g, mode, cmd[t], first)
        g.step_n(DT, 1)
        if groups:
            T.gather(g, groups, first, count, out=out[t])
    return out


def commands(mode, rng, steps, count, x, n_motors=8, width=10):
    """[steps, count, width] payload rows of `mode` (ACTUATOR: n_motors throttles, dense)"""
    w = n_motors if mode == O.ACTUATOR_CMD else width
    c = np.zeros((steps, count, w))
    for t in range(steps):
        p = payload_for(O, mode, rng, count, n_motors, {"x": x})
        if p is not None:
            c[t, :, :p.shape[1]] = p
    return c


def variant_swarm(mrs, scen, arith):
    """the swarm of test_step_variants_gpu (cascade: every mode, or all ACTUATOR_CMD) with crashed UAVs (one collision tick in crash
    mode) and held UAVs inside and outside the range of the calls below"""
    sc = single_scenario(scen == "model")
    g = mrs.Swarm(N_SINGLE, arith=arith)
    build_single(g, sc, lambda name: helpers.to_product_params(mrs, oracle_params(name)))
    g.tick_n(DT, 1, True, True, REBOUNCE)
    g.set_hold(1950, 3, True)
    g.set_hold(100, 2, True)
    return g


# the range of the calls: naki blocks, the mixed-airframe blocks 35-40 and the ragged tail (64 * 40 + 23 UAVs)
FIRST = 1900
COUNT = N_SINGLE - FIRST


@pytest.mark.parametrize("scen", ["cascade", "model"])
def test_literal_equals_the_loop(mrs, scen):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, b = variant_swarm(mrs, scen, mrs.ARITH_LITERAL), variant_swarm(mrs, scen, mrs.ARITH_LITERAL)
    assert np.asarray(a.has_crashed()).any(), "the scenario has crashed UAVs"
    dev = torch_dev(a)
    rng = np.random.default_rng(41)
    modes = range(11) if scen == "cascade" else (O.ACTUATOR_CMD, O.INPUT_UNKNOWN, O.ACTUATOR_CMD)
    for dtype in (torch.float64, torch.float32):
        for mode in modes:
            for steps in (1, 5, LAUNCH_CAP + 3):
                x = a.get_states(FIRST, COUNT)["x"]
                cmd = torch.tensor(commands(mode, rng, steps, COUNT, x), dtype=dtype, device=dev)
                want = loop(a, mode, cmd, T.OBS_ALL, FIRST, dtype)
                got = T.rollout(b, mode, cmd, DT, T.OBS_ALL, first=FIRST)
                what = f"{dtype} mode {mode} T={steps}"
                w, gt = want.cpu().numpy(), got.cpu().numpy()
                assert np.array_equal(w.view(np.uint8), gt.view(np.uint8)), f"{what}: observation rows differ at {np.argwhere(w != gt)[:5]}"
                assert_same_state(a, b, what)
    # the non-finite velocities of the scenario took the NaN-rollback path in both, as often; the other counters agree too
    assert b.get_diag() == a.get_diag() and b.get_diag()["nan_rollback"] > 0


def test_fast_tracks_the_loop_and_itself(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    loop_g = variant_swarm(mrs, "cascade", mrs.ARITH_FAST)
    one, split = variant_swarm(mrs, "cascade", mrs.ARITH_FAST), variant_swarm(mrs, "cascade", mrs.ARITH_FAST)
    dev = torch_dev(one)
    rng = np.random.default_rng(43)
    steps = 24
    cmd = torch.tensor(commands(O.ATTITUDE_RATE_CMD, rng, steps, COUNT, None), dtype=torch.float64, device=dev)
    want = loop(loop_g, O.ATTITUDE_RATE_CMD, cmd, T.OBS_POS | T.OBS_VEL | T.OBS_ROT, FIRST, torch.float64).cpu().numpy()
    got = T.rollout(one, O.ATTITUDE_RATE_CMD, cmd, DT, T.OBS_POS | T.OBS_VEL | T.OBS_ROT, first=FIRST).cpu().numpy()
    ok = np.isfinite(want).all(axis=(0, 2))
    helpers.assert_close(got[0][ok], want[0][ok], RTOL_FAST, "FAST rollout vs loop after one step")
    helpers.assert_close(got[-1][ok], want[-1][ok], RTOL_NORTH_STAR, "FAST rollout vs loop after the run")
    # one call of T steps == T calls of one step, bit for bit
    rows = [T.rollout(split, O.ATTITUDE_RATE_CMD, cmd[t:t + 1], DT, T.OBS_POS | T.OBS_VEL | T.OBS_ROT, first=FIRST) for t in range(steps)]
    assert np.array_equal(torch.cat(rows).cpu().numpy().view(np.uint64), got.view(np.uint64))
    assert_same_state(one, split, "FAST: one call vs single-step calls")
    # the last row is gather_device of the final state
    last = T.rollout(one, O.ATTITUDE_RATE_CMD, cmd[:3], DT, T.OBS_ALL, first=FIRST)[-1]
    assert same(last.cpu().numpy(), T.gather(one, T.OBS_ALL, FIRST, COUNT, dtype=torch.float64).cpu().numpy())


def test_follows_the_oracle(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(47)
    n = 700
    p = helpers.Pair(mrs, n, arith=mrs.ARITH_LITERAL)
    p.construct(0, 400, "x500")
    p.construct(400, 300, "f550")
    st = helpers.random_state(rng, n, 6, tilted=True)
    st["motor_rpm"][:400, 4:] = 0.0
    p.set_state(0, n, st)
    p.both("set_input", 0, n, O.VELOCITY_HDG_CMD, np.tile([0.5, 0.0, 0.2, 0.1], (n, 1)))
    dev = torch_dev(p.g)
    for mode, first, count, steps in ((O.POSITION_CMD, 0, 350, 30), (O.ATTITUDE_RATE_CMD, 350, 100, 20), (O.ACTUATOR_CMD, 450, 250, 25),
                                      (O.ACCELERATION_HDG_CMD, 100, 500, 15)):
        nm = 6 if first + count > 400 else 4
        c = commands(mode, rng, steps, count, p.g.get_states(first, count)["x"], n_motors=nm)
        T.rollout(p.g, mode, torch.tensor(c, device=dev), DT, 0, first=first)
        for t in range(steps):
            p.o.set_input(first, count, mode, c[t])
            p.o.step(DT)
        p.compare(RTOL_LITERAL, f"mode {mode}")


@pytest.mark.parametrize("crash", [False, True])
def test_after_collision_ticks(mrs, crash):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, b = variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL), variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL)
    dev = torch_dev(a)
    rng = np.random.default_rng(53)
    cmd = torch.tensor(commands(O.VELOCITY_HDG_CMD, rng, 12, COUNT, None), device=dev)
    for g in (a, b):
        g.tick_n(DT, 7, True, crash, REBOUNCE)
    want = loop(a, O.VELOCITY_HDG_CMD, cmd, T.OBS_POS | T.OBS_VEL, FIRST, torch.float64)
    got = T.rollout(b, O.VELOCITY_HDG_CMD, cmd, DT, T.OBS_POS | T.OBS_VEL, first=FIRST)
    assert same(want.cpu().numpy(), got.cpu().numpy())
    for g in (a, b):
        g.tick_n(DT, 9, True, crash, REBOUNCE)
    assert_same_state(a, b, f"ticks after the rollout (crash={crash})")


@pytest.mark.parametrize("mode", ["ATTITUDE_RATE_CMD", "ACTUATOR_CMD"])
def test_mppi_fork(mrs, mode):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    m = getattr(O, mode)
    rng = np.random.default_rng(59)
    src = mrs.Swarm(10, arith=mrs.ARITH_LITERAL)
    src.construct(0, 10, mrs.model_params("x500"), np.stack([np.arange(10) * 5.0, np.zeros(10), np.full(10, 8.0)], axis=1))
    src.set_input(0, 10, O.ATTITUDE_RATE_CMD, np.tile([0.1, -0.2, 0.05, 0.6], (10, 1)))
    src.step_n(DT, 50)
    S, H, j = 256, 30, 3
    plan = mrs.Swarm(S, arith=mrs.ARITH_LITERAL)
    plan.construct(0, S, mrs.model_params("x500"))
    dev = torch_dev(src)
    rec = T.save(src, j, 1)
    T.load(plan, rec, index=torch.zeros(S, dtype=torch.int32, device=dev))
    nominal = commands(m, rng, H, 1, None, n_motors=4, width=4)
    cmd = np.repeat(nominal, S, axis=1) + np.concatenate([np.zeros((H, 1, nominal.shape[2])), rng.normal(0, 0.05, (H, S - 1, nominal.shape[2]))], axis=1)
    obs = T.rollout(plan, m, torch.tensor(cmd, device=dev), DT, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, first=0)
    cost = obs[:, :, 2].sum(0)  # a cost in torch: the samples are ranked without leaving the device
    assert cost.shape == (S,)
    own = []
    for t in range(H):
        src.set_input(j, 1, m, nominal[t])
        src.step_n(DT, 1)
        own.append(T.gather(src, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, j, 1, dtype=torch.float64)[0])
    o = obs.cpu().numpy()
    assert same(o[:, 0, :], torch.stack(own).cpu().numpy()), "sample 0 is the source UAV's own continuation"
    assert (np.abs(o[-1, 1:, :3] - o[-1, :1, :3]).max(axis=1) > 0).all(), "perturbed samples differ"


def test_caller_stream_is_fenced(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, b, c = (variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL) for _ in range(3))
    dev = torch_dev(a)
    rng = np.random.default_rng(61)
    src = torch.tensor(commands(O.ATTITUDE_RATE_CMD, rng, 9, COUNT, None), device=dev)
    want = T.rollout(a, O.ATTITUDE_RATE_CMD, src, DT, T.OBS_ALL, first=FIRST).cpu().numpy()
    for g, side in ((b, torch.cuda.Stream(dev)), (c, torch.cuda.ExternalStream(c.stream(), device=dev))):
        cmd = torch.zeros_like(src)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
            cmd.copy_(src)  # written on the caller stream right before the call, no synchronisation
            out = T.rollout(g, O.ATTITUDE_RATE_CMD, cmd, DT, T.OBS_ALL, first=FIRST)
            copy = out.clone()  # torch work after the call sees the rows
        side.synchronize()
        assert same(copy.cpu().numpy(), want)
        assert_same_state(a, g, "fenced rollout")


def _hip_malloc(nbytes):
    """device memory of exactly nbytes (a torch tensor sits inside a larger segment of the caching allocator, whose end the library
    cannot tell from the tensor's)"""
    hip = C.CDLL("libamdhip64.so")
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
    assert hip.hipMemset(p, 0, C.c_size_t(nbytes)) == 0 and hip.hipDeviceSynchronize() == 0
    return hip, p.value


def test_refused_calls_change_nothing(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL)
    dev = torch_dev(g)
    before = T.save(g).cpu().numpy()
    hip, cmd = _hip_malloc(4 * 100 * 10 * 8)  # 4 steps x 100 UAVs x 10 FP64
    _, obs = _hip_malloc(4 * 100 * 36 * 8)
    _, small = _hip_malloc(3 * 100 * 36 * 8)
    host = np.zeros((4, 100, 36))
    ok = dict(first=0, count=100, mode=O.POSITION_CMD, dt=DT, n_steps=4, dev_cmd=cmd, dtype=T.DTYPE_F64, cmd_stride=10, groups=T.OBS_ALL,
              dev_obs=obs, obs_stride=36, ext_stream=None)
    bad = [({"first": N_SINGLE - 5}, 3), ({"count": -1}, 3), ({"mode": 11}, 1), ({"mode": -1}, 1), ({"dtype": 2}, 1), ({"n_steps": 0}, 1),
           ({"dt": 0.0}, 1), ({"dt": -DT}, 1), ({"dt": float("nan")}, 1), ({"dt": float("inf")}, 1), ({"cmd_stride": 3}, 1),
           ({"groups": 0x100}, 1), ({"obs_stride": 35}, 1), ({"dev_obs": None}, 1), ({"dev_cmd": None}, 1), ({"dev_cmd": host.ctypes.data}, 1),
           ({"dev_obs": small}, 1), ({"n_steps": 5}, 1), ({"mode": O.ACTUATOR_CMD, "cmd_stride": 4, "first": 1900}, 1)]
    for change, code in bad:
        with pytest.raises(mrs.MrsError, match=f"error {code}:"):
            g.rollout_device(**dict(ok, **change))
        assert np.array_equal(T.save(g).cpu().numpy(), before), change
    back = np.zeros(4 * 100 * 36)
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(obs), back.nbytes, 2) == 0
    assert not back.any(), "a refused call wrote observation rows"
    # the tensor layer refuses before any library call
    with pytest.raises(ValueError):
        T.rollout(g, O.POSITION_CMD, torch.zeros((4, 100, 4), dtype=torch.float64), DT)
    g.rollout_device(**ok)  # and the unchanged arguments are accepted
    torch.cuda.synchronize(dev)
    assert not np.array_equal(T.save(g).cpu().numpy(), before)
    for p in (cmd, obs, small):
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
    for g in shards:
        x = g.get_states()["x"]
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.rollout(g, O.POSITION_CMD, cmd, DT, out=out)
        assert same(g.get_states()["x"], x)
    assert not out.any()
    for g in shards:
        g.close()
    group.close()


def child_main(out_path):
    """the pointer-addressed kernels (MRS_NO_BUFFER_ADDRESSING=1): cascade, model-only and mixed-block rollouts equal the loop in
    LITERAL, and FAST equals itself split into single steps"""
    import torch
    import mrs_multirotor_simulator_amd as M
    from mrs_multirotor_simulator_amd import tensors as T
    M.load_library()
    rng = np.random.default_rng(67)
    res = []
    for scen, mode in (("cascade", O.VELOCITY_HDG_CMD), ("model", O.ACTUATOR_CMD)):
        a, b = variant_swarm(M, scen, M.ARITH_LITERAL), variant_swarm(M, scen, M.ARITH_LITERAL)
        dev = torch_dev(a)
        cmd = torch.tensor(commands(mode, rng, LAUNCH_CAP + 3, COUNT, a.get_states(FIRST, COUNT)["x"]), dtype=torch.float32, device=dev)
        want = loop(a, mode, cmd, T.OBS_ALL, FIRST, torch.float32).cpu().numpy()
        got = T.rollout(b, mode, cmd, DT, T.OBS_ALL, first=FIRST).cpu().numpy()
        assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), f"LITERAL {scen}"
        assert_same_state(a, b, f"LITERAL {scen}")
        f1, f2 = variant_swarm(M, scen, M.ARITH_FAST), variant_swarm(M, scen, M.ARITH_FAST)
        one = T.rollout(f1, mode, cmd[:6], DT, T.OBS_ALL, first=FIRST)
        split = torch.cat([T.rollout(f2, mode, cmd[t:t + 1], DT, T.OBS_ALL, first=FIRST) for t in range(6)])
        assert torch.equal(one.view(torch.int32), split.view(torch.int32)), f"FAST {scen}"
        res.append(scen)
    np.save(out_path, np.array(res))


def test_pointer_form(mrs, tmp_path):
    if _dead:
        pytest.fail(f"an earlier child process of this module died ({_dead[0]}): no further GPU process is started")
    out = str(tmp_path / "pointer.npy")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MRS_")}
    env["MRS_NO_BUFFER_ADDRESSING"] = "1"
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_rollout_gpu as T; T.child_main({out!r})"
    try:
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _dead.append(f"pointer child timed out after {CHILD_TIMEOUT} s")
        pytest.fail(_dead[0])
    if p.returncode < 0:
        _dead.append(f"pointer child ended by signal {-p.returncode}")
        pytest.fail(f"{_dead[0]}\n{p.stderr[-3000:]}")
    assert p.returncode == 0, p.stderr[-3000:]
    assert list(np.load(out)) == ["cascade", "model"]


def test_cpp_facade_equals_python(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, H = 1000, 20
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rollout.bin")
        out = subprocess.run([build_cpp("rollout_test"), path], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok last_row_equals_pose_array", "ok rows_finite_and_moving", "ok written"):
            assert tag in out.stdout, out.stdout
        raw = np.fromfile(path, np.float64)
    i = np.arange(n)
    pos = np.stack([4.0 * (i % 32), 4.0 * (i // 32), np.full(n, 5.0)], axis=1)
    p = mrs.default_params()
    g = mrs.Swarm(n, arith=mrs.ARITH_FAST)  # (the facade's default)
    g.construct(0, n, p, pos, 0.003 * i)
    t = np.arange(H)[:, None]
    cmd = np.stack([np.broadcast_to(0.02 * np.sin(0.1 * t + 0.001 * i), (H, n)), np.broadcast_to(-0.01 + 0.0 * t + 0.0 * i, (H, n)),
                    np.broadcast_to(0.3 + 0.0001 * i + 0.0 * t, (H, n)), np.broadcast_to(0.55 + 0.005 * t + 0.0 * i, (H, n))], axis=2)
    mine = T.rollout(g, O.ATTITUDE_RATE_CMD, torch.tensor(cmd, device=torch_dev(g)), DT, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT).cpu().numpy()
    assert raw.shape == (H * n * 10,) and same(raw, mine.reshape(-1))
