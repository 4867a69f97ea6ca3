"""Device-resident callers on the GPU (include/mrs_swarm.h, "device-resident callers"; mrs_multirotor_simulator_amd.tensors): observation
rows gathered into torch tensors equal the host downloads bit for bit, commands from device rows equal the host setInput, masked resets
equal a fresh construct, a torch closed loop with lazily evaluated collision ticks equals the numpy host loop, the caller's stream is
fenced, and the C++ facade (tests/cpp/device_io_test.cpp) agrees with the pose array."""
import os
import subprocess

import numpy as np
import pytest

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGES = ((1, 63), (65, 130), (0, 1), (1499, 3))  # + (n - 37, 37): not aligned to 64, across the airframe boundary at 1500
DT = 0.001


def build_cpp(name="device_io_test"):
    from mrs_multirotor_simulator_amd import swarm
    exe = os.path.join(ROOT, "tests", "cpp", name)
    libdir = os.path.dirname(swarm.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-DMRS_NO_EIGEN", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L", libdir, "-lmrs_swarm",
                           "-L", "/opt/rocm/lib", "-lamdhip64", "-lpthread", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def mixed_swarm(mrs, n=3000, seed=5, arith=None, pos=None):
    """x500 (4 motors) in [0, n/2), f550 (6 motors) in [n/2, n), random flight state, no command yet"""
    rng = np.random.default_rng(seed)
    g = mrs.Swarm(n, arith=mrs.ARITH_FAST if arith is None else arith)
    h = n // 2
    g.construct(0, h, mrs.model_params("x500", ground_enabled=True, ground_z=0.0), None if pos is None else pos[:h])
    g.construct(h, n - h, mrs.model_params("f550", ground_enabled=True, ground_z=-2.0), None if pos is None else pos[h:])
    st = helpers.random_state(rng, n, 6, tilted=True)
    st["motor_rpm"][:h, 4:] = 0.0
    g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    return g, st, rng


def torch_dev(g):
    import torch
    return torch.device("cuda", g.device())


@pytest.mark.gpu
def test_gather_equals_the_host_downloads(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, st, rng = mixed_swarm(mrs)
    n = g.n
    g.set_input(0, n // 2, mrs.ACTUATOR_CMD, rng.uniform(0.4, 0.6, (n // 2, 4)))
    g.set_input(n // 2, n // 2, mrs.ACTUATOR_CMD, rng.uniform(0.4, 0.6, (n // 2, 6)))
    g.step_n(DT, 3)
    assert T.gather(g, 0xFF).shape == (n, 36)
    full = T.gather(g, T.OBS_ALL, dtype=torch.float64).cpu().numpy()
    s, poses, outs = g.get_states(), g.get_poses(), g.get_outputs()
    want = np.concatenate([s["x"], s["v"], outs["velocity_body"], s["R"].reshape(n, 9), poses["orientation"], s["omega"],
                           s["imu_acceleration"], s["motor_rpm"]], axis=1)
    assert np.abs(s["imu_acceleration"]).max() > 0 and (s["motor_rpm"][n // 2:, 4:6] != 0).all() and (s["motor_rpm"][:n // 2, 4:] == 0).all()
    for c in range(36):
        assert np.array_equal(full[:, c], want[:, c]), f"column {c}"
    f32 = T.gather(g, T.OBS_ALL).cpu().numpy()
    assert f32.dtype == np.float32 and np.array_equal(f32.view(np.uint32), want.astype(np.float32).view(np.uint32))
    # single groups, sub-ranges not aligned to 64, both dtypes
    cols = {T.OBS_POS: (0, 3), T.OBS_VEL: (3, 6), T.OBS_VEL_BODY: (6, 9), T.OBS_ROT: (9, 18), T.OBS_QUAT: (18, 22), T.OBS_OMEGA: (22, 25),
            T.OBS_IMU: (25, 28), T.OBS_RPM: (28, 36)}
    for first, count in RANGES + ((n - 37, 37),):
        for grp, (a, b) in cols.items():
            got = T.gather(g, grp, first, count, dtype=torch.float64).cpu().numpy()
            assert np.array_equal(got, want[first:first + count, a:b]), (first, count, grp)
        two = T.gather(g, T.OBS_QUAT | T.OBS_POS, first, count).cpu().numpy()  # bit order, not argument order: POS first
        assert np.array_equal(two, want[first:first + count][:, list(range(0, 3)) + list(range(18, 22))].astype(np.float32))
    # rows wider than the groups: the padding is left alone
    for dtype in (torch.float32, torch.float64):
        buf = torch.full((130, 12), 7.25, dtype=dtype, device=torch_dev(g))
        view = T.gather(g, T.OBS_POS | T.OBS_QUAT, 65, 130, out=buf[:, 2:9])
        assert view.shape == (130, 7)
        host = buf.cpu().numpy()
        assert (host[:, :2] == 7.25).all() and (host[:, 9:] == 7.25).all()
        assert np.array_equal(host[:, 2:9], want[65:195][:, [0, 1, 2, 18, 19, 20, 21]].astype(host.dtype))


@pytest.mark.gpu
def test_bad_arguments_are_error_codes(mrs):
    """range, dtype, stride and mode errors come back as codes before any launch; the swarm keeps working"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, _, _ = mixed_swarm(mrs, n=300)
    rows = torch.zeros((300, 8), dtype=torch.float64, device=torch_dev(g))
    st = torch.cuda.current_stream(torch_dev(g)).cuda_stream
    with pytest.raises(mrs.MrsError, match="error 3:"):
        g.gather_device(200, 101, T.OBS_POS, rows.data_ptr(), T.DTYPE_F64, 8, st)
    with pytest.raises(mrs.MrsError, match="error 1:.*stride"):
        g.gather_device(0, 300, T.OBS_ROT, rows.data_ptr(), T.DTYPE_F64, 8, st)
    with pytest.raises(mrs.MrsError, match="error 1:.*dtype"):
        g.gather_device(0, 300, T.OBS_POS, rows.data_ptr(), 2, 8, st)
    with pytest.raises(mrs.MrsError, match="error 1:.*no observation group"):
        g.gather_device(0, 300, 0, rows.data_ptr(), T.DTYPE_F64, 8, st)
    with pytest.raises(mrs.MrsError, match="error 1:.*null pointer"):
        g.gather_device(0, 300, T.OBS_POS, 0, T.DTYPE_F64, 8, st)
    with pytest.raises(mrs.MrsError, match="error 1:.*bad input mode"):
        g.set_input_device(0, 300, 11, rows.data_ptr(), T.DTYPE_F64, 8, st)
    with pytest.raises(mrs.MrsError, match="error 1:.*narrower than n_motors"):
        g.set_input_device(0, 300, mrs.ACTUATOR_CMD, rows.data_ptr(), T.DTYPE_F64, 4, st)  # f550 UAVs have 6 motors
    with pytest.raises(ValueError, match="rows are not contiguous"):
        T.set_input(g, mrs.POSITION_CMD, rows[:, ::2])
    T.set_input(g, mrs.POSITION_CMD, rows[:, :4].contiguous())
    g.step_n(DT, 2)
    assert np.isfinite(T.gather(g, T.OBS_ALL, dtype=torch.float64).cpu().numpy()).all()


def _command_rows(mrs, mode, rng, count, n_motors):
    if mode == mrs.ACTUATOR_CMD:
        return rng.uniform(0.4, 0.6, (count, n_motors))
    if mode == mrs.ATTITUDE_CMD:
        R = helpers.random_rotations(rng, count)
        return np.concatenate([R.reshape(count, 9), rng.uniform(0.45, 0.6, (count, 1))], axis=1)
    return np.concatenate([rng.uniform(-5, 5, (count, 3)) + [0, 0, 20], rng.uniform(-3, 3, (count, 1))], axis=1)  # POSITION


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
@pytest.mark.parametrize("mode", ["ACTUATOR", "ATTITUDE", "POSITION"])
def test_device_commands_equal_host_commands(mrs, arith, mode):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ar = getattr(mrs, f"ARITH_{arith}")
    md = getattr(mrs, f"{mode}_CMD")
    a, _, rng = mixed_swarm(mrs, arith=ar, seed=7)
    b, _, _ = mixed_swarm(mrs, arith=ar, seed=7)
    n, h = a.n, a.n // 2
    dev = torch_dev(b)
    for dtype in (torch.float64, torch.float32):
        # x500 rows and f550 rows separately (4 / 6 actuators), ranges not aligned to 64
        for first, count, nm in ((0, 65, 4), (65, h - 65, 4), (h, n - h - 37, 6), (n - 37, 37, 6)):
            rows = _command_rows(mrs, md, rng, count, nm)
            t = torch.tensor(rows, dtype=dtype, device=dev)
            T.set_input(b, md, t, first)
            a.set_input(first, count, md, t.cpu().numpy().astype(np.float64))
        a.step_n(DT, 50)
        b.step_n(DT, 50)
        sa, sb = a.get_states(), b.get_states()
        for f in sa.dtype.names:
            assert np.array_equal(sa[f], sb[f]), f"{mode} {arith} {dtype}: {f}"
        assert np.array_equal(a.get_pid(), b.get_pid())


def _construct_runs(g, runs, params_of, pos, heading=None, cut=None):
    """construct each run again with its airframe's params; `cut` splits a run that straddles the airframe boundary"""
    for lo, hi in runs:
        for a, b in ((lo, hi),) if cut is None or not lo < cut < hi else ((lo, cut), (cut, hi)):
            g.construct(a, b - a, params_of(a), pos[a:b], None if heading is None else heading[a:b])


def _runs(mask):
    idx = np.flatnonzero(mask)
    runs, lo = [], None
    for k, i in enumerate(idx):
        if lo is None:
            lo = i
        if k + 1 == len(idx) or idx[k + 1] != i + 1:
            runs.append((lo, i + 1))
            lo = None
    return runs


@pytest.mark.gpu
def test_masked_reset_equals_a_fresh_construct(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, h = 3000, 1500
    grid = np.stack([4.0 * (np.arange(n) % 50), 4.0 * (np.arange(n) // 50), np.full(n, 10.0)], axis=1)
    params = {"x500": mrs.model_params("x500", ground_enabled=True, ground_z=0.0), "f550": mrs.model_params("f550", ground_enabled=True, ground_z=-2.0)}
    params_of = lambda i: params["x500"] if i < h else params["f550"]  # noqa: E731
    g, _, rng = mixed_swarm(mrs, pos=grid)
    g.set_state(0, n, grid, None, None, None, None)
    cmd = np.concatenate([grid + rng.uniform(-2, 2, (n, 3)), rng.uniform(-3, 3, (n, 1))], axis=1)
    g.set_input(0, n, mrs.POSITION_CMD, cmd)
    g.tick_n(DT, 30, True, False, 100.0)
    g.crash(60, 10)
    g.set_state(70, 4, None, np.ones((4, 3)), None, None, None)  # v_prev split from v
    mask = np.zeros(n, bool)
    for lo, hi in ((1, 64), (65, 195), (1490, 1530), (n - 37, n)):
        mask[lo:hi] = True
    mask[rng.choice(n, 40, replace=False)] = True
    newpos = grid + rng.uniform(-0.5, 0.5, (n, 3)) + [0, 0, 1.0]
    dev = torch_dev(g)
    before = g.get_states()
    base = g.clone()  # for the tick comparison below: two copies with the same (fresh) collision bookkeeping
    T.reset(g, torch.tensor(mask, device=dev), torch.tensor(newpos, device=dev), takeoff=bool(params["x500"].takeoff_patch_enabled))
    fresh = mrs.Swarm(n, arith=mrs.ARITH_FAST)
    fresh.construct(0, h, params["x500"], newpos[:h])
    fresh.construct(h, n - h, params["f550"], newpos[h:])
    after, want = g.get_states(), fresh.get_states()
    for f in after.dtype.names:
        assert np.array_equal(after[f][mask], want[f][mask]), f"masked {f}"
        assert np.array_equal(after[f][~mask], before[f][~mask]), f"unmasked {f}"
    assert np.array_equal(g.get_pid()[mask], fresh.get_pid()[mask])
    assert np.array_equal(g.get_external_force()[mask], fresh.get_external_force()[mask])
    assert np.array_equal(g.get_imu()[mask], fresh.get_imu()[mask])
    assert not g.has_crashed()[mask].any() and g.has_crashed()[60:70][~mask[60:70]].all()
    for i in np.flatnonzero(mask)[:5]:
        assert g.get_params(int(i)).takeoff_patch_enabled == params_of(i).takeoff_patch_enabled
    # commands and mode kept: 200 collision ticks equal the host-built equivalent (construct the masked UAVs, set their command again)
    dv, host = base.clone(), base.clone()
    T.reset(dv, torch.tensor(mask, device=dev), torch.tensor(newpos, device=dev), takeoff=bool(params["x500"].takeoff_patch_enabled))
    _construct_runs(host, _runs(mask), params_of, newpos, cut=h)
    for lo, hi in _runs(mask):
        host.set_input(lo, hi - lo, mrs.POSITION_CMD, cmd[lo:hi])
    dv.tick_n(DT, 200, True, False, 100.0)
    host.tick_n(DT, 200, True, False, 100.0)
    sg, sh = dv.get_states(), host.get_states()
    for f in sg.dtype.names:
        assert np.array_equal(sg[f], sh[f]), f"after 200 ticks: {f}"
    assert np.array_equal(dv.get_pid(), host.get_pid())
    moved = np.abs(sg["x"][mask] - newpos[mask]).max()
    assert moved > 0.1, moved

    # random headings: R from the device's sin / cos within 4e-16 of the host's
    hd = rng.uniform(-3.14, 3.14, n)
    T.reset(g, torch.tensor(mask, device=dev), torch.tensor(newpos, device=dev), torch.tensor(hd, device=dev))
    fresh.construct(0, h, params["x500"], newpos[:h], hd[:h])
    fresh.construct(h, n - h, params["f550"], newpos[h:], hd[h:])
    got, want = g.get_states(), fresh.get_states()
    assert np.abs(got["R"][mask] - want["R"][mask]).max() <= 4e-16
    for f in ("x", "v", "omega", "motor_rpm"):
        assert np.array_equal(got[f][mask], want[f][mask]), f
    # FP32 positions: the widened values
    T.reset(g, torch.tensor(mask, device=dev).to(torch.uint8), torch.tensor(newpos, dtype=torch.float32, device=dev))
    assert np.array_equal(g.get_states()["x"][mask], newpos.astype(np.float32).astype(np.float64)[mask])


@pytest.mark.gpu
def test_reset_refused_on_a_sharded_swarm(mrs):
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
    for g in shards:
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.reset(g, torch.ones(100, dtype=torch.bool, device=dev), torch.zeros((100, 3), dtype=torch.float64, device=dev))
        x = T.gather(g, T.OBS_POS, dtype=torch.float64).cpu().numpy()  # the local shard
        assert np.array_equal(x, g.get_states()["x"])
    for g in shards:
        g.close()
    group.close()


def _stall_pair(mrs, n, seed, v_fast=170.0, n_fast=8):
    """the stall recipe of test_pose_payload_gpu: dense flight with collisions, a few UAVs fast enough to leave their skin in one step"""
    import bench
    st, cmd = bench.make_inputs(n, "position+collisions", seed=seed, volume_per_uav=16.0)
    st["v"][:n_fast] = [0.0, v_fast, 0.0]
    p = mrs.model_params("x500", ground_enabled=True, ground_z=0.0)

    def make():
        g = mrs.Swarm(n, arith=mrs.ARITH_FAST)
        g.construct(0, n, p)
        g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
        return g

    return make(), make(), st, cmd, p


@pytest.mark.gpu
@pytest.mark.parametrize("crash", [False, True])
def test_closed_loop_with_lazy_collision_ticks(mrs, crash):
    """gather POS -> torch policy -> set_input_device -> tick, resets of crashed UAVs every 50 ticks in crash mode, against the numpy host
    loop (pipelined pose download -> policy -> set_input -> tick, has_crashed + construct): identical final states, stalls happened"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, ticks, k_gain, v_max = 20_000, 300, 0.8, 3.0
    a, b, st, cmd, p = _stall_pair(mrs, n, seed=17)
    goal = cmd[:, :3]
    spawn = st["x"].copy()
    dev = torch_dev(b)
    goal_t, spawn_t = torch.tensor(goal, device=dev), torch.tensor(spawn, device=dev)
    rows_t = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    rows = np.zeros((n, 4))
    resets = 0
    for t in range(ticks):
        if crash and t == 20:  # (so that the resets below have something to do whatever the collisions crashed)
            a.crash(100, 5)
            b.crash(100, 5)
        pos = a.poses_wait(a.get_poses_async())["position"]
        rows[:, :3] = np.clip(k_gain * (goal - pos), -v_max, v_max)
        a.set_input(0, n, mrs.VELOCITY_HDG_CMD, rows)
        a.tick_n(DT, 1, True, crash, 100.0)

        x = T.gather(b, T.OBS_POS, dtype=torch.float64)
        rows_t[:, :3] = torch.clamp(k_gain * (goal_t - x), -v_max, v_max)
        T.set_input(b, mrs.VELOCITY_HDG_CMD, rows_t)
        b.tick_n(DT, 1, True, crash, 100.0)
        if crash and t % 50 == 49:
            c = a.has_crashed().astype(bool)
            for lo, hi in _runs(c):
                a.construct(lo, hi - lo, p, spawn[lo:hi])
            m = T.crashed(b)
            assert np.array_equal(m.cpu().numpy(), c), t
            T.reset(b, m, spawn_t, takeoff=bool(p.takeoff_patch_enabled))
            resets += int(c.sum())
    sa, sb = a.get_states(), b.get_states()
    for f in sa.dtype.names:
        assert np.array_equal(sa[f], sb[f]), f
    assert np.array_equal(a.get_pid(), b.get_pid()) and np.array_equal(a.get_external_force(), b.get_external_force())
    fused, stalls, replayed, ahead = b.fused_stats()
    print(f"closed loop, crash={crash}: {fused} fused launches, {stalls} stalls, {replayed} replayed, {resets} UAVs reset")
    assert stalls >= 1, (fused, stalls)
    if crash:
        assert resets > 0


@pytest.mark.gpu
def test_caller_stream_is_fenced(mrs):
    """the command rows are written on a side stream kept busy by a long sleep; set_input_device called with that stream as the current
    one must read the written rows (the event fence), not the zeros that were there before"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, _, rng = mixed_swarm(mrs, n=3000, seed=9)
    b, _, _ = mixed_swarm(mrs, n=3000, seed=9)
    n = a.n
    cmd = _command_rows(mrs, mrs.POSITION_CMD, rng, n, 4)
    dev = torch_dev(b)
    rows = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    src = torch.tensor(cmd, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)  # milliseconds of stream time before the write
        rows.copy_(src)
        T.set_input(b, mrs.POSITION_CMD, rows)
    a.set_input(0, n, mrs.POSITION_CMD, cmd)
    a.step_n(DT, 20)
    b.step_n(DT, 20)
    sa, sb = a.get_states(), b.get_states()
    for f in sa.dtype.names:
        assert np.array_equal(sa[f], sb[f]), f
    # and the other direction: a gather read on the side stream sees the state after the steps
    with torch.cuda.stream(side):
        torch.cuda._sleep(5_000_000)
        x = T.gather(b, T.OBS_POS, dtype=torch.float64)
        y = x * 1.0
    side.synchronize()
    assert np.array_equal(y.cpu().numpy(), sa["x"])


@pytest.mark.gpu
def test_cpp_facade_gather_equals_pose_array(mrs):
    out = subprocess.run([build_cpp()], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    for tag in ("ok gather_equals_pose_array", "ok device_commands_equal_host_commands", "ok crashed_device"):
        assert tag in out.stdout, out.stdout
