"""State snapshots on the GPU (include/mrs_swarm.h, "state snapshots"; mrs_multirotor_simulator_amd.tensors save / load /
snapshot_fields): every record field equals the host getters bit for bit, a load rewinds a run with collision ticks (stalls included)
bit for bit, saving does not perturb a run, one record forks into many UAVs, edited records load as edited, skipped rows are reported
and left alone, records move between clones, bad arguments are error codes, the caller's stream is fenced, and the C++ facade
(tests/cpp/snapshot_test.cpp) agrees with the Python call.  Both kernel forms (MRS_SNAP_FORM=lane / tile) are covered where the
layout matters."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_device_io_gpu import DT, RANGES, build_cpp, mixed_swarm, torch_dev

FORMS = ["lane", "tile"]


def records_np(t):
    from mrs_multirotor_simulator_amd import swarm
    return np.ascontiguousarray(t.cpu().numpy()).view(swarm.SNAPSHOT_DTYPE).reshape(-1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """bit for bit (a -0.0 / 0.0 difference fails)"""
    return np.array_equal(bits(a), bits(b))


def host_view(g, first=0, count=None):
    s = g.get_states(first, count)
    return {"x": s["x"], "v": s["v"], "v_prev": s["v_prev"], "R": s["R"], "omega": s["omega"], "motor_rpm": s["motor_rpm"],
            "imu_acceleration": g.get_imu(first, count), "external_force": g.get_external_force(first, count), "pid": g.get_pid(first, count),
            "crashed": g.has_crashed(first, count)}


def assert_same_swarm(a, b, what=""):
    ha, hb = host_view(a), host_view(b)
    for f in ha:
        da, db = bits(ha[f]).reshape(len(ha[f]), -1), bits(hb[f]).reshape(len(hb[f]), -1)
        bad = np.flatnonzero((da != db).any(axis=1))
        assert len(bad) == 0, f"{what}: {f} differs for {len(bad)} UAVs, first {bad[:8]}"
    # the IMU of get_states too (the same column through another kernel)
    assert same(a.get_states()["imu_acceleration"], b.get_states()["imu_acceleration"]), what


def fields_swarm(mrs, arith=None):
    """the mixed x500 / f550 swarm after ticks with collisions, a few crashes, a v_prev split, external forces and varied spawn heights"""
    n = 3000
    rng = np.random.default_rng(11)
    spawn = np.stack([4.0 * (np.arange(n) % 50), 4.0 * (np.arange(n) // 50), rng.uniform(5.0, 15.0, n)], axis=1)
    g, st, rng = mixed_swarm(mrs, arith=arith, pos=spawn)
    cmd = np.concatenate([st["x"] + rng.uniform(-3, 3, (n, 3)), rng.uniform(-3, 3, (n, 1))], axis=1)
    g.set_input(0, n, mrs.POSITION_CMD, cmd)
    g.tick_n(DT, 30, True, False, 100.0)
    g.apply_force(200, 20, rng.uniform(-2, 2, (20, 3)))
    g.step_n(DT, 2)
    g.apply_force(1490, 20, rng.uniform(-2, 2, (20, 3)))  # (latched force across the airframe boundary)
    g.crash(60, 10)
    g.crash(n - 20, 5)
    g.set_state(70, 4, None, np.ones((4, 3)), None, None, None)  # v_prev split from v
    return g, spawn


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_record_fields_equal_the_host_getters(mrs, monkeypatch, form):
    from mrs_multirotor_simulator_amd import tensors as T
    monkeypatch.setenv("MRS_SNAP_FORM", form)
    g, spawn = fields_swarm(mrs)
    n, h = g.n, g.n // 2
    full = records_np(T.save(g))
    hv = host_view(g)
    assert np.abs(hv["external_force"]).max() > 0 and np.abs(hv["imu_acceleration"]).max() > 0 and hv["crashed"].sum() == 15
    assert (hv["v_prev"][70:74] != hv["v"][70:74]).all()
    air = full["airframe"]
    assert (air[:h] == air[0]).all() and (air[h:] == air[h]).all() and air[0] != air[h]
    assert (full["magic"] == T.SNAP_MAGIC).all() and (full["_reserved"] == 0).all()
    for first, count in RANGES + ((n - 37, 37), (0, n)):
        r = full[first:first + count] if count == n else records_np(T.save(g, first, count))
        sl = slice(first, first + count)
        for f in ("x", "v", "v_prev", "omega", "motor_rpm", "imu_acceleration", "external_force", "pid"):
            assert same(r[f], hv[f][sl]), (form, first, count, f)
        assert same(r["R"].reshape(count, 9), hv["R"][sl].reshape(count, 9)), (form, first, count)
        assert same(r["initial_z"], spawn[sl, 2]), (form, first, count)
        assert np.array_equal((r["flags"] & T.SNAP_CRASHED) != 0, hv["crashed"][sl] != 0), (form, first, count)
        split = np.zeros(n, bool)
        split[70:74] = True
        assert np.array_equal((r["flags"] & T.SNAP_VPREV_SPLIT) != 0, split[sl]), (form, first, count)
        assert np.array_equal(r["airframe"], air[sl]) and (r["magic"] == T.SNAP_MAGIC).all() and (r["flags"] & np.uint32(0xFFFFFFF8) == 0).all()
        for k in range(0, count, max(1, count // 7)):
            assert bool(r["flags"][k] & T.SNAP_TAKEOFF) == bool(g.get_params(first + k).takeoff_patch_enabled), (form, first + k)


def stall_swarm(mrs, n, seed, arith, v_fast=170.0, n_fast=8):
    """the stall recipe of test_device_io_gpu._stall_pair with a choice of arithmetic"""
    import bench
    st, cmd = bench.make_inputs(n, "position+collisions", seed=seed, volume_per_uav=16.0)
    st["v"][:n_fast] = [0.0, v_fast, 0.0]
    g = mrs.Swarm(n, arith=arith)
    g.construct(0, n, mrs.model_params("x500", ground_enabled=True, ground_z=0.0))
    g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    g.set_input(0, n, mrs.POSITION_CMD, cmd)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("crash", [False, True])
@pytest.mark.parametrize("arith", ["FAST", "LITERAL"])
def test_load_rewinds_a_run_with_collisions(mrs, arith, crash):
    """save, 200 collision ticks -> A; load every UAV, the same 200 ticks -> B: A == B bit for bit.  The fast UAVs of the stall recipe
    leave their skin in both runs, so the lazily evaluated ticks stall and replay (fused_stats); in crash mode the saved crash flags
    come back.  B also equals a clone of the swarm taken at the save and run the same 200 ticks: the load restores exactly what the
    library would continue from.

    FAST arithmetic with elastic collisions: the swarm that goes on after the save steps its first tick as a fused launch (the lists
    are live), a swarm whose positions were just written (load, or any host write; a clone) as a plain one, and in FAST arithmetic the
    two forms differ in the last bits for UAVs in contact (MEASUREMENTS §7.4).  There B is held to the clone; A itself is compared in
    every other case."""
    from mrs_multirotor_simulator_amd import tensors as T
    g = stall_swarm(mrs, 20_000, seed=23, arith=getattr(mrs, f"ARITH_{arith}"))
    g.tick_n(DT, 5, True, crash, 100.0)
    g.crash(100, 5)
    rec = T.save(g)
    ref = g.clone()  # the state at the save
    stalls0 = g.fused_stats()[1]
    g.tick_n(DT, 200, True, crash, 100.0)
    a = g.clone()
    stalls_a = g.fused_stats()[1] - stalls0
    status = T.load(g, rec)
    assert (status.cpu().numpy() == T.SNAP_LOADED).all()
    assert_same_swarm(g, ref, f"{arith} crash={crash}: right after the load")
    stalls1 = g.fused_stats()[1]
    g.tick_n(DT, 200, True, crash, 100.0)
    stalls_b = g.fused_stats()[1] - stalls1
    ref.tick_n(DT, 200, True, crash, 100.0)
    assert_same_swarm(g, ref, f"{arith} crash={crash}: after 200 ticks, against the clone of the save")
    if arith == "LITERAL" or crash:
        assert_same_swarm(a, g, f"{arith} crash={crash}: after 200 ticks")
    fused = g.fused_stats()[0]
    print(f"rewind {arith} crash={crash}: {stalls_a} / {stalls_b} stalls, {fused} fused launches")
    assert stalls_a >= 1 and stalls_b >= 1, (stalls_a, stalls_b)
    assert g.has_crashed()[100:105].all()
    for s in (a, ref):
        s.close()


@pytest.mark.gpu
def test_saving_does_not_perturb_a_run(mrs):
    from mrs_multirotor_simulator_amd import tensors as T
    a = stall_swarm(mrs, 20_000, seed=29, arith=mrs.ARITH_FAST)
    b = a.clone()
    rec = None
    for t in range(0, 200, 10):
        a.tick_n(DT, 10, True, True, 100.0)
        b.tick_n(DT, 10, True, True, 100.0)
        rec = T.save(b, out=rec)
    assert_same_swarm(a, b, "save every 10 ticks")
    assert b.fused_stats()[1] >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_fork_one_record_into_many_slots(mrs, monkeypatch, form):
    """record r loaded into 256 slots through an index (-1 elsewhere): the -1 slots are untouched, the forks equal the source UAV after
    N ticks under its command, and diverge under different commands (collisions off)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    monkeypatch.setenv("MRS_SNAP_FORM", form)
    n, K, src = 1000, 256, 5
    g, st, rng = mixed_swarm(mrs, n=n, seed=3)  # x500 in [0, 500)
    cmd = np.concatenate([st["x"] + rng.uniform(-3, 3, (n, 3)), rng.uniform(-3, 3, (n, 1))], axis=1)
    g.set_input(0, n, mrs.POSITION_CMD, cmd)
    g.step_n(DT, 500)  # (past the saturated start of the random flight state: below, nearby commands must not saturate the controllers)
    dev = torch_dev(g)
    rec = T.save(g, src, 1)
    slots = np.arange(100, 100 + K)  # x500 slots
    index = torch.full((n,), -1, dtype=torch.int32, device=dev)
    index[100:100 + K] = 0
    before = host_view(g)
    status = T.load(g, rec, index=index).cpu().numpy()
    assert (status[slots] == T.SNAP_LOADED).all() and (np.delete(status, slots) == T.SNAP_SKIPPED).all()
    after = host_view(g)
    for f in before:
        assert same(np.delete(after[f], slots, axis=0), np.delete(before[f], slots, axis=0)), f"-1 slots: {f}"
        assert same(after[f][slots], np.repeat(before[f][src:src + 1], K, axis=0)), f"forks: {f}"
    # the same command as the source: the forks follow it bit for bit
    g.set_input(100, K, mrs.POSITION_CMD, np.repeat(cmd[src:src + 1], K, axis=0))
    g.step_n(DT, 300)
    h = host_view(g)
    for f in h:
        assert same(h[f][slots], np.repeat(h[f][src:src + 1], K, axis=0)), f"forks after 300 steps: {f}"
    assert not same(h["x"][src], before["x"][src])
    # different sampled commands: they diverge
    cmds = np.repeat(cmd[src:src + 1], K, axis=0) + np.concatenate([rng.normal(0, 0.5, (K, 3)), np.zeros((K, 1))], axis=1)
    T.load(g, rec, index=index)
    g.set_input(100, K, mrs.POSITION_CMD, cmds)
    g.step_n(DT, 500)
    x = g.get_states()["x"][slots]
    assert len(np.unique(x, axis=0)) == K, len(np.unique(x, axis=0))
    assert np.linalg.norm(x - h["x"][src], axis=1).min() > 1e-3


@pytest.mark.gpu
def test_edited_records_load_as_edited(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, _ = fields_swarm(mrs)
    n = g.n
    rec = T.save(g)
    saved = records_np(rec)
    f = T.snapshot_fields(rec)
    off = torch.tensor([10.0, -20.0, 3.5], dtype=torch.float64, device=rec.device)
    f["x"] += off
    g.step_n(DT, 10)
    assert (T.load(g, rec).cpu().numpy() == 0).all()
    got = records_np(T.save(g))
    want = saved.copy()
    want["x"] += np.array([10.0, -20.0, 3.5])
    assert not same(want["x"], saved["x"])
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))  # translated positions, every other byte as saved
    assert same(g.get_states()["x"], want["x"])
    assert len(got) == n


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_skipped_rows_are_reported_and_untouched(mrs, monkeypatch, form):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    monkeypatch.setenv("MRS_SNAP_FORM", form)
    g, _ = fields_swarm(mrs)
    n, h = g.n, g.n // 2
    dev = torch_dev(g)
    rec = T.save(g)  # x500 records in [0, h), f550 in [h, n)
    g.step_n(DT, 5)
    before = host_view(g)
    flags_before = records_np(T.save(g))["flags"]
    # rows 0 .. 199 of the range [1400, 1600): record 2000 (f550) for all; index -1, n and -7 in a few rows; zeroed records for others
    zeroed = torch.zeros((10, T.SNAP_BYTES), dtype=torch.uint8, device=dev)
    both = torch.cat([rec, zeroed])  # records n .. n + 9 are zero
    idx = np.full(200, 2000, np.int32)
    idx[3], idx[150], idx[151], idx[152], idx[160], idx[161] = -1, n + 10, -7, -1, n + 2, n + 9
    status = T.load(g, both, first=1400, index=torch.tensor(idx, device=dev)).cpu().numpy()
    want = np.where(np.arange(1400, 1600) < h, T.SNAP_BAD_AIRFRAME, T.SNAP_LOADED).astype(np.uint8)
    want[3] = want[152] = T.SNAP_SKIPPED
    want[150] = want[151] = T.SNAP_BAD_INDEX
    want[160] = want[161] = T.SNAP_BAD_MAGIC
    assert np.array_equal(status, want), np.flatnonzero(status != want)
    after = host_view(g)
    skipped = 1400 + np.flatnonzero(want != T.SNAP_LOADED)
    loaded = 1400 + np.flatnonzero(want == T.SNAP_LOADED)
    assert len(loaded) > 0 and len(skipped) > 100
    for f in before:
        assert same(after[f][skipped], before[f][skipped]), f
        assert same(np.delete(after[f], np.arange(1400, 1600), axis=0), np.delete(before[f], np.arange(1400, 1600), axis=0)), f
    assert np.array_equal(records_np(T.save(g))["flags"][skipped], flags_before[skipped])
    s2000 = records_np(rec)[2000]
    got = records_np(T.save(g))[loaded]
    for name in ("x", "v", "pid", "external_force"):
        assert same(got[name], np.repeat(s2000[name][None], len(loaded), axis=0)), name
    # all-zero records without an index: every row status 4, nothing written
    st = T.load(g, torch.zeros((n, T.SNAP_BYTES), dtype=torch.uint8, device=dev)).cpu().numpy()
    assert (st == T.SNAP_BAD_MAGIC).all()
    assert same(g.get_states()["x"], after["x"])


@pytest.mark.gpu
def test_records_load_into_a_clone(mrs):
    from mrs_multirotor_simulator_amd import tensors as T
    g, _ = fields_swarm(mrs)
    c = g.clone()
    rec = T.save(g)
    g.step_n(DT, 20)
    c.tick_n(DT, 30, True, True, 100.0)  # the clone goes elsewhere, crashes included
    assert (T.load(c, rec).cpu().numpy() == T.SNAP_LOADED).all()
    back = g.clone()
    assert (T.load(back, rec).cpu().numpy() == T.SNAP_LOADED).all()
    assert_same_swarm(c, back, "records of a swarm loaded into its clone")
    assert np.array_equal(records_np(T.save(c)).view(np.uint8), records_np(rec).view(np.uint8))
    for s in (c, back):
        s.close()


@pytest.mark.gpu
def test_bad_arguments_are_error_codes(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, _, _ = mixed_swarm(mrs, n=300)
    dev = torch_dev(g)
    st = torch.cuda.current_stream(dev).cuda_stream
    x0 = g.get_states()["x"]
    rec = torch.zeros((301, T.SNAP_BYTES), dtype=torch.uint8, device=dev)
    host = np.zeros((300, T.SNAP_BYTES), np.uint8)
    with pytest.raises(mrs.MrsError, match="error 1:.*host memory|error 1:.*not device memory"):
        g.save_device(0, 300, host.ctypes.data, st)
    with pytest.raises(mrs.MrsError, match="error 1:.*host memory|error 1:.*not device memory"):
        g.load_device(0, 300, host.ctypes.data, 300, 0, 0, st)
    with pytest.raises(mrs.MrsError, match="error 1:.*16-B aligned"):
        g.save_device(0, 10, rec.data_ptr() + 8, st)
    with pytest.raises(mrs.MrsError, match="error 1:.*16-B aligned"):
        g.load_device(0, 10, rec.data_ptr() + 8, 10, 0, 0, st)
    with pytest.raises(mrs.MrsError, match="error 1:.*n_records < count"):
        g.load_device(0, 300, rec.data_ptr(), 299, 0, 0, st)
    # memory of the wrong size: one allocation of its own (a torch tensor may sit inside a larger cached block), as test_nearest_gpu does
    hip = C.CDLL("libamdhip64.so")
    small_p, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(small_p), C.c_size_t(31 * 4096)) == 0  # 256 records
    try:
        assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), small_p) == 0 and size.value < 300 * T.SNAP_BYTES
        small = small_p.value
        with pytest.raises(mrs.MrsError, match="error 1:.*dev_records: the rows extend past"):
            g.save_device(0, 300, small, st)
        with pytest.raises(mrs.MrsError, match="error 1:.*dev_records: the rows extend past"):
            g.load_device(0, 100, small + 31 * 4096 - 99 * T.SNAP_BYTES, 100, 0, 0, st)
        with pytest.raises(mrs.MrsError, match="error 1:.*dev_index: the rows extend past"):
            g.load_device(0, 20, rec.data_ptr(), 301, small + 31 * 4096 - 40, 0, st)
        with pytest.raises(mrs.MrsError, match="error 1:.*dev_status: the rows extend past"):
            g.load_device(0, 20, rec.data_ptr(), 301, 0, small + 31 * 4096 - 10, st)
    finally:
        assert hip.hipFree(small_p) == 0
    with pytest.raises(mrs.MrsError, match="error 1:.*null pointer"):
        g.save_device(0, 300, 0, st)
    with pytest.raises(mrs.MrsError, match="error 3:"):
        g.save_device(200, 101, rec.data_ptr(), st)
    with pytest.raises(mrs.MrsError, match="error 3:"):
        g.load_device(-1, 10, rec.data_ptr(), 301, 0, 0, st)
    if torch.cuda.device_count() > 1:
        other = torch.zeros((300, T.SNAP_BYTES), dtype=torch.uint8, device=torch.device("cuda", (g.device() + 1) % torch.cuda.device_count()))
        with pytest.raises(mrs.MrsError, match="error 1:.*memory of device"):
            g.save_device(0, 300, other.data_ptr(), st)
    assert np.array_equal(g.get_states()["x"], x0)
    assert np.count_nonzero(rec.cpu().numpy()) == 0  # nothing was launched
    T.save(g, out=rec[:300])
    g.step_n(DT, 2)
    assert np.isfinite(g.get_states()["x"]).all()


@pytest.mark.gpu
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
    rec = torch.zeros((100, T.SNAP_BYTES), dtype=torch.uint8, device=dev)
    for g in shards:
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.save(g, out=rec)
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.load(g, rec)
    assert np.count_nonzero(rec.cpu().numpy()) == 0
    for g in shards:
        g.close()
    group.close()


@pytest.mark.gpu
def test_caller_stream_is_fenced(mrs):
    """the records are written on a side stream kept busy by a long sleep; load called with that stream as the current one must read
    the written records, not the zeros that were there before"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, _ = fields_swarm(mrs)
    dev = torch_dev(g)
    src = T.save(g)
    want = host_view(g)
    g.step_n(DT, 20)
    rec = torch.zeros_like(src)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        rec.copy_(src)
        status = T.load(g, rec)
    side.synchronize()
    assert (status.cpu().numpy() == T.SNAP_LOADED).all()
    got = host_view(g)
    for f in want:
        assert same(got[f], want[f]), f
    # and the other direction: a save read on the side stream holds the state after the steps
    g.step_n(DT, 5)
    with torch.cuda.stream(side):
        torch.cuda._sleep(5_000_000)
        out = T.save(g)
        copy = out.clone()
    side.synchronize()
    assert same(records_np(copy)["x"], g.get_states()["x"])


@pytest.mark.gpu
def test_cpp_facade_equals_python(mrs):
    from mrs_multirotor_simulator_amd import tensors as T
    n = 1000
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "snapshot.bin")
        out = subprocess.run([build_cpp("snapshot_test"), path], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok save_equals_pose_array", "ok load_restores_the_save", "ok fork_through_index", "ok written"):
            assert tag in out.stdout, out.stdout
        raw = np.fromfile(path, np.uint8)
    i = np.arange(n)
    pos = np.stack([4.0 * (i % 32), 4.0 * (i // 32), np.zeros(n)], axis=1)
    cmd = np.stack([4.0 * (i % 32) + 1.0, 4.0 * (i // 32) - 0.5, 2.0 + 0.002 * i, 0.001 * i - 0.5], axis=1)
    p = mrs.default_params()
    p.ground_enabled = 1
    p.ground_z = 0.0
    g = mrs.Swarm(n, arith=mrs.ARITH_FAST)  # (the facade's default)
    g.construct(0, n, p, pos, 0.003 * i)
    g.set_input(0, n, mrs.POSITION_CMD, cmd)
    g.step_n(DT, 150)
    mine = T.save(g).cpu().numpy().reshape(-1)
    assert raw.shape == mine.shape and np.array_equal(raw, mine)
