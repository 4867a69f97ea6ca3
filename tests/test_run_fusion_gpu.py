"""Fused plain step runs ("State in registers inside a run"): step_n(dt, K, 1) on a swarm without cascade modes and without
mixed-airframe blocks issues ceil(K / D) launches of up to D steps each, with x, v, R, omega and rpm in registers between the steps of
a launch.  Nothing a caller can see may change: the fused run is held against K single step(dt) calls and against the same run with
MRS_RUN_FUSION=0 (one launch per step), from identical seeded inputs, with numpy.array_equal on the bit patterns of get_state,
get_imu, every field of get_outputs, the PID state and the flags a caller can read (crashed, take-off patch) — in both flavours."""
import numpy as np
import pytest

from helpers import random_state
from step_regimes import N_BUF_LAST, N_W3_FIRST  # 131 072 UAVs (2048 full blocks) and 131 073 (2049 blocks, a one-lane tail block)

pytestmark = pytest.mark.gpu
DT = 0.001
D = 4  # steps per fused launch (MRS_FUSE_MAX, the library's default depth)
N_SPLIT = 66_000  # 1032 blocks of 64 (the last one ragged): runs of four or more launches take the two-stream form
KS = (1, 2, 3, D, D + 1, 2 * D + 1, 4 * D + 3)  # single step, remainder launches of every depth, and (4D+3: five launches) the split form
ARITHS = ["literal", "fast"]
N_BUF = 122_000  # 1907 blocks: above the size up to which FAST launches the non-temporal (*_nt) kernels
# The fused kernels step_device.inc compiles and the cases of this file that force them (the launcher takes the *_nt ones for FAST swarms of
# up to 1900 blocks, the others for LITERAL and for larger FAST swarms; depth D for full launches, 2 .. D-1 for remainders).
# The single-step kernel they are held against changes once more on the way: the two-wave *_buf up to 2048 blocks ([122000-fast],
# [131072-fast]), the three-wave *_buf_w3 above ([131073-fast]: the pairing of the 1 M benchmark leg; the same pair on three blocks
# in test_step_regimes_gpu.py).  The sizes come from step_regimes.py, which test_step_regimes.py holds against the launcher's rule.
# tests/test_run_fusion_table.py holds this table against the source.
_BUF_CASES = ["test_fused_runs_equal_single_steps[1000-literal]", "test_fused_runs_equal_single_steps[122000-fast]",
              "test_fused_runs_equal_single_steps[131072-fast]", "test_fused_runs_equal_single_steps[131073-fast]"]
FUSED_KERNELS = {
    "mrs_uav_model_step_buf_nt_fuse2": ["test_fused_runs_equal_single_steps[1000-fast]"],
    "mrs_uav_model_step_buf_nt_fuse3": ["test_fused_runs_equal_single_steps[1000-fast]"],
    "mrs_uav_model_step_buf_nt_fuse4": ["test_fused_runs_equal_single_steps[1000-fast]"],
    "mrs_uav_model_step_buf_fuse2": list(_BUF_CASES),
    "mrs_uav_model_step_buf_fuse3": list(_BUF_CASES),
    "mrs_uav_model_step_buf_fuse4": list(_BUF_CASES),
}


@pytest.fixture(scope="module")
def M(mrs):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return mrs


def arith_of(M, name):
    return M.ARITH_FAST if name == "fast" else M.ARITH_LITERAL


def launches(k, depth=D):
    """launches of a plain run of k steps: full ones, then one launch of the remainder"""
    return (k + depth - 1) // depth if depth else k


def view(g, flags_of=()):
    out = dict(g.get_state())
    out["imu"] = g.get_imu()
    o = g.get_outputs()
    for f in o.dtype.names:
        out["out." + f] = o[f]
    out["pid"] = g.get_pid()
    out["crashed"] = g.has_crashed()
    out["fext"] = g.get_external_force()
    out["takeoff"] = np.array([g.get_params(i).takeoff_patch_enabled for i in flags_of], dtype=np.int32)
    return out


def same(x, y):
    """numpy.array_equal on the bit patterns (a NaN equals itself, -0.0 differs from 0.0)"""
    if x.dtype == np.float64:
        x, y = np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)
    elif x.dtype == np.float32:
        x, y = np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)
    return np.array_equal(x, y)


def assert_same(a, b, what, flags_of=()):
    va, vb = view(a, flags_of), view(b, flags_of)
    bad = [k for k in va if not same(va[k], vb[k])]
    print(f"{what}: fields that differ: {bad or 'none'}")
    assert not bad, f"{what}: {bad} differ"
    return va


def swarms(M, monkeypatch, n, arith, seed, fusion=(None, None, "0"), takeoff=False, setup=None, inputs=None):
    """swarms with identical seeded state and actuator commands (inputs(g, act): the caller sets them); fusion[j]: MRS_RUN_FUSION of
    swarm j (read when it is created)"""
    rng = np.random.default_rng(seed)
    st = random_state(rng, n, 4)
    act = rng.uniform(0.35, 0.60, (n, 4))
    out = []
    for f in fusion:
        if f is None:
            monkeypatch.delenv("MRS_RUN_FUSION", raising=False)
        else:
            monkeypatch.setenv("MRS_RUN_FUSION", f)
        g = M.Swarm(n, arith=arith)
        g.construct(0, n, M.model_params("x500", ground_enabled=True, ground_z=0.0, takeoff_patch_enabled=takeoff), st["x"], np.zeros(n))
        if setup:
            setup(g, st)
        g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
        if inputs:
            inputs(g, act)
        else:
            g.set_input(0, n, M.ACTUATOR_CMD, act)
        out.append(g)
    monkeypatch.delenv("MRS_RUN_FUSION", raising=False)
    return out


def run_all(a, b, c, k):
    """a: one fused run of k steps; b: k single steps; c: the run with one launch per step"""
    a.step_n(DT, k)
    for _ in range(k):
        b.step(DT)
    c.step_n(DT, k)


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("fleet", ["f550", "naki", "x500+f550+naki"])
def test_fused_runs_equal_single_steps_with_six_and_eight_motors(M, monkeypatch, arith, fleet):
    """Six- and eight-motor airframes: the rpm of the first four motors is carried in registers, the rpm of the others goes through its
    columns every step - a path no other kernel has.  The three-airframe fleet changes type at block borders (UAV 320 and 640), so
    every block is a single-type block of its own motor count and the run is fused."""
    n = 1000
    parts = {"f550": [(0, n, "f550", 6)], "naki": [(0, n, "naki", 8)],
             "x500+f550+naki": [(0, 320, "x500", 4), (320, 320, "f550", 6), (640, n - 640, "naki", 8)]}[fleet]
    rng = np.random.default_rng(91)
    st = random_state(rng, n, 8)
    for first, count, _, nm in parts:
        st["motor_rpm"][first:first + count, nm:] = 0.0
    thr = rng.uniform(0.35, 0.60, (n, 8))

    def setup(g, _):
        for first, count, name, _ in parts:
            g.construct(first, count, M.model_params(name, ground_enabled=True, ground_z=0.0), st["x"][first:first + count], np.zeros(count))
        g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])

    def inputs(g, _):
        g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])  # (after swarms() has set its four-motor state)
        for first, count, _, nm in parts:
            g.set_input(first, count, M.ACTUATOR_CMD, thr[first:first + count, :nm])

    a, b, c = swarms(M, monkeypatch, n, arith_of(M, arith), 92, setup=setup, inputs=inputs)
    a.set_profiling(1)
    for k in (2, 3, D, 2 * D + 1):
        run_all(a, b, c, k)
        v = assert_same(a, b, f"{fleet}, K={k}, {arith}: fused run vs single steps")
        assert_same(a, c, f"{fleet}, K={k}, {arith}: fused run vs MRS_RUN_FUSION=0")
        assert a.last_step_kernel_ms()[1] == launches(k), (k, a.last_step_kernel_ms())
    for first, count, _, nm in parts:  # (the scenario: every motor the airframe has is spinning, and none beyond)
        assert np.all(v["motor_rpm"][first:first + count, :nm] > 0) and np.all(v["motor_rpm"][first:first + count, nm:] == 0)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("n", [37, 64, 1000, N_SPLIT, N_BUF, N_BUF_LAST, N_W3_FIRST])
def test_fused_runs_equal_single_steps(M, monkeypatch, arith, n):
    """tail lanes and one stream (n = 37, 64, 1000), two streams (1032 blocks; 1907 blocks, where FAST leaves the *_nt kernels; 2048
    full blocks, the last size at which a FAST step() is the two-wave *_buf kernel; 2049 blocks with a one-lane tail block, where it
    is the three-wave *_buf_w3 and the fused launch stays the two-wave *_buf_fuseD);
    K = 1, 2, 3, D, D+1, 2D+1, 4D+3 one after the other on the same three swarms: every remainder depth, the single-step remainder, and
    from 1024 blocks on the switch to the two-stream form"""
    a, b, c = swarms(M, monkeypatch, n, arith_of(M, arith), 11 + n)
    a.set_profiling(1)
    c.set_profiling(1)
    for k in KS:
        run_all(a, b, c, k)
        v = assert_same(a, b, f"n={n}, K={k}, {arith}: fused run vs single steps")
        assert_same(a, c, f"n={n}, K={k}, {arith}: fused run vs MRS_RUN_FUSION=0")
        assert np.all(np.isfinite(v["imu"])) and np.abs(v["imu"]).max() > 0
        assert a.last_step_kernel_ms()[1] == launches(k) and c.last_step_kernel_ms()[1] == k, (k, a.last_step_kernel_ms(), c.last_step_kernel_ms())
    if n >= N_SPLIT:  # 4D+3 steps: five fused launches -> the two-stream form, counted in steps
        assert a.split_stats()[0] == 4 * D + 3, a.split_stats()
        assert c.split_stats()[0] == sum(k for k in KS if k >= 4), c.split_stats()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("n", [1000, N_SPLIT, N_BUF_LAST, N_W3_FIRST])
def test_hold_vprev_takeoff_ground_force_and_crash(M, monkeypatch, arith, n):
    """UAVs on hold keep state and IMU; set_state right before the run (v_prev split); the take-off patch and the ground clamp UAVs
    first in the SECOND step of the fused launch; an external force; crashed UAVs"""
    z_above = 1.5e-3  # with v_z = -1 m/s and dt = 1 ms: still above the clamp height after one step, below it after two

    def setup(g, st):  # UAVs 600 .. 663 (block 9 and the start of block 10): no take-off patch, so that the ground is what clamps them
        g.construct(600, 70, M.model_params("x500", ground_enabled=True, ground_z=0.0, takeoff_patch_enabled=False), st["x"][600:670], np.zeros(70))

    a, b, c = swarms(M, monkeypatch, n, arith_of(M, arith), 21, takeoff=True, setup=setup)
    rng = np.random.default_rng(22)
    hold, split, patch, ground, forced, crashed = slice(200, 330), slice(400, 490), slice(0, 150), slice(600, 670), slice(700, 800), slice(820, 900)
    flags_of = range(0, 150, 7)
    v_new, force = rng.normal(0, 2, (90, 3)), rng.normal(0, 3, (100, 3))
    for g in (a, b, c):
        g.step_n(DT, 3)  # every UAV has an IMU value and v_prev == v
    imu_before, st_before = a.get_imu(), a.get_state()
    for g in (a, b, c):
        g.set_hold(hold.start, hold.stop - hold.start, True)
        g.set_state(split.start, 90, None, v_new, None, None, None)  # v replaced, v_prev kept
        for sl in (patch, ground):  # idle motors, sinking: the patch group sits below its spawn height, the ground group just above z = 0
            cnt = sl.stop - sl.start
            st = g.get_state(sl.start, cnt)
            if sl is ground:
                st["x"][:, 2] = z_above
            st["v"][:] = [0.0, 0.0, -1.0]
            g.set_state(sl.start, cnt, st["x"], st["v"], st["R"], np.zeros((cnt, 3)), np.zeros((cnt, 8)))
            g.set_input(sl.start, cnt, M.ACTUATOR_CMD, np.zeros((cnt, 4)))
        g.apply_force(forced.start, 100, force)
        g.crash(crashed.start, 80)
    # (the scenario, seen on the single-step swarm: one step of a twin — the ground group is still falling after it, at rest after two)
    probe = b.clone()
    probe.step(DT)
    assert np.all(probe.get_state()["v"][ground][:, 2] < 0) and np.all(probe.get_state()["x"][ground][:, 2] > 0)
    probe.step(DT)
    assert np.all(probe.get_state()["v"][ground] == 0) and np.all(probe.get_state()["x"][ground][:, 2] == 0)
    run_all(a, b, c, 2 * D + 1)
    v = assert_same(a, b, f"cases, n={n}, {arith}: fused run vs single steps", flags_of)
    assert_same(a, c, f"cases, n={n}, {arith}: fused run vs MRS_RUN_FUSION=0", flags_of)
    assert np.array_equal(v["imu"][hold], imu_before[hold]), "a UAV on hold must keep its IMU over a fused run"
    for k in ("x", "v", "R", "omega", "motor_rpm"):
        assert np.array_equal(v[k][hold], st_before[k][hold]), f"a UAV on hold must keep {k}"
    assert np.all(v["crashed"][crashed] == 1) and np.abs(v["fext"][forced]).min() > 0
    assert np.array_equal(v["v"][split], v["v_prev"][split])
    for g in (a, b, c):
        g.set_hold(hold.start, hold.stop - hold.start, False)
    run_all(a, b, c, D + 2)
    v2 = assert_same(a, b, "after the release", flags_of)
    assert_same(a, c, "after the release, MRS_RUN_FUSION=0", flags_of)
    assert (v2["imu"][hold] != imu_before[hold]).any(axis=1).mean() > 0.25


@pytest.mark.parametrize("arith", ARITHS)
def test_takeoff_patch_clamps_first_in_the_second_step_of_a_launch(M, monkeypatch, arith):
    """UAVs under the take-off patch, idle motors, sinking from 1.5 mm above their spawn height at 1 m/s: free after the first step
    of the fused launch, clamped by its second"""
    n = 300
    a, b, c = swarms(M, monkeypatch, n, arith_of(M, arith), 31, takeoff=True)
    for g in (a, b, c):
        st = g.get_state(0, 150)
        st["x"][:, 2] += 1.5e-3  # (spawned at st["x"]: the patch holds a UAV at its spawn height)
        st["v"][:] = [0.0, 0.0, -1.0]
        g.set_state(0, 150, st["x"], st["v"], st["R"], np.zeros((150, 3)), np.zeros((150, 8)))
        g.set_input(0, 150, M.ACTUATOR_CMD, np.zeros((150, 4)))
    z0 = a.get_state(0, 150)["x"][:, 2] - 1.5e-3
    probe = b.clone()
    probe.step(DT)
    assert np.all(probe.get_state(0, 150)["v"][:, 2] < 0) and np.all(probe.get_state(0, 150)["x"][:, 2] > z0)
    probe.step(DT)
    assert np.all(probe.get_state(0, 150)["v"] == 0) and np.all(np.abs(probe.get_state(0, 150)["x"][:, 2] - z0) < 1e-12)
    for k in (D, 3):
        run_all(a, b, c, k)
        assert_same(a, b, f"take-off patch, K={k}, {arith}: fused run vs single steps", range(0, 300, 7))
        assert_same(a, c, f"take-off patch, K={k}, {arith}: fused run vs MRS_RUN_FUSION=0", range(0, 300, 7))
    assert any(a.get_params(i).takeoff_patch_enabled for i in range(150)) and not all(a.get_params(i).takeoff_patch_enabled for i in range(300))


@pytest.mark.parametrize("arith", ARITHS)
def test_nan_first_in_a_later_step_of_a_fused_launch(M, monkeypatch, arith):
    """body rates of 1e150 rad/s, as test_nan_rollback_inside_a_fused_launch builds them: R^T R overflows a few steps in -> NaN
    derivatives -> the UAV is rolled back to the start of THAT step, which inside a fused launch only the kernel still has"""
    n, wild = 192, [7, 70, 130]
    rng = np.random.default_rng(61)
    st = random_state(rng, n, 4)
    st["omega"][7] = [1e150, 0.0, 0.0]
    st["omega"][70] = [0.0, 3e151, 1e150]
    st["omega"][130] = [1e100, 1e100, 1e100]
    a, b, c = swarms(M, monkeypatch, n, arith_of(M, arith), 62)
    for g in (a, b, c):
        g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    counts = []
    for _ in range(3 * D):
        b.step(DT)
        counts.append(b.get_diag()["nan_rollback"])
    first = int(np.argmax(np.asarray(counts) > 0))
    assert counts[-1] > 0 and first > 0, counts
    lead = 1 if first % D == 0 else 0  # the first rollback must not fall on the first step of a fused launch
    for g in (a, c):
        if lead:
            g.step(DT)
        g.step_n(DT, 3 * D - lead)
    assert (first - lead) % D != 0
    assert a.get_diag()["nan_rollback"] == c.get_diag()["nan_rollback"] == counts[-1], (a.get_diag(), c.get_diag(), counts)
    v = assert_same(a, b, f"NaN rollback, {arith}: fused run vs single steps")
    assert_same(a, c, f"NaN rollback, {arith}: fused run vs MRS_RUN_FUSION=0")
    clean = np.ones(n, bool)
    clean[wild] = False
    assert np.all(np.isfinite(v["x"][clean]))


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("n", [1000, N_SPLIT, N_BUF_LAST, N_W3_FIRST])
def test_run_directly_after_a_collision_tick(M, monkeypatch, arith, n):
    """the first step of the run carries the collision tick and stays a launch of its own, the rest fuse"""
    a, b, c = swarms(M, monkeypatch, n, arith_of(M, arith), 41)
    a.set_profiling(1)
    c.set_profiling(1)
    k = 2 * D + 2
    for g in (a, b, c):
        g.step_n(DT, 2)
        g.handle_collisions(True, False, 100.0)
    run_all(a, b, c, k)
    assert_same(a, b, f"after a collision tick, n={n}, {arith}: fused run vs single steps")
    assert_same(a, c, f"after a collision tick, n={n}, {arith}: fused run vs MRS_RUN_FUSION=0")
    assert a.last_step_kernel_ms()[1] == 1 + launches(k - 1) and c.last_step_kernel_ms()[1] == k, (a.last_step_kernel_ms(), c.last_step_kernel_ms())


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("n", [900, N_SPLIT, N_BUF_LAST, N_W3_FIRST])
def test_two_runs_back_to_back_then_a_single_step(M, monkeypatch, arith, n):
    a, b, c = swarms(M, monkeypatch, n, arith_of(M, arith), 51)
    seen = []
    for k in (4 * D + 1, D + 3):
        run_all(a, b, c, k)
        seen.append(assert_same(a, b, f"run of {k}, n={n}, {arith}: fused run vs single steps")["imu"])
        assert_same(a, c, f"run of {k}, n={n}, {arith}: fused run vs MRS_RUN_FUSION=0")
    for g in (a, b, c):
        g.step(DT)
    seen.append(assert_same(a, b, "runs followed by step()")["imu"])
    assert_same(a, c, "runs followed by step(), MRS_RUN_FUSION=0")
    for p, q in zip(seen, seen[1:]):
        assert (p != q).any(axis=1).mean() > 0.9, "the IMU must move from one comparison to the next"


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("case", ["mixed", "position"])
def test_swarms_that_do_not_qualify_take_the_launches_they_took(M, monkeypatch, arith, case):
    """mixed-airframe blocks, a UAV in a cascade mode: same bits and same launch count as MRS_RUN_FUSION=0"""
    n = 700

    def setup(g, st):
        if case == "mixed":  # six-motor airframes from the middle of block 1 to the middle of block 4
            g.construct(100, 200, M.model_params("f550", ground_enabled=True, ground_z=0.0), st["x"][100:300], np.zeros(200))
        for nm in ("set_mixer_params", "set_rate_params", "set_attitude_params", "set_velocity_params", "set_position_params"):
            getattr(g, nm)(0, n)

    six = np.random.default_rng(72).uniform(0.35, 0.60, (200, 6))

    def inputs(g, act):
        if case == "mixed":  # six throttles for the six-motor airframes: no UAV in a cascade mode, the mixed blocks alone keep the run unfused
            g.set_input(0, 100, M.ACTUATOR_CMD, act[:100])
            g.set_input(100, 200, M.ACTUATOR_CMD, six)
            g.set_input(300, n - 300, M.ACTUATOR_CMD, act[300:])
        else:  # one UAV of 700 follows a position reference
            g.set_input(0, n, M.ACTUATOR_CMD, act)
            g.set_input(5, 1, M.POSITION_CMD, np.array([[1.0, 2.0, 3.0, 0.5]]))

    a, b, c = swarms(M, monkeypatch, n, arith_of(M, arith), 71, setup=setup, inputs=inputs)
    a.set_profiling(1)
    c.set_profiling(1)
    k = 2 * D + 1
    run_all(a, b, c, k)
    assert_same(a, b, f"{case}, {arith}: run vs single steps")
    assert_same(a, c, f"{case}, {arith}: run vs MRS_RUN_FUSION=0")
    assert a.last_step_kernel_ms()[1] == c.last_step_kernel_ms()[1] == k, (a.last_step_kernel_ms(), c.last_step_kernel_ms())


@pytest.mark.parametrize("arith", ARITHS)
def test_depth_override_and_caller_given_substeps(M, monkeypatch, arith):
    """MRS_RUN_FUSION=2 and 3 choose the depth (tuning aid); substeps_per_launch > 1 keeps the *_multi kernels and their launch count"""
    n, k = 1000, 11
    a2, a3, b, c = swarms(M, monkeypatch, n, arith_of(M, arith), 81, fusion=("2", "3", None, "0"))
    for g in (a2, a3, c):
        g.set_profiling(1)
    a2.step_n(DT, k)
    a3.step_n(DT, k)
    for _ in range(k):
        b.step(DT)
    c.step_n(DT, k)
    assert_same(a2, b, f"depth 2, {arith}")
    assert_same(a3, b, f"depth 3, {arith}")
    assert_same(c, b, f"one launch per step, {arith}")
    assert a2.last_step_kernel_ms()[1] == launches(k, 2) and a3.last_step_kernel_ms()[1] == launches(k, 3) and c.last_step_kernel_ms()[1] == k
    a2.step_n(DT, 9, 3)
    assert a2.last_step_kernel_ms()[1] == 3
