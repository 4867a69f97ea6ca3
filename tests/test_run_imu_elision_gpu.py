"""Runs of steps skip the IMU stores nobody can read ("IMU columns inside a run"): inside one step_n(dt, K) call only the
last launch writes the three IMU columns; every launch before it has the stores switched off.  Nothing a caller can see may change:
step_n(dt, K) is held against K single step(dt) calls — which always write the IMU — from identical seeded inputs, with
numpy.array_equal on get_state, get_imu and every field of get_outputs, in every launch form a run can take (two streams, one
stream, ragged tail, mixed-airframe blocks, fused sub-steps, the position cascade), with UAVs on hold / under the take-off patch /
with a split v_prev, over runs back to back, against the CPU oracle, and through a snapshot."""
import numpy as np
import pytest

import helpers
from helpers import RTOL_FAST, RTOL_LITERAL, RTOL_NORTH_STAR, Pair, random_state
from step_regimes import N_BUF_LAST, N_CASCADE_BUF_FIRST, N_W3_FIRST, two_streams

pytestmark = pytest.mark.gpu
DT = 0.001
N_SPLIT = 66_000  # 1032 blocks of 64 (the last one ragged): runs of four or more launches take the two-stream form


@pytest.fixture(scope="module")
def M(mrs):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return mrs


def view(g):
    """everything the issue's comparison covers: get_state, get_imu and the packed outputs, field by field"""
    out = dict(g.get_state())
    out["imu"] = g.get_imu()
    o = g.get_outputs()
    for f in o.dtype.names:
        out["out." + f] = o[f]
    out["pid"] = g.get_pid()
    out["crashed"] = g.has_crashed()
    return out


def same(x, y):
    """numpy.array_equal on the bit patterns of floating-point arrays (a NaN equals itself, -0.0 differs from 0.0)"""
    if x.dtype == np.float64:
        x, y = np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)
    elif x.dtype == np.float32:
        x, y = np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)
    return np.array_equal(x, y)


def assert_same(a, b, what):
    va, vb = view(a), view(b)
    for k in va:
        print(f"{what}: {k}: equal = {same(va[k], vb[k])}")
    for k in va:
        assert same(va[k], vb[k]), f"{what}: {k} differs"
    return va


def assert_close_views(a, b, rtol, what):
    va, vb = view(a), view(b)
    for k in va:
        if va[k].dtype.kind == "f":
            e = helpers.rel_linf(va[k], vb[k])
            print(f"{what}: {k}: relative L-inf = {e:.3e}")
    for k in va:
        if va[k].dtype.kind == "f":
            helpers.assert_close(va[k], vb[k], rtol, f"{what}: {k}")
        else:
            assert np.array_equal(va[k], vb[k]), f"{what}: {k} differs"


def twin_swarms(M, n, arith, seed, workload="actuator", mixed=False, takeoff=False):
    """two swarms with identical seeded state and commands"""
    rng = np.random.default_rng(seed)
    st = random_state(rng, n, 4, tilted=(workload == "position"))
    act = rng.uniform(0.35, 0.60, (n, 4))
    goal = np.concatenate([st["x"] + rng.uniform(-5, 5, (n, 3)), rng.uniform(-3.14, 3.14, (n, 1))], axis=1)
    pair = []
    for _ in range(2):
        g = M.Swarm(n, arith=arith)
        g.construct(0, n, M.model_params("x500", ground_enabled=True, ground_z=0.0, takeoff_patch_enabled=takeoff), st["x"], np.zeros(n))
        if mixed:  # six-motor airframes from the middle of block 1 to the middle of block 4: blocks 1 and 4 hold two airframe types
            g.construct(100, 200, M.model_params("f550", ground_enabled=True, ground_z=0.0), st["x"][100:300], np.zeros(200))
        for nm in ("set_mixer_params", "set_rate_params", "set_attitude_params", "set_velocity_params", "set_position_params"):
            getattr(g, nm)(0, n)
        g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
        if workload == "position" or mixed:
            g.set_input(0, n, M.POSITION_CMD, goal)
        if workload == "actuator":
            lo = 300 if mixed else 0  # (an actuator row of four columns is too narrow for a six-motor airframe)
            g.set_input(lo, n - lo, M.ACTUATOR_CMD, act[lo:])
        pair.append(g)
    return pair


def run_both(a, b, k, sub=1):
    """a: one run of k steps; b: k single steps, each of which writes its IMU"""
    a.step_n(DT, k, sub)
    for _ in range(k):
        b.step(DT)


ARITHS = ["literal", "fast"]


def arith_of(M, name):
    return M.ARITH_FAST if name == "fast" else M.ARITH_LITERAL


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("split_env", [None, "0"])
def test_run_equals_single_steps_on_a_two_stream_swarm(M, monkeypatch, arith, split_env):
    """1032 blocks, K = 6: the two-stream form, and the same swarm with MRS_SPLIT_STREAMS=0 (one full-swarm launch per step)"""
    if split_env is not None:
        monkeypatch.setenv("MRS_SPLIT_STREAMS", split_env)  # read when the swarm is created
    a, b = twin_swarms(M, N_SPLIT, arith_of(M, arith), 1)
    run_both(a, b, 6)
    v = assert_same(a, b, f"two-stream swarm, split={split_env}, {arith}")
    assert np.abs(v["imu"]).min(axis=1).max() > 0 and np.all(np.isfinite(v["imu"]))


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("n,k", [(512, 5), (1000, 7), (37, 2), (64, 1)])
def test_run_equals_single_steps_on_one_stream(M, arith, n, k):
    """small swarms on a single stream; n = 1000 and n = 37 are no multiples of 64"""
    a, b = twin_swarms(M, n, arith_of(M, arith), 2 + n)
    run_both(a, b, k)
    assert_same(a, b, f"n={n}, K={k}, {arith}")


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("n", [700, N_SPLIT])
def test_run_equals_single_steps_with_mixed_airframe_blocks(M, arith, n):
    """blocks 1 and 4 hold two airframe types: the mixed-block launch rides with the first stream's launch of every step"""
    a, b = twin_swarms(M, n, arith_of(M, arith), 3, mixed=True)
    run_both(a, b, 5)
    v = assert_same(a, b, f"mixed blocks, n={n}, {arith}")
    assert np.abs(v["imu"][100:300]).max() > 0


@pytest.mark.parametrize("workload", ["actuator", "position"])
@pytest.mark.parametrize("k,sub", [(12, 4), (10, 4), (9, 2)])
def test_run_with_fused_substeps_literal_is_bit_identical(M, workload, k, sub):
    """substeps_per_launch > 1 (k = 10, sub = 4: launches of 4, 4 and 2 sub-steps; k = 9, sub = 2: five launches -> two streams at
    N_SPLIT)"""
    for n in (512, N_SPLIT):
        a, b = twin_swarms(M, n, M.ARITH_LITERAL, 4, workload=workload)
        run_both(a, b, k, sub)
        assert_same(a, b, f"literal, fused sub-steps {k}/{sub}, n={n}, {workload}")


@pytest.mark.parametrize("workload", ["actuator", "position"])
@pytest.mark.parametrize("k,sub", [(12, 4), (10, 4), (9, 2)])
def test_run_with_fused_substeps_fast_within_tolerance(M, workload, k, sub):
    """FAST: the fused kernels are other instantiations than the single-step ones and FMA contraction is the compiler's choice per
    instantiation — RTOL_FAST, as test_pointer_addressed_kernels_match_buffer_addressed_ones holds two FAST instantiations together"""
    for n in (512, N_SPLIT):
        a, b = twin_swarms(M, n, M.ARITH_FAST, 4, workload=workload)
        run_both(a, b, k, sub)
        assert_close_views(a, b, RTOL_FAST, f"fast, fused sub-steps {k}/{sub}, n={n}, {workload}")


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("n", [2048, N_SPLIT])
def test_run_equals_single_steps_position_cascade(M, arith, n):
    a, b = twin_swarms(M, n, arith_of(M, arith), 5, workload="position")
    run_both(a, b, 6)
    assert_same(a, b, f"position cascade, n={n}, {arith}")


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("workload,n", [("model", N_BUF_LAST), ("model", N_W3_FIRST), ("position", N_CASCADE_BUF_FIRST), ("position", N_W3_FIRST)])
def test_run_equals_single_steps_in_the_two_wave_and_three_wave_regimes(M, monkeypatch, arith, workload, n):
    """The kernels the cases above never run with MRS_OPT_IMU_DEAD set (sizes and regimes: step_regimes.py).  Model-only, 2048 full
    blocks and 2049 blocks with a one-lane tail, MRS_RUN_FUSION=0 at creation so that the run's launches are the single-step kernels:
    in FAST the two-wave *_model_step_buf and the three-wave *_model_step_buf_w3.  Position cascade (never fused), 901 blocks: FAST
    has left mrs_uav_step_buf_nt for mrs_uav_step_buf, on one stream; 2049 blocks: mrs_uav_step_buf_w3, on two.  K = 7: from 1024 blocks
    on the two-stream form.  Both sides of the comparison run the SAME instantiation, the run with the IMU stores of its first six
    launches switched off: bit identity is owed in both flavours.  One block of UAVs on hold keeps the IMU it had."""
    k = 7
    if workload == "model":
        monkeypatch.setenv("MRS_RUN_FUSION", "0")  # read when the swarm is created
    a, b = twin_swarms(M, n, arith_of(M, arith), 10, workload="actuator" if workload == "model" else "position")
    monkeypatch.delenv("MRS_RUN_FUSION", raising=False)
    hold = slice(4 * 64 - 3, 5 * 64 + 3)  # block 4 entirely, and three lanes of each neighbour
    for g in (a, b):
        g.step_n(DT, 3)  # every UAV has an IMU value now
        g.set_hold(hold.start, hold.stop - hold.start, True)
    imu_before, st_before = a.get_imu(), a.get_state()
    assert same(imu_before, b.get_imu()) and np.abs(imu_before[hold]).min(axis=1).max() > 0
    a.set_profiling(1)
    run_both(a, b, k)
    v = assert_same(a, b, f"{workload}, n={n}, K={k}, {arith}")
    assert a.last_step_kernel_ms()[1] == k, ("one launch per step", a.last_step_kernel_ms())
    assert a.split_stats()[0] == (k if two_streams(n, k) else 0), a.split_stats()
    assert same(v["imu"][hold], imu_before[hold]) and same(b.get_imu()[hold], imu_before[hold]), "a UAV on hold must keep its IMU over a run"
    for f in ("x", "v", "R", "omega", "motor_rpm"):
        assert same(v[f][hold], st_before[f][hold]), f"a UAV on hold must keep {f}"
    moved = np.ones(n, bool)
    moved[hold] = False
    assert np.all(np.isfinite(v["imu"])) and (v["imu"][moved] != imu_before[moved]).any(axis=1).mean() > 0.9  # (scenario sanity: the others are stepped)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("n", [1500, N_SPLIT])
def test_hold_takeoff_and_split_v_prev(M, arith, n):
    """UAVs on hold keep the IMU they had before the run; UAVs under the take-off patch and UAVs whose v was replaced by set_state
    (FLAG_VPREV_SPLIT: the IMU of their next step uses the kept v_prev) follow the stepwise form bit for bit"""
    a, b = twin_swarms(M, n, arith_of(M, arith), 6, takeoff=True)
    rng = np.random.default_rng(66)
    hold = slice(200, 330)  # crosses block borders, covers block 4 entirely
    for g in (a, b):
        # the first 150 sit below their spawn height with idle motors, sinking: the take-off patch clamps them (multirotor_model.hpp:264-277)
        st = g.get_state(0, 150)
        st["v"][:, 2] = -1.0
        g.set_state(0, 150, st["x"], st["v"], st["R"], st["omega"], np.zeros((150, 8)))
        g.set_input(0, 150, M.ACTUATOR_CMD, np.zeros((150, 4)))
        g.step_n(DT, 3)  # every UAV has an IMU value now
    imu_before = a.get_imu()
    assert np.array_equal(imu_before, b.get_imu()) and np.abs(imu_before[hold]).min(axis=1).max() > 0
    v_new = rng.normal(0, 2, (90, 3))
    for g in (a, b):
        g.set_hold(hold.start, hold.stop - hold.start, True)
        g.set_state(400, 90, None, v_new, None, None, None)  # v replaced, v_prev kept
        assert not np.array_equal(g.get_state()["v_prev"][400:490], g.get_state()["v"][400:490])
    run_both(a, b, 5)
    v = assert_same(a, b, f"hold / take-off / v_prev split, n={n}, {arith}")
    assert np.array_equal(v["imu"][hold], imu_before[hold]), "a UAV on hold must keep its IMU over a run"
    assert np.array_equal(b.get_imu()[hold], imu_before[hold])
    moved = np.ones(n, bool)
    moved[hold] = False
    # (sanity of the scenario, not a bound on the code: the run must have moved the IMU of the UAVs in free flight — one that the
    #  take-off patch clamps at rest, up to half of a swarm with random throttles, may repeat its value)
    assert (v["imu"][moved] != imu_before[moved]).any(axis=1).mean() > 0.25
    assert [a.get_params(i).takeoff_patch_enabled for i in range(0, 150, 7)] == [b.get_params(i).takeoff_patch_enabled for i in range(0, 150, 7)]
    assert any(a.get_params(i).takeoff_patch_enabled for i in range(150)), "some UAVs should still be under the take-off patch"
    # released again: the next run steps them and writes their IMU
    for g in (a, b):
        g.set_hold(hold.start, hold.stop - hold.start, False)
    run_both(a, b, 4)
    v2 = assert_same(a, b, "after the release")
    assert (v2["imu"][hold] != imu_before[hold]).any(axis=1).mean() > 0.25  # (scenario sanity again: they are stepped now)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("n", [900, N_SPLIT])
def test_runs_back_to_back_and_a_run_followed_by_a_step(M, arith, n):
    """step_n(K1), step_n(K2), step(): the IMU is that of the last step each time"""
    a, b = twin_swarms(M, n, arith_of(M, arith), 7)
    seen = []
    for k in (5, 3, 4, 1):
        run_both(a, b, k)
        seen.append(assert_same(a, b, f"after a run of {k}, n={n}, {arith}")["imu"])
    a.step(DT)
    b.step(DT)
    seen.append(assert_same(a, b, "run followed by step()")["imu"])
    a.step_n(DT, 2)  # two launches: the first one skips its IMU stores, on one stream
    b.step(DT)
    b.step(DT)
    seen.append(assert_same(a, b, "step() followed by a run of two")["imu"])
    for p, q in zip(seen, seen[1:]):
        assert (p != q).any(axis=1).mean() > 0.9, "the IMU must move from one comparison to the next"


@pytest.mark.parametrize("arith,rtol", [("literal", RTOL_LITERAL), ("fast", RTOL_NORTH_STAR)])
@pytest.mark.parametrize("n", [4096, N_SPLIT])
def test_imu_after_a_run_against_the_oracle(M, oracle, arith, rtol, n):
    """Pair.compare holds the IMU (and the state) against the CPU oracle: RTOL_LITERAL for the LITERAL kernels, the north-star
    tolerance for multi-step FAST runs, as tests/test_parity_gpu.py does"""
    rng = np.random.default_rng(8)
    p = Pair(M, n, arith=arith_of(M, arith))
    p.construct(0, n, "x500")
    p.set_state(0, n, random_state(rng, n, 4))
    p.both("set_input", 0, n, oracle.ACTUATOR_CMD, rng.uniform(0.35, 0.60, (n, 4)))
    p.step(DT, 8)
    worst = p.compare(rtol, f"IMU after a run of 8, n={n}, {arith}")
    print(f"n={n} {arith}: worst relative L-inf vs oracle = {worst:.3e}")
    p.step(DT, 2)
    p.compare(rtol, "after a run of 2")


@pytest.mark.parametrize("n", [1200, N_SPLIT])
def test_snapshot_after_a_run_restores_the_same_imu(M, n):
    from mrs_multirotor_simulator_amd import tensors as T
    a, b = twin_swarms(M, n, M.ARITH_FAST, 9)
    run_both(a, b, 6)
    imu = a.get_imu()
    ra, rb = T.save(a), T.save(b)
    assert np.array_equal(ra.cpu().numpy(), rb.cpu().numpy()), "records after a run != records after single steps"
    run_both(a, b, 4)
    assert not np.array_equal(a.get_imu(), imu)
    T.load(a, ra)
    T.load(b, rb)
    assert_same(a, b, f"restored, n={n}")
    assert np.array_equal(a.get_imu(), imu) and np.array_equal(b.get_imu(), imu)
    run_both(a, b, 5)
    assert_same(a, b, f"a run after the restore, n={n}")
