"""Cost rollouts on the GPU (include/mrs_swarm.h, "cost rollouts"; tensors.rollout_cost): the weighted squared distance of a UAV's
observation row from a target row, summed over the evaluations of the call inside the step kernels.  On the variant-test swarm of
test_rollout_gpu.py (three airframes, mixed-airframe blocks, a ragged tail, held, crashed and NaN-rollback UAVs, the held and crashed ones
inside the range):

* nothing but the cost elements of the range is written, and commands, targets and weights are read only (sentinel-filled slack, padded
  strides) — checked before any test hands the library an exactly sized buffer;
* cost and final state equal the reference in both flavours, both scenarios (all 11 modes), FP64 and FP32, six (hold, cost_every, steps)
  tuples, per-UAV and shared targets, per-evaluation and shared weights;
* a call split into two halves with accumulate=True equals the single call; accumulate=False overwrites;
* non-finite targets, a zero weight against an infinite target and a negative weight follow the restatement and leave every other UAV's
  cost alone; refused calls change neither state nor `out`;
* the pointer-addressed kernels (child process), the caller-stream fence, the C++ facade (tests/cpp/rollout_cost_test.cpp) and an
  MPPI-shaped fork agree.

The reference is always a twin swarm: tensors.rollout(hold=, obs_every=cost_every) with FP64 commands (FP32 commands widened) writes the
FP64 rows, and `restate` applies the restatement of the ABI comment to them in numpy (element-wise FP64 operations, one rounding each).
Every comparison is bit for bit.  One thing the restatement does not define is compared as a class: a cost that is NaN must be NaN in
both, whatever its sign and payload (IEEE 754 leaves the bits of a generated NaN to the implementation, and the host's and the GPU's
default NaNs differ in the sign bit).

ROLLOUT_COST_KERNELS maps every entry point of rollout_cost_device.inc to the tests that force it (test_rollout_cost.py keeps it complete)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import test_rollout_gpu as R
from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_rollout_gpu import COUNT, FIRST, LAUNCH_CAP, _hip_malloc, assert_same_state, commands, variant_swarm
from test_rollout_rate_gpu import raw_equal
from test_step_variants_gpu import N_SINGLE

pytestmark = pytest.mark.gpu
DT = R.DT
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 300
SENTINEL = -1234.5  # (exact in FP32 and FP64)

# (hold, cost_every, steps).  132 = 2 * LAUNCH_CAP + 4.  (3, 1, 132): an evaluation at every sub-step across both launch boundaries;
# (3, 6, 132), (10, 5, 70): blocks straddling launches; hold 70 > LAUNCH_CAP: a launch that reads no command row; (5, 130, 130): one
# terminal evaluation
RATES = ((1, 1, 5), (3, 1, 132), (3, 6, 132), (10, 5, 70), (70, 140, 140), (5, 130, 130))
assert all(s % h == 0 and s % e == 0 for h, e, s in RATES) and 70 > LAUNCH_CAP and 132 == 2 * LAUNCH_CAP + 4

# which tests force each entry point of rollout_cost_device.inc (both flavours)
ROLLOUT_COST_KERNELS = {
    "mrs_uav_rollout_cost": ("test_pointer_form",),
    "mrs_uav_rollout_cost_buf": ("test_cost_and_state_equal_the_reference[cascade-LITERAL]", "test_cost_and_state_equal_the_reference[cascade-FAST]"),
    "mrs_uav_model_rollout_cost": ("test_pointer_form",),
    "mrs_uav_model_rollout_cost_buf": ("test_cost_and_state_equal_the_reference[model-LITERAL]", "test_cost_and_state_equal_the_reference[model-FAST]",
                                       "test_mppi_iteration"),
    "mrs_uav_rollout_cost_mixed": ("test_cost_and_state_equal_the_reference[cascade-LITERAL]", "test_cost_and_state_equal_the_reference[cascade-FAST]"),
}

_sentinel = []  # the outcome of sentinel_check(), once: None (passed) or the failure


def restate(rows, targets, weights, start=None):
    """the restatement of mrs_swarm_rollout_cost_device on FP64 rows [E, count, w], targets [E, count | 1, >= w], weights [E | 1, >= w]
    (numpy arrays; FP32 inputs are widened exactly): element-wise FP64 operations in the stated order, one rounding each"""
    rows = np.asarray(rows, dtype=np.float64)
    tg, wt = np.asarray(targets).astype(np.float64), np.asarray(weights).astype(np.float64)
    E, count, w = rows.shape
    assert tg.shape[0] == E and tg.shape[1] in (1, count) and wt.shape[0] in (1, E)
    c = np.zeros(count) if start is None else np.array(start, dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(E):
            term = np.zeros(count)
            wj = wt[j if wt.shape[0] > 1 else 0]
            for col in range(w):
                d = rows[j, :, col] - tg[j, :, col]
                term = term + (wj[col] * d) * d
            c = c + term
    return c


def cost_equal(got, want):
    """bit for bit; where the restatement gives NaN, NaN (see the module docstring)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def assert_cost(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    if not cost_equal(got, want):
        bad = np.flatnonzero(~((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))))
        raise AssertionError(f"{what}: cost differs for {len(bad)} UAVs, first {bad[:6]}: got {got[bad[:6]]}, want {want[bad[:6]]}")


def reference_rows(twin, mode, cmd, groups, hold, every):
    """the FP64 rows of the twin: tensors.rollout with the commands widened"""
    from mrs_multirotor_simulator_amd import tensors as T
    return T.rollout(twin, mode, cmd.double(), DT, groups, first=FIRST, hold=hold, obs_every=every).cpu().numpy()


def make_targets(rng, E, w, dtype, dev, shared_targets, shared_weights):
    """targets near the flight envelope, weights positive with a heavier last row (a terminal cost) when they are per evaluation"""
    import torch
    tg = torch.tensor(rng.normal(0.0, 2.0, (E, 1 if shared_targets else COUNT, w)), dtype=dtype, device=dev)
    wt = rng.uniform(0.1, 2.0, (1 if shared_weights else E, w))
    if not shared_weights:
        wt[-1] *= 10.0
    return tg, torch.tensor(wt, dtype=dtype, device=dev)


def sentinel_check(mrs):
    """`out` is a view into a larger sentinel-filled vector; targets, weights and commands are views with padded strides into
    sentinel-filled tensors.  Every sentinel is intact afterwards, the three inputs are unchanged bit for bit, the cost is the reference's."""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(211)
    w = T.gather_width(T.OBS_ALL)
    for scen, mode, dtype, pad in (("cascade", O.VELOCITY_HDG_CMD, torch.float32, 3), ("cascade", O.ATTITUDE_CMD, torch.float64, 2),
                                   ("model", O.ACTUATOR_CMD, torch.float32, 0)):  # (ACTUATOR rows are dense: no column padding)
        for hold, every, steps in ((3, 1, 132), (3, 6, 132), (10, 5, 70), (5, 130, 130)):
            a, b = variant_swarm(mrs, scen, mrs.ARITH_LITERAL), variant_swarm(mrs, scen, mrs.ARITH_LITERAL)
            dev = torch_dev(a)
            B, E = steps // hold, steps // every
            c = torch.tensor(commands(mode, rng, B, COUNT, a.get_states(FIRST, COUNT)["x"]), dtype=dtype, device=dev)
            cmd_big = torch.full((steps + 1, COUNT, c.shape[2] + pad), SENTINEL, dtype=dtype, device=dev)
            cmd_big[:B, :, :c.shape[2]] = c
            tg, wt = make_targets(rng, E, w, dtype, dev, False, False)
            tg_big = torch.full((E + 2, COUNT, w + 5), SENTINEL, dtype=dtype, device=dev)
            tg_big[:E, :, :w] = tg
            wt_big = torch.full((E + 2, w + 7), SENTINEL, dtype=dtype, device=dev)
            wt_big[:E, :w] = wt
            refs = [t.clone() for t in (cmd_big, tg_big, wt_big)]
            out_big = torch.full((COUNT + 200,), SENTINEL, dtype=torch.float64, device=dev)
            want = restate(reference_rows(a, mode, c, T.OBS_ALL, hold, every), tg.cpu().numpy(), wt.cpu().numpy())
            got = T.rollout_cost(b, mode, cmd_big[:B, :, :c.shape[2]] if pad else cmd_big[:B], DT, T.OBS_ALL, tg_big[:E, :, :w], wt_big[:E, :w],
                                 first=FIRST, hold=hold, cost_every=every, out=out_big[100:100 + COUNT])
            torch.cuda.synchronize(dev)
            what = f"{scen} mode {mode} {dtype} hold {hold} cost_every {every} steps {steps}"
            assert got.data_ptr() == out_big[100:].data_ptr() and got.shape == (COUNT,)
            assert bool((out_big[:100] == SENTINEL).all()) and bool((out_big[100 + COUNT:] == SENTINEL).all()), f"{what}: written outside the cost vector"
            for t, ref, name in zip((cmd_big, tg_big, wt_big), refs, ("commands", "targets", "weights")):
                assert raw_equal(t, ref), f"{what}: the {name} tensor was written"
            assert_cost(got, want, what)
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


def test_nothing_outside_the_cost_vector_is_written(mrs):
    require_sentinel(mrs)


def test_held_and_crashed_uavs_are_inside_the_range(mrs):
    g = variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL)
    assert FIRST <= 1950 and 1953 <= FIRST + COUNT, "variant_swarm holds UAVs 1950-1952"
    assert np.asarray(g.has_crashed())[FIRST:FIRST + COUNT].any(), "a crashed UAV inside the range"


@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
@pytest.mark.parametrize("scen", ["cascade", "model"])
def test_cost_and_state_equal_the_reference(mrs, scen, arith):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    require_sentinel(mrs)
    ar = getattr(mrs, "ARITH_" + arith)
    a, b = variant_swarm(mrs, scen, ar), variant_swarm(mrs, scen, ar)
    assert np.asarray(a.has_crashed())[FIRST:FIRST + COUNT].any(), "the scenario has crashed UAVs inside the range"
    dev = torch_dev(a)
    rng = np.random.default_rng(223)
    w = T.gather_width(T.OBS_ALL)
    modes = range(11) if scen == "cascade" else (O.ACTUATOR_CMD, O.INPUT_UNKNOWN, O.ACTUATOR_CMD, O.ACTUATOR_CMD)
    seen = set()
    held = slice(1950 - FIRST, 1953 - FIRST)
    for dtype in (torch.float64, torch.float32):
        for mi, mode in enumerate(modes):
            for ri, (hold, every, steps) in enumerate(RATES):
                # the four target / weight forms rotate over the modes: every rate meets every form in both dtypes
                form = (mi + ri) % 4
                shared_t, shared_w = bool(form & 1), bool(form & 2)
                seen.add((dtype, ri, form))
                x = a.get_states(FIRST, COUNT)["x"]
                cmd = torch.tensor(commands(mode, rng, steps // hold, COUNT, x), dtype=dtype, device=dev)
                tg, wt = make_targets(rng, steps // every, w, dtype, dev, shared_t, shared_w)
                rows = reference_rows(a, mode, cmd, T.OBS_ALL, hold, every)
                want = restate(rows, tg.cpu().numpy(), wt.cpu().numpy())
                got = T.rollout_cost(b, mode, cmd, DT, T.OBS_ALL, tg, wt, first=FIRST, hold=hold, cost_every=every)
                what = f"{arith} {scen} {dtype} mode {mode} hold {hold} cost_every {every} steps {steps} shared targets {shared_t} weights {shared_w}"
                assert got.shape == (COUNT,) and got.dtype == torch.float64, what
                assert_cost(got, want, what)
                assert_same_state(a, b, what)
                assert np.isfinite(want[held]).all() and (want[held] > 0).all(), f"{what}: the held UAVs add a term per evaluation"
    assert len({(d, r) for d, r, f in seen}) * 4 == len(seen), "every rate met the four target / weight forms in both dtypes"
    assert b.get_diag() == a.get_diag() and b.get_diag()["nan_rollback"] > 0


@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
def test_accumulate(mrs, arith):
    """two calls over the halves of a horizon, the second with accumulate=True, give the bits of one call; accumulate=False overwrites"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    require_sentinel(mrs)
    ar = getattr(mrs, "ARITH_" + arith)
    one, two, twin = (variant_swarm(mrs, "cascade", ar) for _ in range(3))
    dev = torch_dev(one)
    rng = np.random.default_rng(227)
    w = T.gather_width(T.OBS_ALL)
    for mode, dtype, (hold, every, steps) in ((O.VELOCITY_HDG_CMD, torch.float64, (3, 6, 132)), (O.ATTITUDE_RATE_CMD, torch.float32, (10, 5, 140)),
                                             (O.POSITION_CMD, torch.float64, (1, 1, 10))):
        B, E = steps // hold, steps // every
        assert B % 2 == 0 and E % 2 == 0
        cmd = torch.tensor(commands(mode, rng, B, COUNT, one.get_states(FIRST, COUNT)["x"]), dtype=dtype, device=dev)
        tg, wt = make_targets(rng, E, w, dtype, dev, False, False)
        out1 = torch.full((COUNT,), SENTINEL, dtype=torch.float64, device=dev)
        whole = T.rollout_cost(one, mode, cmd, DT, T.OBS_ALL, tg, wt, first=FIRST, hold=hold, cost_every=every, out=out1)  # overwrites the sentinels
        assert whole.data_ptr() == out1.data_ptr()
        out2 = torch.full((COUNT,), SENTINEL, dtype=torch.float64, device=dev)
        T.rollout_cost(two, mode, cmd[:B // 2], DT, T.OBS_ALL, tg[:E // 2], wt[:E // 2], first=FIRST, hold=hold, cost_every=every, out=out2)
        T.rollout_cost(two, mode, cmd[B // 2:], DT, T.OBS_ALL, tg[E // 2:], wt[E // 2:], first=FIRST, hold=hold, cost_every=every, out=out2,
                       accumulate=True)
        what = f"{arith} mode {mode} {dtype} hold {hold} cost_every {every}"
        want = restate(reference_rows(twin, mode, cmd, T.OBS_ALL, hold, every), tg.cpu().numpy(), wt.cpu().numpy())
        assert_cost(whole, want, what + ": the single call")
        assert_cost(out2, want, what + ": two halves")
        a1, a2 = out1.cpu().numpy(), out2.cpu().numpy()
        fin = np.isfinite(a1)
        assert np.array_equal(a1[fin].view(np.uint64), a2[fin].view(np.uint64)) and fin.sum() > COUNT // 2, what
        assert_same_state(one, two, what)
        assert_same_state(one, twin, what)


def test_non_finite_and_zero_inputs_follow_the_restatement(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    require_sentinel(mrs)
    rng = np.random.default_rng(229)
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_QUAT | T.OBS_RPM
    w = T.gather_width(groups)
    mode, (hold, every, steps) = O.VELOCITY_HDG_CMD, (3, 6, 72)
    B, E = steps // hold, steps // every
    twin = variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL)
    dev = torch_dev(twin)
    cmd = torch.tensor(commands(mode, rng, B, COUNT, twin.get_states(FIRST, COUNT)["x"]), device=dev)
    rows = reference_rows(twin, mode, cmd, groups, hold, every)
    tg0, wt0 = make_targets(rng, E, w, torch.float64, dev, False, True)
    base = restate(rows, tg0.cpu().numpy(), wt0.cpu().numpy())
    finite = np.flatnonzero(np.isfinite(base))
    u, v = int(finite[7]), int(finite[40])  # two UAVs whose cost is finite in the base case
    for case in ("nan target", "zero weight, infinite target", "negative weight", "base"):
        tg, wt = tg0.clone(), wt0.clone()
        if case == "nan target":
            tg[2, u, 4] = float("nan")
        elif case == "zero weight, infinite target":
            wt[0, 1] = 0.0
            tg[3, u, 1] = float("inf")
            tg[5, v, 1] = float("-inf")
        elif case == "negative weight":
            wt[0, 6] = -3.0
        want = restate(rows, tg.cpu().numpy(), wt.cpu().numpy())
        g = variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL)
        got = T.rollout_cost(g, mode, cmd, DT, groups, tg, wt, first=FIRST, hold=hold, cost_every=every).cpu().numpy()
        assert_cost(got, want, case)
        assert_same_state(twin, g, case)
        others = np.setdiff1d(finite, [u, v])
        if case == "nan target":
            assert np.isnan(got[u]) and np.array_equal(got[others].view(np.uint64), base[others].view(np.uint64)) and got[v] == base[v]
        elif case == "zero weight, infinite target":
            assert np.isnan(got[u]) and np.isnan(got[v]), "0 * inf is NaN: a zero weight does not mask a column"
            assert np.isfinite(got[others]).all(), "every other UAV's cost is unaffected by the two targets"
        elif case == "negative weight":
            assert (got[finite] < base[finite]).any() and np.isfinite(got[finite]).all()


def test_refused_calls_change_nothing(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL)
    dev = torch_dev(g)
    before = T.save(g).cpu().numpy()
    # 12 steps of 100 UAVs: 4 command row blocks of 10 FP64 (held for 3 steps), 3 evaluations (every 4 steps) of 36 columns
    hip, cmd = _hip_malloc(4 * 100 * 10 * 8)
    _, tgt = _hip_malloc(3 * 100 * 36 * 8)
    _, tgt_short = _hip_malloc((3 * 100 - 1) * 36 * 8)
    _, wt = _hip_malloc(3 * 36 * 8)
    _, wt_short = _hip_malloc((3 * 36 - 1) * 8)
    _, cost = _hip_malloc(100 * 8)
    _, cost_short = _hip_malloc(99 * 8)
    bufs = (cmd, tgt, tgt_short, wt, wt_short, cost, cost_short)
    host = np.zeros(100)
    ok = dict(first=0, count=100, mode=O.POSITION_CMD, dt=DT, n_steps=12, cmd_every=3, cost_every=4, dev_cmd=cmd, dtype=T.DTYPE_F64, cmd_stride=10,
              groups=T.OBS_ALL, dev_target=tgt, target_stride=36, dev_weight=wt, weight_stride=36, dev_cost=cost, accumulate=True, ext_stream=None)
    bad = [({"groups": 0}, 1), ({"dev_target": None}, 1), ({"dev_weight": None}, 1), ({"dev_cost": None}, 1), ({"cost_every": 0}, 1),
           ({"cost_every": -1}, 1), ({"cost_every": 5}, 1), ({"cost_every": 24}, 1), ({"cmd_every": 5}, 1), ({"cmd_every": 0}, 1),
           ({"target_stride": 35}, 1), ({"target_stride": -1}, 1), ({"weight_stride": 35}, 1), ({"weight_stride": 1}, 1),
           ({"dev_target": tgt_short}, 1), ({"dev_weight": wt_short}, 1), ({"dev_cost": cost_short}, 1), ({"dev_cost": host.ctypes.data}, 1),
           ({"cost_every": 2}, 1), ({"n_steps": 24}, 1), ({"n_steps": 0}, 1),  # (cost_every 2 / n_steps 24: more rows than the buffers hold)
           ({"first": N_SINGLE - 5}, 3), ({"count": -1}, 3), ({"mode": 11}, 1), ({"dtype": 2}, 1), ({"dt": 0.0}, 1), ({"cmd_stride": 3}, 1),
           ({"groups": 0x100}, 1), ({"dev_cmd": None}, 1)]
    for change, code in bad:
        with pytest.raises(mrs.MrsError, match=f"error {code}:"):
            g.rollout_cost_device(**dict(ok, **change))
        assert np.array_equal(T.save(g).cpu().numpy(), before), change
    back = np.ones(100)
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(cost), back.nbytes, 2) == 0
    assert not back.any(), "a refused call wrote the cost vector"
    # a sharded swarm refuses the call, state and cost untouched
    group = mrs.LoopbackGroup(2)
    shards = []
    for r in range(2):
        s = mrs.Swarm(100)
        s.construct(0, 100, mrs.model_params("x500"), np.stack([np.arange(100) * 3.0 + 400 * r, np.zeros(100), np.full(100, 5.0)], axis=1))
        s.comm_init_loopback(group, r, 200)
        shards.append(s)
    tc = torch.zeros((2, 100, 4), dtype=torch.float64, device=dev)
    tt = torch.zeros((1, 100, 10), dtype=torch.float64, device=dev)
    tw = torch.ones((1, 10), dtype=torch.float64, device=dev)
    to = torch.full((100,), SENTINEL, dtype=torch.float64, device=dev)
    for s in shards:
        x = s.get_states()["x"]
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.rollout_cost(s, O.POSITION_CMD, tc, DT, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, tt, tw, hold=4, cost_every=8, out=to)
        assert R.same(s.get_states()["x"], x)
    assert bool((to == SENTINEL).all())
    for s in shards:
        s.close()
    group.close()
    # the exactly sized buffers are accepted, also as shared rows — once the sentinel check has shown that nothing else is written
    require_sentinel(mrs)
    g.rollout_cost_device(**ok)
    g.rollout_cost_device(**dict(ok, target_stride=0, weight_stride=0, dev_target=wt, accumulate=False))  # [3, 36] shared targets, one weight row
    torch.cuda.synchronize(dev)
    assert not np.array_equal(T.save(g).cpu().numpy(), before)
    for p in bufs:
        hip.hipFree(C.c_void_p(p))


def test_caller_stream_is_fenced(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    require_sentinel(mrs)
    a, b, c = (variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL) for _ in range(3))
    dev = torch_dev(a)
    rng = np.random.default_rng(233)
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_QUAT
    cmd = torch.tensor(commands(O.ATTITUDE_RATE_CMD, rng, 9, COUNT, None), device=dev)
    src, wt = make_targets(rng, 9, T.gather_width(groups), torch.float64, dev, False, False)
    want = T.rollout_cost(a, O.ATTITUDE_RATE_CMD, cmd, DT, groups, src, wt, first=FIRST, hold=4).cpu().numpy()
    for g, side in ((b, torch.cuda.Stream(dev)), (c, torch.cuda.ExternalStream(c.stream(), device=dev))):
        tg = torch.zeros_like(src)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
            tg.copy_(src)  # written on the caller stream right before the call, no synchronisation
            out = T.rollout_cost(g, O.ATTITUDE_RATE_CMD, cmd, DT, groups, tg, wt, first=FIRST, hold=4)
            copy = out.clone()  # torch work after the call sees the cost
        side.synchronize()
        assert_cost(copy, want, "fenced cost rollout")
        assert_same_state(a, g, "fenced cost rollout")


def child_main(out_path):
    """the pointer-addressed kernels (MRS_NO_BUFFER_ADDRESSING=1): cascade, model-only and mixed-block cost rollouts equal the reference
    in both flavours"""
    import torch
    import mrs_multirotor_simulator_amd as M
    from mrs_multirotor_simulator_amd import tensors as T
    M.load_library()
    rng = np.random.default_rng(239)
    w = T.gather_width(T.OBS_ALL)
    res = []
    for scen, mode in (("cascade", O.VELOCITY_HDG_CMD), ("model", O.ACTUATOR_CMD)):
        for arith in (M.ARITH_LITERAL, M.ARITH_FAST):
            for (hold, every, steps), shared in (((3, 1, 132), False), ((70, 140, 140), True)):
                a, b = variant_swarm(M, scen, arith), variant_swarm(M, scen, arith)
                dev = torch_dev(a)
                cmd = torch.tensor(commands(mode, rng, steps // hold, COUNT, a.get_states(FIRST, COUNT)["x"]), dtype=torch.float32, device=dev)
                tg, wt = make_targets(rng, steps // every, w, torch.float32, dev, shared, shared)
                want = restate(reference_rows(a, mode, cmd, T.OBS_ALL, hold, every), tg.cpu().numpy(), wt.cpu().numpy())
                got = T.rollout_cost(b, mode, cmd, DT, T.OBS_ALL, tg, wt, first=FIRST, hold=hold, cost_every=every)
                assert_cost(got, want, f"{scen} arith {arith} hold {hold}")
                assert_same_state(a, b, f"{scen} arith {arith} hold {hold}")
        res.append(scen)
    np.save(out_path, np.array(res))


def test_pointer_form(mrs, tmp_path):
    if R._dead:
        pytest.fail(f"an earlier child process died ({R._dead[0]}): no further GPU process is started")
    require_sentinel(mrs)
    out = str(tmp_path / "pointer.npy")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MRS_")}
    env["MRS_NO_BUFFER_ADDRESSING"] = "1"
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_rollout_cost_gpu as T; T.child_main({out!r})"
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
    require_sentinel(mrs)  # (the C++ test hands the library exactly sized buffers)
    n, B, hold, every, W = 1000, 6, 10, 20, 10
    E = B * hold // every
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rollout_cost.bin")
        try:
            out = subprocess.run([build_cpp("rollout_cost_test"), path], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            R._dead.append(f"rollout_cost_test timed out after {CHILD_TIMEOUT} s")
            pytest.fail(R._dead[0])
        print(out.stdout)
        if out.returncode < 0:
            R._dead.append(f"rollout_cost_test ended by signal {-out.returncode}")
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok cost_equals_the_restatement", "ok final_state_equals_the_rate_rollout", "ok refused_call_changes_nothing", "ok accumulate_adds",
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
    e, c = np.arange(E)[:, None, None], np.arange(W)[None, None, :]
    tg = 0.25 * c - 0.5 * e + 0.002 * i[None, :, None]
    wt = np.where(np.arange(E)[:, None] == E - 1, 10.0, 1.0) + 0.125 * np.arange(W)[None, :]
    dev = torch_dev(g)
    mine = T.rollout_cost(g, O.ATTITUDE_RATE_CMD, torch.tensor(cmd, device=dev), DT, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, torch.tensor(tg, device=dev),
                          torch.tensor(wt, device=dev), hold=hold, cost_every=every).cpu().numpy()
    assert raw.shape == (n,) and np.array_equal(raw.view(np.uint64), mine.view(np.uint64))


def test_mppi_iteration(mrs):
    """save one UAV, indexed-load it into 64 slots, rollout_cost at hold = 10 with per-sample commands: the slot whose commands are the
    source's has the cost the source's own continuation gives, and a softmin over the costs stays on the device"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    require_sentinel(mrs)
    m = O.ACTUATOR_CMD
    rng = np.random.default_rng(241)
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_QUAT
    w = T.gather_width(groups)
    src = mrs.Swarm(10, arith=mrs.ARITH_LITERAL)
    src.construct(0, 10, mrs.model_params("x500"), np.stack([np.arange(10) * 5.0, np.zeros(10), np.full(10, 8.0)], axis=1))
    src.set_input(0, 10, O.ATTITUDE_RATE_CMD, np.tile([0.1, -0.2, 0.05, 0.6], (10, 1)))
    src.step_n(DT, 50)
    S, H, hold, j = 64, 8, 10, 3  # 80 steps: two launches
    plan = mrs.Swarm(S, arith=mrs.ARITH_LITERAL)
    plan.construct(0, S, mrs.model_params("x500"))
    dev = torch_dev(src)
    rec = T.save(src, j, 1)
    T.load(plan, rec, index=torch.zeros(S, dtype=torch.int32, device=dev))
    nominal = commands(m, rng, H, 1, None, n_motors=4, width=4)
    u = np.repeat(nominal, S, axis=1) + np.concatenate([np.zeros((H, 1, 4)), rng.normal(0, 0.05, (H, S - 1, 4))], axis=1)
    goal = np.concatenate([src.get_states(j, 1)["x"][0] + [0.0, 0.0, 0.5], np.zeros(3), [0.0, 0.0, 0.0, 1.0]])
    tg = torch.tensor(np.tile(goal, (H, 1, 1)), device=dev)  # one shared row per evaluation
    wt = np.tile([1.0, 1.0, 4.0, 0.1, 0.1, 0.1, 0.5, 0.5, 0.5, 0.5], (H, 1))
    wt[-1] *= 20.0  # terminal cost
    wt = torch.tensor(wt, device=dev)
    cost = T.rollout_cost(plan, m, torch.tensor(u, device=dev), DT, groups, tg, wt, hold=hold)
    assert cost.shape == (S,) and cost.dtype == torch.float64
    weights = torch.softmax(-(cost - cost.min()) / 0.05, dim=0)  # the softmin of an MPPI update, on the device
    assert weights.shape == (S,) and abs(float(weights.sum()) - 1.0) < 1e-12
    own = []
    for t in range(H):
        src.set_input(j, 1, m, nominal[t])
        src.step_n(DT, hold)
        own.append(T.gather(src, groups, j, 1, dtype=torch.float64)[0])
    rows = torch.stack(own).cpu().numpy().reshape(H, 1, w)
    want = restate(rows, tg.cpu().numpy(), wt.cpu().numpy())
    c = cost.cpu().numpy()
    assert np.isfinite(c).all() and c[:1].view(np.uint64) == want.view(np.uint64), "sample 0 has the cost of the source UAV's own continuation"
    assert len(np.unique(c)) > S // 2, "perturbed samples cost differently"
