"""Feedback rollouts on the GPU (include/mrs_swarm.h, "feedback rollouts"; tensors.rollout_feedback): the command written at the start of
a command block is cmd_row + G (ref_row - obs_row), formed inside the step kernels from the state before the step.  On the variant-test
swarm of test_rollout_gpu.py (three airframes, mixed-airframe blocks, a ragged tail, held, crashed and NaN-rollback UAVs inside the range,
LAUNCH_CAP sub-steps per launch):

* nothing but the cost elements of the range is written, and commands, gains, setpoints, targets and weights are read only
  (sentinel-filled slack, padded strides) — checked before any test hands the library an exactly sized buffer;
* cost and final state equal the reference in both flavours, both scenarios (every mode with a payload), FP64 and FP32, three feedback
  group sets, shared and per-UAV gains and setpoints, one block for the call and one per command block, four (hold, cost_every, steps);
* zero gains give the bits of tensors.rollout_cost; a horizon split into two calls with accumulate=True equals the single call;
  cost_groups = 0 steps the same state; the sign of the residual is ref - obs (a damping gain damps);
* refused calls change neither state nor `out`; the pointer-addressed kernels (child process), the caller-stream fence, the C++ facade
  (tests/cpp/rollout_feedback_test.cpp) and an ARS-shaped iteration agree.

The reference is always a twin swarm of the same flavour, advanced one command block at a time: tensors.gather(fb_groups, float64) ->
`restate_feedback` in numpy on the host (element-wise FP64 operations, one rounding each) -> tensors.rollout with that one command block;
test_rollout_cost_gpu.restate is applied to its FP64 rows for the cost.  Every comparison is bit for bit; a NaN cost is compared as a
class (test_rollout_cost_gpu).  In LITERAL the state is also compared with the plain set_input / step_n loop.

FEEDBACK_KERNELS maps every entry point of the feedback family of rollout_cost_device.inc to the tests that force it (test_rollout_feedback.py keeps it
complete)."""
import ctypes as C
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import test_rollout_gpu as R
from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_rollout_cost_gpu import assert_cost, restate
from test_rollout_gpu import COUNT, FIRST, LAUNCH_CAP, _hip_malloc, assert_same_state, commands, variant_swarm
from test_rollout_rate_gpu import raw_equal

pytestmark = pytest.mark.gpu
DT = R.DT
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 300
SENTINEL = -1234.5  # (exact in FP32 and FP64)

# (hold, cost_every, steps).  132 = 2 * LAUNCH_CAP + 4.  (3, 1, 132): feedback and evaluations across both launch boundaries;
# (10, 5, 70): blocks straddling launches; hold 70 > LAUNCH_CAP: a launch in which no block starts
RATES = ((1, 1, 5), (3, 1, 132), (10, 5, 70), (70, 140, 140))
assert all(s % h == 0 and s % e == 0 for h, e, s in RATES) and 70 > LAUNCH_CAP and 132 == 2 * LAUNCH_CAP + 4
NAN_OK = np.array([2400 - FIRST])  # the UAV of the range whose velocity the fixture makes non-finite (test_step_variants_gpu.single_scenario)
assert 0 <= NAN_OK[0] < COUNT

# which tests force each entry point of the feedback family of rollout_cost_device.inc (both flavours)
FEEDBACK_KERNELS = {
    "mrs_uav_rollout_feedback": ("test_pointer_form",),
    "mrs_uav_rollout_feedback_buf": ("test_cost_and_state_equal_the_reference[cascade-LITERAL]", "test_cost_and_state_equal_the_reference[cascade-FAST]"),
    "mrs_uav_model_rollout_feedback": ("test_pointer_form",),
    "mrs_uav_model_rollout_feedback_buf": ("test_cost_and_state_equal_the_reference[model-LITERAL]",
                                           "test_cost_and_state_equal_the_reference[model-FAST]", "test_ars_iteration"),
    "mrs_uav_rollout_feedback_mixed": ("test_cost_and_state_equal_the_reference[cascade-LITERAL]", "test_cost_and_state_equal_the_reference[cascade-FAST]"),
}

_sentinel = []  # the outcome of sentinel_check(), once: None (passed) or the failure


def restate_feedback(obs, cmd, gains, refs, b=0):
    """the restatement of mrs_swarm_rollout_feedback_device for command block b: obs [count, W_o] FP64 rows of fb_groups before the step,
    cmd [B, count, >= W_c], gains [Bg, W_c, W_o] (shared) or [Bg, W_c, W_o, count] (per UAV, UAV-minor), refs [Bg, count | 1, >= W_o],
    Bg in {1, B} (numpy arrays; FP32 inputs are widened exactly).  Returns u [count, W_c]: element-wise FP64 operations in the stated
    order, one rounding each.  Host arithmetic hands a NaN operand on with its sign and payload; the kernels pin the same for the
    residual (obs_row.h), so the NaN-rollback UAV's command, and the PID state that remembers it, compare bit for bit too"""
    obs = np.asarray(obs, dtype=np.float64)
    cmd, G, ref = (np.asarray(a, dtype=np.float64) for a in (cmd, gains, refs))  # (widening FP32 is exact)
    count, wo = obs.shape
    wc = G.shape[1]
    assert G.shape[2] == wo and G.ndim in (3, 4) and (G.ndim == 3 or G.shape[3] == count) and ref.shape[1] in (1, count)
    assert G.shape[0] in (1, cmd.shape[0]) and ref.shape[0] in (1, cmd.shape[0])
    Gb, rb = G[b if G.shape[0] > 1 else 0], ref[b if ref.shape[0] > 1 else 0]
    u = np.empty((count, wc))
    with np.errstate(all="ignore"):
        e = [rb[:, j] - obs[:, j] for j in range(wo)]
        for c in range(wc):
            acc = cmd[b, :, c].copy()
            for j in range(wo):
                acc = acc + (Gb[c, j] * e[j])
            u[:, c] = acc
    return u


def draw(rng, mode, fb_groups, B, dtype, dev, per_uav, gain_blocks, shared_refs, ref_blocks, scale=1e-3):
    """gains small enough that the closed loop stays finite over a test's horizon (the rpm columns are thousands: smaller still), in the
    layout of the call, and setpoints near the flight envelope"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    wo, wc = T.gather_width(fb_groups), T.command_width(mode, 8 if mode == O.ACTUATOR_CMD else 10)
    col = np.full(wo, scale)
    if fb_groups & T.OBS_RPM:
        col[-T.MAX_MOTORS:] = scale * 1e-4
    Bg = B if gain_blocks else 1
    gen = torch.Generator(device=dev)  # (per-UAV gains of every block are millions of numbers: drawn where they are used)
    gen.manual_seed(int(rng.integers(1 << 31)))
    g = torch.randn((Bg, wc, wo, COUNT) if per_uav else (Bg, wc, wo), generator=gen, dtype=torch.float64, device=dev)
    g = g * torch.tensor(col[:, None] if per_uav else col, device=dev)
    r = rng.normal(0.0, 2.0, (B if ref_blocks else 1, 1 if shared_refs else COUNT, wo))
    return g.to(dtype), torch.tensor(r, dtype=dtype, device=dev)


def reference(twin, mode, cmd, fb_groups, gains, refs, hold, every, cost_groups, loop=None):
    """the loop the call stands for, on the twin: per command block gather -> restate_feedback -> tensors.rollout with that one block.
    Returns the FP64 rows of cost_groups at the evaluations [E, COUNT, w] (None without cost groups).  loop: a third swarm that takes the
    same blocks through set_input / step_n"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    dev = cmd.device
    cn, gn, rn = (t.double().cpu().numpy() for t in (cmd, gains, refs))  # (widened once, not per block)
    g = math.gcd(hold, every)
    rows = []
    for b in range(cmd.shape[0]):
        o = T.gather(twin, fb_groups, FIRST, COUNT, dtype=torch.float64).cpu().numpy()
        u = torch.tensor(restate_feedback(o, cn, gn, rn, b)[None], device=dev)
        r = T.rollout(twin, mode, u, DT, cost_groups, first=FIRST, hold=hold, obs_every=g)
        if cost_groups:
            rows.append(r.cpu().numpy())
        if loop is not None:
            ol = T.gather(loop, fb_groups, FIRST, COUNT, dtype=torch.float64).cpu().numpy()
            T.set_input(loop, mode, torch.tensor(restate_feedback(ol, cn, gn, rn, b), device=dev), FIRST)
            loop.step_n(DT, hold)
    if not cost_groups:
        return None
    rows = np.concatenate(rows)
    return rows[every // g - 1::every // g]


def assert_twin_finite(twin, what):
    """at most the NaN-rollback UAV of the range may hold a non-finite value: the gains kept every other closed loop finite"""
    st = twin.get_states(FIRST, COUNT)
    bad = np.zeros(COUNT, dtype=bool)
    for f in ("x", "v", "R", "omega"):
        bad |= ~np.isfinite(np.asarray(st[f]).reshape(COUNT, -1)).all(axis=1)
    assert not np.setdiff1d(np.flatnonzero(bad), NAN_OK).size, f"{what}: the twin left the finite range for UAVs {np.flatnonzero(bad)[:8]}"


def make_cost(rng, E, w, dtype, dev):
    import torch
    tg = torch.tensor(rng.normal(0.0, 2.0, (E, COUNT, w)), dtype=dtype, device=dev)
    wt = rng.uniform(0.1, 2.0, (E, w))
    wt[-1] *= 10.0
    return tg, torch.tensor(wt, dtype=dtype, device=dev)


def padded(t, fill_rows, fill_cols):
    """`t` as a view with a padded last dimension (and slack behind the first) into a sentinel-filled tensor, and that tensor"""
    import torch
    big = torch.full((t.shape[0] + fill_rows,) + tuple(t.shape[1:-1]) + (t.shape[-1] + fill_cols,), SENTINEL, dtype=t.dtype, device=t.device)
    view = big[:t.shape[0], ..., :t.shape[-1]]
    view.copy_(t)
    return view, big


def sentinel_check(mrs):
    """every input is a view with padded strides into a sentinel-filled tensor (the gains, which must be dense, with slack in front and
    behind), `out` a view into a larger sentinel vector: every sentinel is intact afterwards, the inputs are unchanged bit for bit, cost
    and state are the reference's"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(311)
    w = T.gather_width(T.OBS_ALL)
    for scen, mode, dtype, pad, per_uav in (("cascade", O.VELOCITY_HDG_CMD, torch.float32, 3, True), ("cascade", O.ATTITUDE_CMD, torch.float64, 2, False),
                                            ("model", O.ACTUATOR_CMD, torch.float32, 0, True)):  # (ACTUATOR rows are dense: no column padding)
        for hold, every, steps in ((3, 1, 132), (10, 5, 70)):
            a, b = variant_swarm(mrs, scen, mrs.ARITH_LITERAL), variant_swarm(mrs, scen, mrs.ARITH_LITERAL)
            dev = torch_dev(a)
            B, E = steps // hold, steps // every
            c = torch.tensor(commands(mode, rng, B, COUNT, a.get_states(FIRST, COUNT)["x"]), dtype=dtype, device=dev)
            gains, refs = draw(rng, mode, T.OBS_ALL, B, dtype, dev, per_uav, True, False, True)
            tg, wt = make_cost(rng, E, w, dtype, dev)
            cmd_v, cmd_big = padded(c, 1, pad)
            ref_v, ref_big = padded(refs, 2, 5)
            tg_v, tg_big = padded(tg, 2, 5)
            wt_v, wt_big = padded(wt, 2, 7)
            gain_big = torch.full((gains.numel() + 200,), SENTINEL, dtype=dtype, device=dev)
            gain_v = gain_big[100:100 + gains.numel()].view(gains.shape)
            gain_v.copy_(gains)
            bigs = (cmd_big, ref_big, tg_big, wt_big, gain_big)
            keep = [t.clone() for t in bigs]
            out_big = torch.full((COUNT + 200,), SENTINEL, dtype=torch.float64, device=dev)
            rows = reference(a, mode, c, T.OBS_ALL, gains, refs, hold, every, T.OBS_ALL)
            want = restate(rows, tg.cpu().numpy(), wt.cpu().numpy())
            got = T.rollout_feedback(b, mode, cmd_v, DT, T.OBS_ALL, gain_v, ref_v, T.OBS_ALL, tg_v, wt_v, first=FIRST, hold=hold, cost_every=every,
                                     out=out_big[100:100 + COUNT])
            torch.cuda.synchronize(dev)
            what = f"{scen} mode {mode} {dtype} hold {hold} cost_every {every} steps {steps}"
            assert got.data_ptr() == out_big[100:].data_ptr() and got.shape == (COUNT,)
            assert bool((out_big[:100] == SENTINEL).all()) and bool((out_big[100 + COUNT:] == SENTINEL).all()), f"{what}: written outside the cost vector"
            for t, k, name in zip(bigs, keep, ("commands", "refs", "targets", "weights", "gains")):
                assert raw_equal(t, k), f"{what}: the {name} tensor was written"
            assert_twin_finite(a, what)
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


@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
@pytest.mark.parametrize("scen", ["cascade", "model"])
def test_cost_and_state_equal_the_reference(mrs, scen, arith):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    require_sentinel(mrs)
    ar = getattr(mrs, "ARITH_" + arith)
    a, b = variant_swarm(mrs, scen, ar), variant_swarm(mrs, scen, ar)
    loop = variant_swarm(mrs, scen, ar) if arith == "LITERAL" else None
    assert np.asarray(a.has_crashed())[FIRST:FIRST + COUNT].any(), "the scenario has crashed UAVs inside the range"
    dev = torch_dev(a)
    rng = np.random.default_rng(313)
    cost_groups = T.OBS_ALL
    w = T.gather_width(cost_groups)
    groups = (T.OBS_ALL, T.OBS_OMEGA, T.OBS_POS | T.OBS_VEL | T.OBS_ROT | T.OBS_OMEGA)
    # every mode with a payload; the model scenario: ACTUATOR, three times so that the forms below rotate there too
    modes = range(1, 11) if scen == "cascade" else (O.ACTUATOR_CMD,) * 3
    assert all(T.command_width(m, 8) > 0 for m in modes) and T.command_width(O.INPUT_UNKNOWN, 8) == 0
    seen = set()
    for di, dtype in enumerate((torch.float64, torch.float32)):
        for mi, mode in enumerate(modes):
            for ri, (hold, every, steps) in enumerate(RATES):
                # the 16 forms (per-UAV gains, a gain block per command block, shared setpoints, a setpoint block per command block) and
                # the three group sets rotate over modes, rates and dtypes
                form = (mi * 5 + ri * 3 + di * 7) % 16
                per_uav, gblocks, shared_r, rblocks = bool(form & 1), bool(form & 2), bool(form & 4), bool(form & 8)
                fb = groups[(mi + ri + di) % 3]
                seen.add((form, (mi + ri + di) % 3, ri, di))
                B, E = steps // hold, steps // every
                cmd = torch.tensor(commands(mode, rng, B, COUNT, a.get_states(FIRST, COUNT)["x"]), dtype=dtype, device=dev)
                gains, refs = draw(rng, mode, fb, B, dtype, dev, per_uav, gblocks, shared_r, rblocks)
                tg, wt = make_cost(rng, E, w, dtype, dev)
                rows = reference(a, mode, cmd, fb, gains, refs, hold, every, cost_groups, loop)
                want = restate(rows, tg.cpu().numpy(), wt.cpu().numpy())
                got = T.rollout_feedback(b, mode, cmd, DT, fb, gains, refs, cost_groups, tg, wt, first=FIRST, hold=hold, cost_every=every)
                what = (f"{arith} {scen} {dtype} mode {mode} hold {hold} cost_every {every} steps {steps} fb_groups {fb:#x} per-UAV gains {per_uav} "
                        f"gain blocks {gains.shape[0]} shared refs {shared_r} ref blocks {refs.shape[0]}")
                assert got.shape == (COUNT,) and got.dtype == torch.float64, what
                assert_twin_finite(a, what)
                assert_cost(got, want, what)
                assert_same_state(a, b, what)
                if loop is not None:
                    assert_same_state(loop, b, what + ": the set_input / step_n loop")
    assert {g for _, g, _, _ in seen} == {0, 1, 2} and {f & 3 for f, _, _, _ in seen} == {0, 1, 2, 3} and {f >> 2 for f, _, _, _ in seen} == {0, 1, 2, 3}
    assert scen != "cascade" or {f for f, _, _, _ in seen} == set(range(16)), "every form and group set was met"
    assert {(r, d) for _, _, r, d in seen} == {(r, d) for r in range(len(RATES)) for d in range(2)}
    assert b.get_diag() == a.get_diag() and b.get_diag()["nan_rollback"] > 0


@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
def test_zero_gains_are_the_cost_rollout(mrs, arith):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    require_sentinel(mrs)
    ar = getattr(mrs, "ARITH_" + arith)
    rng = np.random.default_rng(317)
    w = T.gather_width(T.OBS_ALL)
    for scen, mode, dtype, per_uav, (hold, every, steps) in (("cascade", O.VELOCITY_HDG_CMD, torch.float64, False, (3, 1, 132)),
                                                             ("cascade", O.ATTITUDE_RATE_CMD, torch.float32, True, (10, 5, 70)),
                                                             ("model", O.ACTUATOR_CMD, torch.float64, True, (70, 140, 140))):
        a, b = variant_swarm(mrs, scen, ar), variant_swarm(mrs, scen, ar)
        dev = torch_dev(a)
        B, E = steps // hold, steps // every
        cmd = torch.tensor(commands(mode, rng, B, COUNT, a.get_states(FIRST, COUNT)["x"]), dtype=dtype, device=dev)
        gains, refs = draw(rng, mode, T.OBS_POS | T.OBS_OMEGA | T.OBS_RPM, B, dtype, dev, per_uav, True, False, True)
        tg, wt = make_cost(rng, E, w, dtype, dev)
        want = T.rollout_cost(a, mode, cmd, DT, T.OBS_ALL, tg, wt, first=FIRST, hold=hold, cost_every=every).cpu().numpy()
        got = T.rollout_feedback(b, mode, cmd, DT, T.OBS_POS | T.OBS_OMEGA | T.OBS_RPM, torch.zeros_like(gains), refs, T.OBS_ALL, tg, wt, first=FIRST,
                                 hold=hold, cost_every=every)
        what = f"{arith} {scen} mode {mode} {dtype} hold {hold}"
        # (cmd + 0 * e == cmd for every finite e, and the NaN-rollback UAV's command is not finite: it is rolled back either way)
        assert_cost(got, want, what)
        assert_same_state(a, b, what)


@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
def test_split_horizon_and_no_cost(mrs, arith):
    """two calls over the halves of a horizon, the second with accumulate=True, give the bits of one call (the feedback has no memory);
    accumulate=False overwrites; cost_groups = 0 without a cost vector steps the same state"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    require_sentinel(mrs)
    ar = getattr(mrs, "ARITH_" + arith)
    rng = np.random.default_rng(331)
    w = T.gather_width(T.OBS_ALL)
    fb = T.OBS_POS | T.OBS_VEL | T.OBS_ROT | T.OBS_OMEGA
    for mode, dtype, per_uav, (hold, every, steps) in ((O.VELOCITY_HDG_CMD, torch.float64, True, (3, 6, 132)),
                                                       (O.ATTITUDE_RATE_CMD, torch.float32, False, (10, 5, 140)),
                                                       (O.POSITION_CMD, torch.float64, True, (1, 1, 10))):
        one, two, bare = (variant_swarm(mrs, "cascade", ar) for _ in range(3))
        dev = torch_dev(one)
        B, E = steps // hold, steps // every
        assert B % 2 == 0 and E % 2 == 0
        cmd = torch.tensor(commands(mode, rng, B, COUNT, one.get_states(FIRST, COUNT)["x"]), dtype=dtype, device=dev)
        gains, refs = draw(rng, mode, fb, B, dtype, dev, per_uav, True, False, True)
        tg, wt = make_cost(rng, E, w, dtype, dev)
        out1 = torch.full((COUNT,), SENTINEL, dtype=torch.float64, device=dev)
        whole = T.rollout_feedback(one, mode, cmd, DT, fb, gains, refs, T.OBS_ALL, tg, wt, first=FIRST, hold=hold, cost_every=every, out=out1)
        assert whole.data_ptr() == out1.data_ptr() and not bool((out1 == SENTINEL).any()), "accumulate=False overwrites"
        out2 = torch.full((COUNT,), SENTINEL, dtype=torch.float64, device=dev)
        h, e = B // 2, E // 2
        T.rollout_feedback(two, mode, cmd[:h], DT, fb, gains[:h], refs[:h], T.OBS_ALL, tg[:e], wt[:e], first=FIRST, hold=hold, cost_every=every, out=out2)
        T.rollout_feedback(two, mode, cmd[h:], DT, fb, gains[h:], refs[h:], T.OBS_ALL, tg[e:], wt[e:], first=FIRST, hold=hold, cost_every=every, out=out2,
                           accumulate=True)
        what = f"{arith} mode {mode} {dtype} hold {hold} cost_every {every}"
        assert_cost(out2, out1.cpu().numpy(), what + ": two halves")
        assert_same_state(one, two, what)
        assert T.rollout_feedback(bare, mode, cmd, DT, fb, gains, refs, first=FIRST, hold=hold) is None
        assert_same_state(one, bare, what + ": no cost")


def test_the_residual_is_ref_minus_obs(mrs):
    """one airframe, 64 UAVs with perturbed body rates, ATTITUDE_RATE commands of rate 0: a gain k I on OBS_OMEGA with a zero setpoint
    commands the rate -k omega.  With k > 0 every UAV's |omega| after 200 steps is smaller than with zero gain, with k < 0 larger"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, steps = 64, 200
    rng = np.random.default_rng(337)
    omega0 = rng.uniform(0.2, 0.5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    norms = {}
    for k in (0.0, 0.5, -0.5):
        g = mrs.Swarm(n, arith=mrs.ARITH_LITERAL)
        g.construct(0, n, mrs.model_params("x500"), np.stack([np.arange(n) * 5.0, np.zeros(n), np.full(n, 50.0)], axis=1))
        g.set_state(0, n, omega=omega0)
        dev = torch_dev(g)
        cmd = torch.tensor(np.tile([0.0, 0.0, 0.0, 0.5], (steps, n, 1)), device=dev)
        gain = torch.zeros((1, 4, 3), dtype=torch.float64, device=dev)
        gain[0, :3, :] = k * torch.eye(3, dtype=torch.float64, device=dev)
        T.rollout_feedback(g, O.ATTITUDE_RATE_CMD, cmd, DT, T.OBS_OMEGA, gain, torch.zeros((1, 1, 3), dtype=torch.float64, device=dev))
        norms[k] = np.linalg.norm(g.get_states()["omega"], axis=1)
        g.close()
    assert np.isfinite(norms[0.0]).all() and (norms[0.0] > 0).all()
    assert (norms[0.5] < norms[0.0]).all(), "a damping gain on ref - obs damps"
    assert (norms[-0.5] > norms[0.0]).all(), "the flipped gain excites"


def test_refused_calls_change_nothing(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL)
    dev = torch_dev(g)
    before = T.save(g).cpu().numpy()
    # 12 steps of 100 UAVs in POSITION_CMD (W_c = 4): 4 command blocks (held for 3 steps), OBS_OMEGA | OBS_POS feedback (W_o = 6), 3
    # evaluations of 36 columns
    hip, cmd = _hip_malloc(4 * 100 * 10 * 8)
    _, gain = _hip_malloc(4 * 4 * 6 * 100 * 8)
    _, gain_short = _hip_malloc((4 * 4 * 6 * 100 - 1) * 8)
    _, ref = _hip_malloc(4 * 100 * 6 * 8)
    _, ref_short = _hip_malloc((4 * 100 * 6 - 1) * 8)
    _, tgt = _hip_malloc(3 * 100 * 36 * 8)
    _, wt = _hip_malloc(3 * 36 * 8)
    _, cost = _hip_malloc(100 * 8)
    bufs = (cmd, gain, gain_short, ref, ref_short, tgt, wt, cost)
    host = np.zeros(4 * 4 * 6 * 100)
    fb = T.OBS_POS | T.OBS_OMEGA
    ok = dict(first=0, count=100, mode=O.POSITION_CMD, dt=DT, n_steps=12, cmd_every=3, cost_every=4, dev_cmd=cmd, dtype=T.DTYPE_F64, cmd_stride=10,
              fb_groups=fb, dev_gain=gain, gain_per_uav=1, gain_blocks=4, dev_ref=ref, ref_stride=6, ref_blocks=4, cost_groups=T.OBS_ALL,
              dev_target=tgt, target_stride=36, dev_weight=wt, weight_stride=36, dev_cost=cost, accumulate=True, ext_stream=None)
    bad = [({"gain_blocks": 2}, 1), ({"gain_blocks": 3}, 1), ({"gain_blocks": 0}, 1), ({"ref_blocks": 2}, 1), ({"ref_blocks": 12}, 1),  # a wrong Bg
           ({"gain_per_uav": 2}, 1), ({"gain_per_uav": -1}, 1), ({"dtype": 2}, 1),
           ({"fb_groups": 0}, 1), ({"fb_groups": 0x100}, 1),  # W_o = 0, an unknown group bit
           ({"mode": O.INPUT_UNKNOWN}, 1), ({"mode": 11}, 1),  # a mode without a payload
           ({"dev_gain": host.ctypes.data}, 1), ({"dev_ref": host.ctypes.data}, 1), ({"dev_cost": host.ctypes.data}, 1),  # host pointers
           ({"dev_gain": None}, 1), ({"dev_ref": None}, 1), ({"dev_gain": gain_short}, 1), ({"dev_ref": ref_short}, 1),
           ({"ref_stride": 5}, 1), ({"ref_stride": -1}, 1), ({"cost_groups": 0}, 1),  # (cost pointers without cost groups)
           ({"dev_cost": None}, 1), ({"dev_target": None}, 1), ({"target_stride": 35}, 1), ({"cost_every": 5}, 1), ({"cmd_every": 5}, 1),
           ({"first": R.N_SINGLE - 5}, 3), ({"count": -1}, 3), ({"dt": 0.0}, 1), ({"cmd_stride": 3}, 1), ({"dev_cmd": None}, 1)]
    for change, code in bad:
        with pytest.raises(mrs.MrsError, match=f"error {code}:"):
            g.rollout_feedback_device(**dict(ok, **change))
        assert np.array_equal(T.save(g).cpu().numpy(), before), change
    back = np.ones(100)
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(cost), back.nbytes, 2) == 0
    assert not back.any(), "a refused call wrote the cost vector"
    # the tensor layer: non-dense per-UAV gains, a dtype mismatch, a wrong Bg, W_o = 0 and a payload-less mode never reach the library
    tc = torch.zeros((4, 100, 10), dtype=torch.float64, device=dev)
    tg_ = torch.zeros((4, 4, 6, 100), dtype=torch.float64, device=dev)
    tr = torch.zeros((4, 100, 6), dtype=torch.float64, device=dev)
    to = torch.full((100,), SENTINEL, dtype=torch.float64, device=dev)
    tt, tw = torch.zeros((3, 100, 36), dtype=torch.float64, device=dev), torch.ones((3, 36), dtype=torch.float64, device=dev)
    for kw, msg in ((dict(gains=torch.zeros((4, 100, 4, 6), dtype=torch.float64, device=dev).permute(0, 2, 3, 1)), "gains must be dense"),
                    (dict(gains=torch.zeros((4, 4, 6, 200), dtype=torch.float64, device=dev)[..., ::2]), "gains must be dense"),
                    (dict(gains=tg_.float()), "gains has dtype torch.float32"), (dict(refs=tr.float()), "refs has dtype torch.float32"),
                    (dict(gains=tg_[:2]), "gains: expected"), (dict(refs=tr[:3]), "refs: expected"), (dict(fb_groups=0), "at least one observation group"),
                    (dict(mode=O.INPUT_UNKNOWN), "a mode with a payload"), (dict(gains=tg_.cpu()), "gains is on cpu")):
        a = dict(dict(mode=O.POSITION_CMD, fb_groups=fb, gains=tg_, refs=tr), **kw)
        with pytest.raises(ValueError, match=msg):
            T.rollout_feedback(g, a["mode"], tc, DT, a["fb_groups"], a["gains"], a["refs"], T.OBS_ALL, tt, tw, hold=3, cost_every=4, out=to)
        assert np.array_equal(T.save(g).cpu().numpy(), before), kw
    assert bool((to == SENTINEL).all())
    # the exactly sized buffers are accepted, also as shared gains and rows — once the sentinel check has shown that nothing else is written
    require_sentinel(mrs)
    g.rollout_feedback_device(**dict(ok, dev_gain=wt, dev_ref=wt, dev_target=wt, accumulate=False, gain_per_uav=0, gain_blocks=1,
                                     ref_stride=0, ref_blocks=4, target_stride=0, weight_stride=0))  # (zero-filled buffers: zero gains, finite)
    g.rollout_feedback_device(**dict(ok, cost_groups=0, dev_target=None, dev_weight=None, dev_cost=None, accumulate=False))
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
    rng = np.random.default_rng(347)
    fb, groups = T.OBS_POS | T.OBS_VEL | T.OBS_OMEGA, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT
    cmd = torch.tensor(commands(O.ATTITUDE_RATE_CMD, rng, 9, COUNT, None), device=dev)
    src, refs = draw(rng, O.ATTITUDE_RATE_CMD, fb, 9, torch.float64, dev, True, True, False, True)
    tg, wt = make_cost(rng, 9, T.gather_width(groups), torch.float64, dev)
    want = T.rollout_feedback(a, O.ATTITUDE_RATE_CMD, cmd, DT, fb, src, refs, groups, tg, wt, first=FIRST, hold=4).cpu().numpy()
    for g, side in ((b, torch.cuda.Stream(dev)), (c, torch.cuda.ExternalStream(c.stream(), device=dev))):
        gains = torch.zeros_like(src)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
            gains.copy_(src)  # written on the caller stream right before the call, no synchronisation
            out = T.rollout_feedback(g, O.ATTITUDE_RATE_CMD, cmd, DT, fb, gains, refs, groups, tg, wt, first=FIRST, hold=4)
            copy = out.clone()  # torch work after the call sees the cost
        side.synchronize()
        assert_cost(copy, want, "fenced feedback rollout")
        assert_same_state(a, g, "fenced feedback rollout")


def child_main(out_path):
    """the pointer-addressed kernels (MRS_NO_BUFFER_ADDRESSING=1): cascade, model-only and mixed-block feedback rollouts equal the
    reference in both flavours"""
    import torch
    import mrs_multirotor_simulator_amd as M
    from mrs_multirotor_simulator_amd import tensors as T
    M.load_library()
    rng = np.random.default_rng(349)
    w = T.gather_width(T.OBS_ALL)
    res = []
    for scen, mode in (("cascade", O.VELOCITY_HDG_CMD), ("model", O.ACTUATOR_CMD)):
        for arith in (M.ARITH_LITERAL, M.ARITH_FAST):
            for (hold, every, steps), per_uav in (((3, 1, 132), True), ((70, 140, 140), False)):
                a, b = variant_swarm(M, scen, arith), variant_swarm(M, scen, arith)
                dev = torch_dev(a)
                B, E = steps // hold, steps // every
                cmd = torch.tensor(commands(mode, rng, B, COUNT, a.get_states(FIRST, COUNT)["x"]), dtype=torch.float32, device=dev)
                gains, refs = draw(rng, mode, T.OBS_ALL, B, torch.float32, dev, per_uav, per_uav, not per_uav, True)
                tg, wt = make_cost(rng, E, w, torch.float32, dev)
                want = restate(reference(a, mode, cmd, T.OBS_ALL, gains, refs, hold, every, T.OBS_ALL), tg.cpu().numpy(), wt.cpu().numpy())
                got = T.rollout_feedback(b, mode, cmd, DT, T.OBS_ALL, gains, refs, T.OBS_ALL, tg, wt, first=FIRST, hold=hold, cost_every=every)
                assert_twin_finite(a, f"{scen} arith {arith} hold {hold}")
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
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_rollout_feedback_gpu as T; T.child_main({out!r})"
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
        path = os.path.join(d, "rollout_feedback.bin")
        try:
            out = subprocess.run([build_cpp("rollout_feedback_test"), path], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            R._dead.append(f"rollout_feedback_test timed out after {CHILD_TIMEOUT} s")
            pytest.fail(R._dead[0])
        print(out.stdout)
        if out.returncode < 0:
            R._dead.append(f"rollout_feedback_test ended by signal {-out.returncode}")
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok zero_gains_are_the_cost_rollout", "ok feedback_changes_the_run", "ok no_cost_steps_the_same_state", "ok refused_call_changes_nothing",
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
    # gains [1, 4, 6, n] on OBS_VEL | OBS_OMEGA, UAV-minor, and one shared setpoint row per block
    cc, jj = np.arange(4)[:, None, None], np.arange(6)[None, :, None]
    gains = (0.01 * (cc + 1) - 0.004 * jj + 0.00001 * i[None, None, :])[None]
    refs = (0.1 * np.arange(6)[None, :] - 0.05 * np.arange(B)[:, None])[:, None, :]
    dev = torch_dev(g)
    mine = T.rollout_feedback(g, O.ATTITUDE_RATE_CMD, torch.tensor(cmd, device=dev), DT, T.OBS_VEL | T.OBS_OMEGA, torch.tensor(gains, device=dev),
                              torch.tensor(refs, device=dev), T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, torch.tensor(tg, device=dev),
                              torch.tensor(wt, device=dev), hold=hold, cost_every=every).cpu().numpy()
    assert raw.shape == (n,) and np.array_equal(raw.view(np.uint64), mine.view(np.uint64))


def test_ars_iteration(mrs):
    """one ARS-shaped iteration: one state forked into 64 slots (tensors.load(index=)), a perturbed gain per slot (per-UAV, UAV-minor),
    one call, the argmin of the cost — against the reference loop on a twin fork"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    require_sentinel(mrs)
    m = O.ACTUATOR_CMD
    rng = np.random.default_rng(353)
    fb, groups = T.OBS_POS | T.OBS_VEL | T.OBS_ROT | T.OBS_OMEGA, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT
    wo, w = T.gather_width(fb), T.gather_width(groups)
    src = mrs.Swarm(10, arith=mrs.ARITH_LITERAL)
    src.construct(0, 10, mrs.model_params("x500"), np.stack([np.arange(10) * 5.0, np.zeros(10), np.full(10, 8.0)], axis=1))
    src.set_input(0, 10, O.ATTITUDE_RATE_CMD, np.tile([0.1, -0.2, 0.05, 0.6], (10, 1)))
    src.step_n(DT, 50)
    S, H, hold, j = 64, 8, 10, 3  # 80 steps: two launches
    dev = torch_dev(src)
    rec = T.save(src, j, 1)
    plans = []
    for _ in range(2):
        p = mrs.Swarm(S, arith=mrs.ARITH_LITERAL)
        p.construct(0, S, mrs.model_params("x500"))
        T.load(p, rec, index=torch.zeros(S, dtype=torch.int32, device=dev))
        plans.append(p)
    plan, twin = plans
    x0 = src.get_states(j, 1)
    hover = torch.tensor(np.full((H, S, 4), 0.55), device=dev)
    base = rng.normal(0.0, 1e-3, (1, 4, wo))
    per = base[:, None] + np.concatenate([np.zeros((1, 1, 4, wo)), rng.normal(0.0, 5e-4, (1, S - 1, 4, wo))], axis=1)  # [1, S, W_c, W_o]
    gains = torch.tensor(per, device=dev).permute(0, 2, 3, 1).contiguous()  # UAV-minor
    goal = np.concatenate([x0["x"][0] + [0.0, 0.0, 0.5], np.zeros(3), np.eye(3).ravel(), np.zeros(3)])
    refs = torch.tensor(goal[None, None, :], device=dev)  # one shared setpoint row for the whole call
    tg = torch.tensor(np.tile(np.concatenate([goal[:6], [0.0, 0.0, 0.0, 1.0]]), (H, 1, 1)), device=dev)
    wt = np.tile([1.0, 1.0, 4.0, 0.1, 0.1, 0.1, 0.5, 0.5, 0.5, 0.5], (H, 1))
    wt[-1] *= 20.0
    wt = torch.tensor(wt, device=dev)
    cost = T.rollout_feedback(plan, m, hover, DT, fb, gains, refs, groups, tg, wt, hold=hold)
    assert cost.shape == (S,) and cost.dtype == torch.float64
    best = int(torch.argmin(cost))  # stays on the device until here
    # the reference loop on the twin fork (FIRST / COUNT of this module do not apply: the whole swarm is the range)
    cn, gn, rn = hover.cpu().numpy(), gains.cpu().numpy(), refs.cpu().numpy()
    rows = []
    for b in range(H):
        o = T.gather(twin, fb, 0, S, dtype=torch.float64).cpu().numpy()
        u = torch.tensor(restate_feedback(o, cn, gn, rn, b)[None], device=dev)
        rows.append(T.rollout(twin, m, u, DT, groups, hold=hold).cpu().numpy())
    want = restate(np.concatenate(rows), tg.cpu().numpy(), wt.cpu().numpy())
    c = cost.cpu().numpy()
    assert np.isfinite(want).all() and np.array_equal(c.view(np.uint64), want.view(np.uint64))
    assert best == int(np.argmin(want)) and len(np.unique(c)) > S // 2, "perturbed gains cost differently"
    assert_same_state(plan, twin, "ARS fork")
