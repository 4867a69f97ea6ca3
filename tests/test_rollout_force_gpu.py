"""Device-resident external forces on the GPU (include/mrs_swarm.h, "device-resident external forces"; tensors.apply_force and
tensors.rollout(forces=, force_hold=)): force row block j is applied before step j * force_hold and stays latched for force_hold steps.
On the variant-test swarm of test_rollout_gpu.py (three airframes, mixed-airframe blocks, a ragged tail, held, crashed and NaN-rollback
UAVs):

* nothing but the due rows is read or written (sentinel-filled slack, padded force rows) — checked before any test hands the library an
  exactly sized buffer;
* in LITERAL a force rollout equals the set_input / apply_force / step_n / gather loop of the ABI comment bit for bit (rows, state, PID,
  IMU, external force, crash flags, diag) in all 11 modes, FP64 and FP32, for every tuple of RATES;
* in both flavours a force rollout whose blocks all hold the same rows equals host apply_force followed by the rate (or plain) rollout;
* FAST tracks the FAST loop within the tolerances of test_rollout_gpu.test_fast_tracks_the_loop_and_itself, is bit-identical to itself
  split at force-block boundaries, and its last row block is gather of the final state;
* held UAVs report their unchanged state and are left, like the whole range, carrying the last force block; UAVs outside keep theirs;
* apply_force_device equals host apply_force, also with a collision tick pending;
* refused calls change nothing, and the exactly sized buffers are accepted;
* it follows the CPU oracle under a gust sequence; an MPPI fork under sampled gusts reproduces the source UAV's own continuation; the
  pointer-addressed kernels (child process), the caller-stream fence and the C++ facade (tests/cpp/rollout_force_test.cpp) agree.

Forces are drawn up to a few newtons per axis (the order of the airframes' weight), include exact zeros, and one UAV of one block gets a
non-finite component: whatever the loop does with it, the rollout does.  Every test against the loop also shows that the forced run
differs from an unforced twin.  All comparisons are bit for bit except the two against other arithmetic (the oracle: RTOL_LITERAL; the
FAST loop: RTOL_FAST after one step, RTOL_NORTH_STAR after the run), which sit exactly where test_rollout_rate_gpu uses them."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import helpers
import test_rollout_gpu as R
import test_rollout_rate_gpu as RR
from helpers import RTOL_FAST, RTOL_LITERAL, RTOL_NORTH_STAR
from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_rollout_gpu import COUNT, FIRST, LAUNCH_CAP, _hip_malloc, assert_same_state, commands, same, variant_swarm
from test_rollout_rate_gpu import SENTINEL, raw_equal
from test_step_variants_gpu import N_SINGLE

pytestmark = pytest.mark.gpu
DT = R.DT
REBOUNCE = R.REBOUNCE
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 300
FORCE_MAX = 4.0  # N per axis: the order of the airframes' weight

# (cmd_every, obs_every, force_every, steps).  132 = 2 * LAUNCH_CAP + 4: all three kinds of block straddle both launch boundaries;
# (70, 140, 35, 140): the second launch reads no command row; (2, 2, 70, 140): the second launch reads no force row
RATES = ((1, 1, 1, 5), (4, 4, 2, 8), (3, 6, 4, 132), (10, 5, 7, 70), (70, 140, 35, 140), (5, 130, 130, 130), (130, 5, 1, 130), (2, 2, 70, 140))
assert all(s % c == 0 and s % o == 0 and s % f == 0 for c, o, f, s in RATES) and 70 > LAUNCH_CAP and 132 == 2 * LAUNCH_CAP + 4

# which test forces each kernel of the force family of rollout_rate_device.inc (both flavours; test_rollout_force.py keeps the table complete)
ROLLOUT_FORCE_KERNELS = {
    "mrs_uav_rollout_force": ("test_pointer_form",),
    "mrs_uav_rollout_force_buf": ("test_literal_equals_the_loop[cascade]", "test_equals_apply_force_and_the_rate_rollout[cascade-FAST]"),
    "mrs_uav_model_rollout_force": ("test_pointer_form",),
    "mrs_uav_model_rollout_force_buf": ("test_literal_equals_the_loop[model]", "test_mppi_fork_under_gusts[ACTUATOR_CMD]"),
    "mrs_uav_rollout_force_mixed": ("test_literal_equals_the_loop[cascade]",),
}

_sentinel = []  # the outcome of sentinel_check(), once: None (passed) or the failure


def forces(rng, blocks, count, bad=None):
    """[blocks, count, 3] forces up to FORCE_MAX N per axis; every seventh row and the whole of block 1 (if there is one) are exact zeros;
    bad = (block, uav, value): one non-finite component"""
    f = rng.uniform(-FORCE_MAX, FORCE_MAX, (blocks, count, 3))
    f[:, ::7] = 0.0
    if blocks > 1:
        f[1] = 0.0
    if bad is not None:
        f[bad[0] % blocks, bad[1], 1] = bad[2]
    return f


def force_loop(g, mode, cmd, frc, groups, first, out_dtype, hold, every, fhold):
    """the loop of the ABI comment of mrs_swarm_rollout_force_device, through tensors"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    steps, count = cmd.shape[0] * hold, cmd.shape[1]
    assert frc.shape[0] * fhold == steps
    out = torch.empty((steps // every, count, T.gather_width(groups)), dtype=out_dtype, device=cmd.device) if groups else None
    for t in range(steps):
        if t % hold == 0:
            T.set_input(g, mode, cmd[t // hold], first)
        if t % fhold == 0:
            T.apply_force(g, frc[t // fhold], first)
        g.step_n(DT, 1)
        if groups and (t + 1) % every == 0:
            T.gather(g, groups, first, count, out=out[(t + 1) // every - 1])
    return out


def differing(a, b):
    """fraction of the UAVs (axis 1) whose rows differ anywhere between two row tensors.  The callers ask for more than half: six UAVs of
    seven get a non-zero force in block 0, and a few of the range are held or carry non-finite state in both runs"""
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return float(((a != b) & ~(np.isnan(a) & np.isnan(b))).any(axis=(0, 2)).mean())


def sentinel_check(mrs):
    """commands, forces and rows are views into larger sentinel-filled tensors: padded row strides (force_stride > 3), and behind the last
    due block as many blocks as a kernel that still read (or wrote) a row per step would touch.  Commands and forces are bit-unchanged, no
    sentinel is overwritten, the due rows are the loop's."""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(171)
    for scen, mode, dtype, pad in (("cascade", O.VELOCITY_HDG_CMD, torch.float32, 3), ("cascade", O.ATTITUDE_CMD, torch.float64, 2),
                                   ("model", O.ACTUATOR_CMD, torch.float32, 0)):  # (ACTUATOR rows are dense: no column padding)
        for hold, every, fhold, steps in ((4, 4, 2, 8), (3, 6, 4, 132), (10, 5, 7, 70), (5, 130, 130, 130), (2, 2, 70, 140)):
            a, b = variant_swarm(mrs, scen, mrs.ARITH_LITERAL), variant_swarm(mrs, scen, mrs.ARITH_LITERAL)
            dev = torch_dev(a)
            B, due, Bf, ow = steps // hold, steps // every, steps // fhold, T.gather_width(T.OBS_ALL)
            c = torch.tensor(commands(mode, rng, B, COUNT, a.get_states(FIRST, COUNT)["x"]), dtype=dtype, device=dev)
            f = torch.tensor(forces(rng, Bf, COUNT), dtype=dtype, device=dev)
            cmd_big = torch.full((steps + 1, COUNT, c.shape[2] + pad), SENTINEL, dtype=dtype, device=dev)
            cmd_big[:B, :, :c.shape[2]] = c
            cmd_ref = cmd_big.clone()
            frc_big = torch.full((steps + 1, COUNT, 3 + 2 + pad), SENTINEL, dtype=dtype, device=dev)  # force_stride 5 .. 8
            frc_big[:Bf, :, :3] = f
            frc_ref = frc_big.clone()
            obs_big = torch.full((steps + 1, COUNT, ow + 5), SENTINEL, dtype=dtype, device=dev)
            want = force_loop(a, mode, c, f, T.OBS_ALL, FIRST, dtype, hold, every, fhold)
            got = T.rollout(b, mode, cmd_big[:B], DT, T.OBS_ALL, first=FIRST, out=obs_big[:due], hold=hold, obs_every=every, forces=frc_big[:Bf],
                            force_hold=fhold)
            torch.cuda.synchronize(dev)
            what = f"{scen} mode {mode} {dtype} hold {hold} obs_every {every} force_hold {fhold} steps {steps}"
            assert got.shape == (due, COUNT, ow) and got.data_ptr() == obs_big.data_ptr()
            assert raw_equal(cmd_big, cmd_ref), f"{what}: the command tensor was written"
            assert raw_equal(frc_big, frc_ref), f"{what}: the force tensor was written"
            assert bool((obs_big[due:] == SENTINEL).all()), f"{what}: rows behind the last due row block were written"
            assert bool((obs_big[:due, :, ow:] == SENTINEL).all()), f"{what}: elements past a row's width were written"
            assert raw_equal(got, want), f"{what}: the due rows are not the loop's"
            assert_same_state(a, b, what)
            # (a kernel that read a sentinel as a force would have left it in the force columns)
            assert same(b.get_external_force(FIRST, COUNT), f[-1].double().cpu().numpy()), f"{what}: the force left behind"


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


def test_nothing_outside_the_due_rows_is_touched(mrs):
    require_sentinel(mrs)


@pytest.mark.parametrize("scen", ["cascade", "model"])
def test_literal_equals_the_loop(mrs, scen):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, b, calm = (variant_swarm(mrs, scen, mrs.ARITH_LITERAL) for _ in range(3))
    assert np.asarray(a.has_crashed()).any(), "the scenario has crashed UAVs"
    dev = torch_dev(a)
    rng = np.random.default_rng(173)
    modes = range(11) if scen == "cascade" else (O.ACTUATOR_CMD, O.INPUT_UNKNOWN, O.ACTUATOR_CMD)
    first_case = True
    for dtype in (torch.float64, torch.float32):
        for mode in modes:
            for k, (hold, every, fhold, steps) in enumerate(RATES):
                x = a.get_states(FIRST, COUNT)["x"]
                cmd = torch.tensor(commands(mode, rng, steps // hold, COUNT, x), dtype=dtype, device=dev)
                # one UAV of one block gets a non-finite component, once per mode (UAV 40 of the range is neither held nor at a block edge)
                bad = (2, 40, float("nan") if mode % 2 else float("inf")) if k == 2 else None
                frc = torch.tensor(forces(rng, steps // fhold, COUNT, bad), dtype=dtype, device=dev)
                want = force_loop(a, mode, cmd, frc, T.OBS_ALL, FIRST, dtype, hold, every, fhold)
                got = T.rollout(b, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every, forces=frc, force_hold=fhold)
                what = f"{dtype} mode {mode} hold {hold} obs_every {every} force_hold {fhold} steps {steps}"
                assert got.shape == (steps // every, COUNT, T.gather_width(T.OBS_ALL)), what
                w, gt = want.cpu().numpy(), got.cpu().numpy()
                assert np.array_equal(w.view(np.uint8), gt.view(np.uint8)), f"{what}: observation rows differ at {np.argwhere(w != gt)[:5]}"
                assert_same_state(a, b, what)
                assert same(b.get_external_force(FIRST, COUNT), frc[-1].double().cpu().numpy()), f"{what}: the force left behind"
                if first_case:  # the same call without forces, from the same state: the forces moved the state visibly
                    first_case = False
                    unforced = T.rollout(calm, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every)
                    assert differing(got, unforced) > 0.5, f"{what}: the forced rows are the unforced twin's"
    # the non-finite velocities of the scenario took the NaN-rollback path in both, as often; the other counters agree too
    assert b.get_diag() == a.get_diag() and b.get_diag()["nan_rollback"] > 0


@pytest.mark.parametrize("arith", ["FAST", "LITERAL"])
@pytest.mark.parametrize("scen", ["cascade", "model"])
def test_equals_apply_force_and_the_rate_rollout(mrs, scen, arith):
    """rollout(cmd, hold=C, obs_every=O, forces=[f] * Bf) == host apply_force(f); rollout(cmd, hold=C, obs_every=O) on a twin, rows and
    final state, bit for bit: the force kernels are the existing kernels plus the force rows"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ar = getattr(mrs, "ARITH_" + arith)
    a, b, calm = (variant_swarm(mrs, scen, ar) for _ in range(3))
    dev = torch_dev(a)
    rng = np.random.default_rng(179)
    modes = (O.ATTITUDE_RATE_CMD, O.POSITION_CMD, O.ACTUATOR_CMD) if scen == "cascade" else (O.ACTUATOR_CMD,)
    first_case = True
    for dtype in (torch.float64, torch.float32):
        for mode in modes:
            for hold, every, fhold, steps in RATES:
                x = a.get_states(FIRST, COUNT)["x"]
                cmd = torch.tensor(commands(mode, rng, steps // hold, COUNT, x), dtype=dtype, device=dev)
                f0 = torch.tensor(forces(rng, 1, COUNT), dtype=dtype, device=dev)
                a.apply_force(FIRST, COUNT, f0[0].double().cpu().numpy())
                want = T.rollout(a, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every)
                got = T.rollout(b, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every,
                                forces=f0.repeat(steps // fhold, 1, 1).contiguous(), force_hold=fhold)
                what = f"{arith} {scen} {dtype} mode {mode} hold {hold} obs_every {every} force_hold {fhold} steps {steps}"
                assert raw_equal(got, want), f"{what}: rows differ from apply_force + the rate rollout"
                assert_same_state(a, b, what)
                if first_case:
                    first_case = False
                    unforced = T.rollout(calm, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every)
                    assert differing(got, unforced) > 0.5, f"{what}: the forced rows are the unforced twin's"


def test_fast_tracks_the_loop_and_its_splits(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    loop_g, calm = variant_swarm(mrs, "cascade", mrs.ARITH_FAST), variant_swarm(mrs, "cascade", mrs.ARITH_FAST)
    one, split = variant_swarm(mrs, "cascade", mrs.ARITH_FAST), variant_swarm(mrs, "cascade", mrs.ARITH_FAST)
    dev = torch_dev(one)
    rng = np.random.default_rng(183)
    groups = T.OBS_POS | T.OBS_VEL | T.OBS_ROT
    # against the FAST loop: 6 commands held for 4 steps, a force every 2 steps, a row per step — the first row is the state after ONE
    # step (RTOL_FAST), the last after the run of 24 steps (RTOL_NORTH_STAR), over the UAVs whose rows are finite in the loop
    hold, fhold, B = 4, 2, 6
    cmd = torch.tensor(commands(O.ATTITUDE_RATE_CMD, rng, B, COUNT, None), dtype=torch.float64, device=dev)
    frc = torch.tensor(forces(rng, B * hold // fhold, COUNT), dtype=torch.float64, device=dev)
    want = force_loop(loop_g, O.ATTITUDE_RATE_CMD, cmd, frc, groups, FIRST, torch.float64, hold, 1, fhold).cpu().numpy()
    got_t = T.rollout(one, O.ATTITUDE_RATE_CMD, cmd, DT, groups, first=FIRST, hold=hold, obs_every=1, forces=frc, force_hold=fhold)
    got = got_t.cpu().numpy()
    assert got.shape == want.shape == (24, COUNT, 15)
    ok = np.isfinite(want).all(axis=(0, 2))
    helpers.assert_close(got[0][ok], want[0][ok], RTOL_FAST, "FAST force rollout vs loop after one step")
    helpers.assert_close(got[-1][ok], want[-1][ok], RTOL_NORTH_STAR, "FAST force rollout vs loop after the run")
    unforced = T.rollout(calm, O.ATTITUDE_RATE_CMD, cmd, DT, groups, first=FIRST, hold=hold, obs_every=1)
    assert differing(got_t, unforced) > 0.5, "FAST: the forced rows are the unforced twin's"
    T.rollout(split, O.ATTITUDE_RATE_CMD, cmd, DT, groups, first=FIRST, hold=hold, obs_every=1, forces=frc, force_hold=fhold)
    # one call == the same horizon split into calls at force-block boundaries, bit for bit (force blocks of 10 steps holding two command
    # blocks and two row blocks each; 70 steps: two launches)
    hold, every, fhold, Bf = 5, 5, 10, 7
    cmd = torch.tensor(commands(O.ATTITUDE_RATE_CMD, rng, Bf * fhold // hold, COUNT, None), dtype=torch.float64, device=dev)
    frc = torch.tensor(forces(rng, Bf, COUNT), dtype=torch.float64, device=dev)
    whole = T.rollout(one, O.ATTITUDE_RATE_CMD, cmd, DT, groups, first=FIRST, hold=hold, obs_every=every, forces=frc, force_hold=fhold)
    parts = [T.rollout(split, O.ATTITUDE_RATE_CMD, cmd[2 * j:2 * j + 2], DT, groups, first=FIRST, hold=hold, obs_every=every, forces=frc[j:j + 1],
                       force_hold=fhold) for j in range(Bf)]
    assert whole.shape == (14, COUNT, 15) and all(p.shape == (2, COUNT, 15) for p in parts)
    assert raw_equal(torch.cat(parts), whole), "FAST: one call vs calls split at force-block boundaries"
    assert_same_state(one, split, "FAST: one call vs calls split at force-block boundaries")
    # the last row block is gather_device of the final state
    last = T.rollout(one, O.ATTITUDE_RATE_CMD, cmd[:2], DT, T.OBS_ALL, first=FIRST, hold=3, obs_every=6, forces=frc[:3], force_hold=2)
    assert last.shape[0] == 1 and same(last[0].cpu().numpy(), T.gather(one, T.OBS_ALL, FIRST, COUNT, dtype=torch.float64).cpu().numpy())


def test_held_uavs_and_the_force_left_behind(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, b, calm = (variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL) for _ in range(3))
    dev = torch_dev(a)
    rng = np.random.default_rng(189)
    held = slice(1950 - FIRST, 1953 - FIRST)  # variant_swarm: set_hold(1950, 3) inside the range, set_hold(100, 2) outside
    for g in (a, b):  # the UAVs outside the range carry a force of their own
        g.apply_force(0, FIRST, np.tile([0.5, -0.25, 1.0], (FIRST, 1)))
    outside_f = b.get_external_force(0, FIRST)
    for n_case, (mode, hold, every, fhold, steps) in enumerate(((O.VELOCITY_HDG_CMD, 3, 6, 4, 132), (O.ATTITUDE_RATE_CMD, 70, 35, 140, 140),
                                                                (O.POSITION_CMD, 10, 5, 7, 70), (O.ATTITUDE_RATE_CMD, 2, 2, 70, 140))):
        dtype = torch.float32 if n_case == 2 else torch.float64
        before = T.gather(b, T.OBS_ALL, 1950, 3, dtype=dtype).double().cpu().numpy()
        outside = T.gather(b, T.OBS_ALL, 100, 2, dtype=torch.float64).cpu().numpy()
        cmd = torch.tensor(commands(mode, rng, steps // hold, COUNT, a.get_states(FIRST, COUNT)["x"]), dtype=dtype, device=dev)
        frc = torch.tensor(forces(rng, steps // fhold, COUNT), dtype=dtype, device=dev)
        frc[-1, held] = torch.tensor([[1.5, -2.5, 0.75]] * 3, dtype=dtype, device=dev)  # (not one of the zero rows)
        want = force_loop(a, mode, cmd, frc, T.OBS_ALL, FIRST, dtype, hold, every, fhold)
        got = T.rollout(b, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every, forces=frc, force_hold=fhold)
        assert got.shape[0] == steps // every and raw_equal(got, want)
        g64 = got.double().cpu().numpy()
        for j in range(steps // every):
            assert same(g64[j, held], before), f"mode {mode}: row block {j} of the held UAVs is not their unchanged state"
        assert same(T.gather(b, T.OBS_ALL, 100, 2, dtype=torch.float64).cpu().numpy(), outside), "a held UAV outside the range moved"
        assert not same(g64[0], g64[-1])  # the moving UAVs did move between two row blocks
        # the whole range, held UAVs included, carries the last force block, widened; the UAVs outside keep theirs
        assert same(b.get_external_force(FIRST, COUNT), frc[-1].double().cpu().numpy()), f"mode {mode}: the force left behind"
        assert same(b.get_external_force(0, FIRST), outside_f), "a force outside the range changed"
        assert_same_state(a, b, f"mode {mode}")
        if n_case == 0:
            unforced = T.rollout(calm, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every)
            assert differing(got, unforced) > 0.5, "the forced rows are the unforced twin's"
    # released, the held UAVs fly on the LAST command and force row blocks in both
    before = T.gather(b, T.OBS_ALL, 1950, 3, dtype=torch.float64).cpu().numpy()
    for g in (a, b):
        g.set_hold(1950, 3, False)
        g.set_hold(100, 2, False)
        g.step_n(DT, 3)
    assert_same_state(a, b, "after the hold was released")
    assert not same(T.gather(b, T.OBS_ALL, 1950, 3, dtype=torch.float64).cpu().numpy(), before), "the released UAVs moved"


def test_apply_force_device_equals_apply_force(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(191)
    for scen in ("cascade", "model"):
        a, b, calm = (variant_swarm(mrs, scen, mrs.ARITH_LITERAL) for _ in range(3))
        dev = torch_dev(a)
        for dtype, first, count, pad in ((torch.float64, FIRST, COUNT, 0), (torch.float32, 0, N_SINGLE, 2), (torch.float64, 37, 1000, 5),
                                         (torch.float32, 1950, 3, 0)):
            f = torch.tensor(forces(rng, 1, count, (0, count // 2, float("nan")))[0], dtype=dtype, device=dev)
            big = torch.full((count, 3 + pad), SENTINEL, dtype=dtype, device=dev)
            big[:, :3] = f
            ref = big.clone()
            a.apply_force(first, count, f.double().cpu().numpy())
            T.apply_force(b, big[:, :3] if pad else big, first)
            assert raw_equal(big, ref), "the force rows were written"
            assert same(b.get_external_force(), a.get_external_force())
            for g in (a, b):
                g.step_n(DT, 3)
            assert_same_state(a, b, f"{scen} {dtype} [{first}, {first + count}): steps after apply_force")
        calm.step_n(DT, 12)
        assert not same(calm.get_states()["x"], b.get_states()["x"]), "the forces moved nothing"
        # collision ticks evaluate pending forces and set every UAV's force: both twins go through them identically
        for g in (a, b):
            g.tick_n(DT, 5, True, False, REBOUNCE)
        assert_same_state(a, b, f"{scen}: ticks after apply_force")
        # a collision tick is pending (it writes the same columns): the device call settles it first, as the host call does
        f = torch.tensor(forces(rng, 1, COUNT)[0], device=dev)
        a.apply_force(FIRST, COUNT, f.cpu().numpy())
        T.apply_force(b, f, FIRST)
        assert same(b.get_external_force(), a.get_external_force())
        assert same(b.get_external_force(FIRST, COUNT), f.cpu().numpy())
        for g in (a, b):
            g.step_n(DT, 2)
            g.tick_n(DT, 3, True, True, REBOUNCE)
        assert_same_state(a, b, f"{scen}: apply_force over a pending collision tick")
        # and so does the force rollout: block 0 replaces the pending tick's force for the range, as the loop's first apply_force would
        cmd = torch.tensor(commands(O.ACTUATOR_CMD, rng, 3, COUNT, None), device=dev)
        frc = torch.tensor(forces(rng, 2, COUNT), device=dev)
        want = force_loop(a, O.ACTUATOR_CMD, cmd, frc, T.OBS_ALL, FIRST, torch.float64, 2, 3, 3)
        got = T.rollout(b, O.ACTUATOR_CMD, cmd, DT, T.OBS_ALL, first=FIRST, hold=2, obs_every=3, forces=frc, force_hold=3)
        assert raw_equal(got, want)
        for g in (a, b):
            g.tick_n(DT, 4, True, False, REBOUNCE)
        assert_same_state(a, b, f"{scen}: a force rollout over a pending collision tick, and ticks after it")


def test_refused_calls_change_nothing(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL)
    dev = torch_dev(g)
    before = T.save(g).cpu().numpy()
    # 12 steps of 100 UAVs: 4 command row blocks of 10 FP64 (held for 3 steps), 3 observation row blocks of 36 FP64 (every 4 steps), 6 force
    # row blocks of stride 4 (every 2 steps)
    hip, cmd = _hip_malloc(4 * 100 * 10 * 8)
    _, obs = _hip_malloc(3 * 100 * 36 * 8)
    _, frc = _hip_malloc(((6 * 100 - 1) * 4 + 3) * 8)         # exactly the 6 blocks: the last row has no padding
    _, frc_short = _hip_malloc(((6 * 100 - 2) * 4 + 3) * 8)   # one row short
    _, obs_short = _hip_malloc((3 * 100 - 1) * 36 * 8)
    _, cmd_short = _hip_malloc((4 * 100 - 1) * 10 * 8)
    bufs = (cmd, obs, frc, frc_short, obs_short, cmd_short)
    host = np.zeros((6, 100, 4))
    ok = dict(first=0, count=100, mode=O.POSITION_CMD, dt=DT, n_steps=12, cmd_every=3, obs_every=4, force_every=2, dev_cmd=cmd, dtype=T.DTYPE_F64,
              cmd_stride=10, dev_force=frc, force_stride=4, groups=T.OBS_ALL, dev_obs=obs, obs_stride=36, ext_stream=None)
    bad = [({"force_every": 0}, 1), ({"force_every": -1}, 1), ({"force_every": 5}, 1), ({"force_every": 24}, 1), ({"force_every": 1}, 1),
           ({"dev_force": frc_short}, 1), ({"dev_force": None}, 1), ({"dev_force": host.ctypes.data}, 1), ({"force_stride": 2}, 1),
           ({"force_stride": 0}, 1), ({"force_stride": 5}, 1),  # (force_every 1 / force_stride 5: more than the buffer holds)
           ({"cmd_every": 0}, 1), ({"cmd_every": -1}, 1), ({"obs_every": 0}, 1), ({"obs_every": -1}, 1), ({"cmd_every": 5}, 1), ({"obs_every": 5}, 1),
           ({"cmd_every": 24}, 1), ({"obs_every": 24}, 1), ({"dev_obs": obs_short}, 1), ({"dev_cmd": cmd_short}, 1), ({"dev_obs": None}, 1),
           ({"dev_cmd": None}, 1), ({"cmd_every": 2}, 1), ({"obs_every": 3}, 1), ({"obs_every": 1}, 1), ({"n_steps": 24}, 1), ({"n_steps": 0}, 1),
           ({"first": N_SINGLE - 5}, 3), ({"count": -1}, 3), ({"mode": 11}, 1), ({"dtype": 2}, 1), ({"dt": 0.0}, 1), ({"cmd_stride": 3}, 1),
           ({"groups": 0x100}, 1), ({"obs_stride": 35}, 1)]
    for change, code in bad:
        with pytest.raises(mrs.MrsError, match=f"error {code}:"):
            g.rollout_force_device(**dict(ok, **change))
        assert np.array_equal(T.save(g).cpu().numpy(), before), change
    ok_a = dict(first=0, count=100, dev_force=frc, dtype=T.DTYPE_F64, stride=4, ext_stream=None)
    _, one_short = _hip_malloc(((100 - 2) * 4 + 3) * 8)
    _, one_exact = _hip_malloc(((100 - 1) * 4 + 3) * 8)
    bufs += (one_short, one_exact)
    for change, code in [({"first": N_SINGLE - 5}, 3), ({"count": -1}, 3), ({"dtype": 2}, 1), ({"stride": 2}, 1), ({"stride": 0}, 1),
                         ({"dev_force": None}, 1), ({"dev_force": host.ctypes.data}, 1), ({"dev_force": one_short}, 1)]:
        with pytest.raises(mrs.MrsError, match=f"error {code}:"):
            g.apply_force_device(**dict(ok_a, **change))
        assert np.array_equal(T.save(g).cpu().numpy(), before), change
    g.apply_force_device(**dict(ok_a, count=0))  # MRS_OK, and nothing changes
    assert np.array_equal(T.save(g).cpu().numpy(), before)
    back = np.zeros(3 * 100 * 36)
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(obs), back.nbytes, 2) == 0
    assert not back.any(), "a refused call wrote observation rows"
    # a sharded swarm refuses both calls, state and rows untouched
    group = mrs.LoopbackGroup(2)
    shards = []
    for r in range(2):
        s = mrs.Swarm(100)
        s.construct(0, 100, mrs.model_params("x500"), np.stack([np.arange(100) * 3.0 + 400 * r, np.zeros(100), np.full(100, 5.0)], axis=1))
        s.comm_init_loopback(group, r, 200)
        shards.append(s)
    tc = torch.zeros((2, 100, 4), dtype=torch.float64, device=dev)
    tf = torch.ones((4, 100, 3), dtype=torch.float64, device=dev)
    to = torch.zeros((1, 100, 10), dtype=torch.float64, device=dev)
    for s in shards:
        x = s.get_states()["x"]
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.rollout(s, O.POSITION_CMD, tc, DT, out=to, hold=4, obs_every=8, forces=tf, force_hold=2)
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.apply_force(s, tf[0])
        assert same(s.get_states()["x"], x) and not s.get_external_force().any()
    assert not to.any()
    for s in shards:
        s.close()
    group.close()
    # the exactly sized buffers are accepted — once the sentinel check has shown that nothing is touched outside the due rows
    require_sentinel(mrs)
    g.apply_force_device(**dict(ok_a, dev_force=one_exact))
    g.rollout_force_device(**ok)
    torch.cuda.synchronize(dev)
    assert not np.array_equal(T.save(g).cpu().numpy(), before)
    assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(obs), back.nbytes, 2) == 0
    assert back.reshape(3, 100, 36)[:, :, 9:18].any(axis=2).all(), "every due row was written (its rotation matrix is not zero)"
    for p in bufs:
        hip.hipFree(C.c_void_p(p))


def test_follows_the_oracle_under_gusts(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(197)
    n = 700
    p = helpers.Pair(mrs, n, arith=mrs.ARITH_LITERAL)
    p.construct(0, 400, "x500")
    p.construct(400, 300, "f550")
    st = helpers.random_state(rng, n, 6, tilted=True)
    st["motor_rpm"][:400, 4:] = 0.0
    p.set_state(0, n, st)
    p.both("set_input", 0, n, O.VELOCITY_HDG_CMD, np.tile([0.5, 0.0, 0.2, 0.1], (n, 1)))
    dev = torch_dev(p.g)
    for mode, first, count, blocks, hold, fhold in ((O.POSITION_CMD, 0, 350, 6, 5, 3), (O.ATTITUDE_RATE_CMD, 350, 100, 2, 10, 4),
                                                    (O.ACTUATOR_CMD, 450, 250, 6, 4, 12), (O.ACCELERATION_HDG_CMD, 100, 500, 5, 3, 1)):
        nm = 6 if first + count > 400 else 4
        steps = blocks * hold
        c = commands(mode, rng, blocks, count, p.g.get_states(first, count)["x"], n_motors=nm)
        f = forces(rng, steps // fhold, count)
        T.rollout(p.g, mode, torch.tensor(c, device=dev), DT, 0, first=first, hold=hold, forces=torch.tensor(f, device=dev), force_hold=fhold)
        for t in range(steps):
            if t % hold == 0:
                p.o.set_input(first, count, mode, c[t // hold])
            if t % fhold == 0:
                p.o.apply_force(first, count, f[t // fhold])
            p.o.step(DT)
        p.compare(RTOL_LITERAL, f"mode {mode} held for {hold} steps, a gust every {fhold}")
        assert same(p.g.get_external_force(), p.o.get_external_force())


@pytest.mark.parametrize("mode", ["ATTITUDE_RATE_CMD", "ACTUATOR_CMD"])
def test_mppi_fork_under_gusts(mrs, mode):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    m = getattr(O, mode)
    rng = np.random.default_rng(201)
    src = mrs.Swarm(10, arith=mrs.ARITH_LITERAL)
    src.construct(0, 10, mrs.model_params("x500"), np.stack([np.arange(10) * 5.0, np.zeros(10), np.full(10, 8.0)], axis=1))
    src.set_input(0, 10, O.ATTITUDE_RATE_CMD, np.tile([0.1, -0.2, 0.05, 0.6], (10, 1)))
    src.apply_force(0, 10, np.tile([1.0, 0.5, -0.5], (10, 1)))
    src.step_n(DT, 50)
    S, H, hold, j = 256, 8, 10, 3  # 80 steps: two launches
    plan = mrs.Swarm(S, arith=mrs.ARITH_LITERAL)
    plan.construct(0, S, mrs.model_params("x500"))
    dev = torch_dev(src)
    rec = T.save(src, j, 1)
    T.load(plan, rec, index=torch.zeros(S, dtype=torch.int32, device=dev))
    nominal = commands(m, rng, H, 1, None, n_motors=4, width=4)
    u = np.repeat(nominal, S, axis=1) + np.concatenate([np.zeros((H, 1, nominal.shape[2])), rng.normal(0, 0.05, (H, S - 1, nominal.shape[2]))], axis=1)
    wind = torch.tensor([2.0, -1.0, 0.5], dtype=torch.float64, device=dev)
    gust = wind[None, None, :] + 1.5 * torch.randn(H, S, 3, device=dev, dtype=torch.float64, generator=torch.Generator(dev).manual_seed(5))
    own_gust = forces(rng, H, 1)[:, 0]  # sample 0: the real UAV's own force sequence
    gust[:, 0] = torch.tensor(own_gust, device=dev)
    obs = T.rollout(plan, m, torch.tensor(u, device=dev), DT, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, first=0, hold=hold, forces=gust, force_hold=hold)
    assert obs.shape == (H, S, 10)
    cost = obs[:, :, 2].sum(0)  # a cost in torch: the samples are ranked without leaving the device
    assert cost.shape == (S,)
    own, calm = [], src.clone()
    for t in range(H):
        src.set_input(j, 1, m, nominal[t])
        src.apply_force(j, 1, own_gust[t][None])
        src.step_n(DT, hold)
        own.append(T.gather(src, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, j, 1, dtype=torch.float64)[0])
        calm.set_input(j, 1, m, nominal[t])
        calm.step_n(DT, hold)
    o = obs.cpu().numpy()
    assert same(o[:, 0, :], torch.stack(own).cpu().numpy()), "sample 0 is the source UAV's own continuation"
    assert not same(src.get_states(j, 1)["x"], calm.get_states(j, 1)["x"]), "the gusts moved nothing"
    assert (np.abs(o[-1, 1:, :3] - o[-1, :1, :3]).max(axis=1) > 0).all(), "perturbed samples differ"


def test_caller_stream_is_fenced(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    a, b, c = (variant_swarm(mrs, "cascade", mrs.ARITH_LITERAL) for _ in range(3))
    dev = torch_dev(a)
    rng = np.random.default_rng(203)
    src = torch.tensor(commands(O.ATTITUDE_RATE_CMD, rng, 9, COUNT, None), device=dev)
    fsrc = torch.tensor(forces(rng, 12, COUNT), device=dev)
    want = T.rollout(a, O.ATTITUDE_RATE_CMD, src, DT, T.OBS_ALL, first=FIRST, hold=4, forces=fsrc, force_hold=3).cpu().numpy()
    assert want.shape[0] == 9
    for g, side in ((b, torch.cuda.Stream(dev)), (c, torch.cuda.ExternalStream(c.stream(), device=dev))):
        cmd, frc = torch.zeros_like(src), torch.zeros_like(fsrc)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
            cmd.copy_(src)  # written on the caller stream right before the call, no synchronisation
            frc.copy_(fsrc)
            out = T.rollout(g, O.ATTITUDE_RATE_CMD, cmd, DT, T.OBS_ALL, first=FIRST, hold=4, forces=frc, force_hold=3)
            copy = out.clone()  # torch work after the call sees the rows
            f1 = torch.zeros((COUNT, 3), dtype=torch.float64, device=dev)
            f1.copy_(fsrc[5])
            T.apply_force(g, f1, FIRST)
        side.synchronize()
        assert same(copy.cpu().numpy(), want)
        assert same(g.get_external_force(FIRST, COUNT), fsrc[5].cpu().numpy())
    a.apply_force(FIRST, COUNT, fsrc[5].cpu().numpy())
    for g in (b, c):
        assert_same_state(a, g, "fenced force rollout and apply_force")


def child_main(out_path):
    """the pointer-addressed kernels (MRS_NO_BUFFER_ADDRESSING=1): cascade, model-only and mixed-block force rollouts equal the loop in
    LITERAL, and FAST equals apply_force + the rate rollout for one force held over the run"""
    import torch
    import mrs_multirotor_simulator_amd as M
    from mrs_multirotor_simulator_amd import tensors as T
    M.load_library()
    rng = np.random.default_rng(207)
    res = []
    for scen, mode in (("cascade", O.VELOCITY_HDG_CMD), ("model", O.ACTUATOR_CMD)):
        for hold, every, fhold, steps in ((3, 6, 4, 132), (70, 35, 140, 140), (2, 2, 70, 140)):
            a, b, calm = (variant_swarm(M, scen, M.ARITH_LITERAL) for _ in range(3))
            dev = torch_dev(a)
            cmd = torch.tensor(commands(mode, rng, steps // hold, COUNT, a.get_states(FIRST, COUNT)["x"]), dtype=torch.float32, device=dev)
            frc = torch.tensor(forces(rng, steps // fhold, COUNT, (0, 40, float("nan"))), dtype=torch.float32, device=dev)
            want = force_loop(a, mode, cmd, frc, T.OBS_ALL, FIRST, torch.float32, hold, every, fhold)
            got = T.rollout(b, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every, forces=frc, force_hold=fhold)
            assert raw_equal(got, want), f"LITERAL {scen} hold {hold}"
            assert_same_state(a, b, f"LITERAL {scen} hold {hold}")
            unforced = T.rollout(calm, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every)
            assert differing(got, unforced) > 0.5, f"LITERAL {scen} hold {hold}: the forced rows are the unforced twin's"
            f1, f2 = variant_swarm(M, scen, M.ARITH_FAST), variant_swarm(M, scen, M.ARITH_FAST)
            one = T.rollout(f1, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every,
                            forces=frc[-1:].repeat(steps // fhold, 1, 1).contiguous(), force_hold=fhold)
            f2.apply_force(FIRST, COUNT, frc[-1].double().cpu().numpy())
            rate = T.rollout(f2, mode, cmd, DT, T.OBS_ALL, first=FIRST, hold=hold, obs_every=every)
            assert raw_equal(one, rate), f"FAST {scen} hold {hold}"
            assert_same_state(f1, f2, f"FAST {scen} hold {hold}")
        res.append(scen)
    np.save(out_path, np.array(res))


def test_pointer_form(mrs, tmp_path):
    if R._dead:
        pytest.fail(f"an earlier child process died ({R._dead[0]}): no further GPU process is started")
    out = str(tmp_path / "pointer.npy")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MRS_")}
    env["MRS_NO_BUFFER_ADDRESSING"] = "1"
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_rollout_force_gpu as T; T.child_main({out!r})"
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
    require_sentinel(mrs)  # (the C++ test hands the library force rows of exactly the due size)
    n, B, hold, every, fhold = 1000, 6, 10, 20, 5
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rollout_force.bin")
        try:
            out = subprocess.run([build_cpp("rollout_force_test"), path], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            R._dead.append(f"rollout_force_test timed out after {CHILD_TIMEOUT} s")
            pytest.fail(R._dead[0])
        print(out.stdout)
        if out.returncode < 0:
            R._dead.append(f"rollout_force_test ended by signal {-out.returncode}")
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok steady_force_equals_apply_force_and_the_rate_rollout", "ok the_force_moves_every_uav", "ok last_row_equals_pose_array",
                    "ok last_force_block_is_left_behind", "ok apply_force_device_equals_apply_force", "ok refused_call_changes_nothing", "ok written"):
            assert tag in out.stdout, out.stdout
        raw = np.fromfile(path, np.float64)
    i = np.arange(n)
    pos = np.stack([4.0 * (i % 32), 4.0 * (i // 32), np.full(n, 5.0)], axis=1)
    g = mrs.Swarm(n, arith=mrs.ARITH_FAST)  # (the facade's default)
    g.construct(0, n, mrs.default_params(), pos, 0.003 * i)
    t = np.arange(B)[:, None]
    cmd = np.stack([np.broadcast_to(0.02 * np.sin(0.1 * t + 0.001 * i), (B, n)), np.broadcast_to(-0.01 + 0.0 * t + 0.0 * i, (B, n)),
                    np.broadcast_to(0.3 + 0.0001 * i + 0.0 * t, (B, n)), np.broadcast_to(0.55 + 0.005 * t + 0.0 * i, (B, n))], axis=2)
    Bf = B * hold // fhold
    t = np.arange(Bf)[:, None]
    gust = np.stack([0.5 * (t % 5) - 1.0 + 0.004 * i, np.broadcast_to(-1.5 + 0.25 * t + 0.0 * i, (Bf, n)),
                     np.where(t % 3 == 0, 0.0, np.broadcast_to(0.002 * i - 1.0, (Bf, n)))], axis=2)
    dev = torch_dev(g)
    mine = T.rollout(g, O.ATTITUDE_RATE_CMD, torch.tensor(cmd, device=dev), DT, T.OBS_POS | T.OBS_VEL | T.OBS_QUAT, hold=hold, obs_every=every,
                     forces=torch.tensor(gust, device=dev), force_hold=fhold).cpu().numpy()
    assert mine.shape == (B * hold // every, n, 10)
    assert raw.shape == (mine.size,) and same(raw, mine.reshape(-1))
