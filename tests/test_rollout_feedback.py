"""CPU-side checks of feedback rollouts (include/mrs_swarm.h, "feedback rollouts"): the numpy restatement the GPU tests use is the scalar
loop of the contract (both gain layouts, one block for the call and one per command block, FP32 inputs widened, a non-finite residual under
a zero gain); mrs_swarm_rollout_feedback_device is declared, exported and listed, and its header prototype, its ctypes argtypes and the
parameters of Swarm.rollout_feedback_device agree; the width helpers refuse unknown group bits; tensors.rollout_feedback refuses what it
cannot address before the library is reached and hands the strides on; tests/cpp/rollout_feedback_test.cpp compiles.  CPU tensors only:
no pointer reaches the library.

The call has kernels of its own (the _feedback family of helpers.rollout_kernels): every one of them has a row in
test_rollout_feedback_gpu.FEEDBACK_KERNELS, one per cost kernel, and none of them belongs to another family or to the tick kernels."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import test_rollout_feedback_gpu as RF
from helpers import CTYPE, ROOT, abi_prototype, fake_cuda, rollout_kernels, stand_in

NAMES = ["s", "first", "count", "mode", "dt", "n_steps", "cmd_every", "cost_every", "dev_cmd", "dtype", "cmd_stride", "fb_groups", "dev_gain",
         "gain_per_uav", "gain_blocks", "dev_ref", "ref_stride", "ref_blocks", "cost_groups", "dev_target", "target_stride", "dev_weight",
         "weight_stride", "dev_cost", "accumulate", "ext_stream"]


def scalar_feedback(obs, cmd, gains, refs, b):
    """the contract, one Python float operation at a time: e[j] = ref - o, then per payload element the sum over ascending j"""
    count, wo = obs.shape
    wc = gains.shape[1]
    gb, rb = (b if gains.shape[0] > 1 else 0), (b if refs.shape[0] > 1 else 0)
    u = np.empty((count, wc))
    for k in range(count):
        e = [float(refs[rb, k if refs.shape[1] > 1 else 0, j]) - float(obs[k, j]) for j in range(wo)]
        for c in range(wc):
            acc = float(cmd[b, k, c])
            for j in range(wo):
                g = float(gains[gb, c, j, k]) if gains.ndim == 4 else float(gains[gb, c, j])
                acc = acc + (g * e[j])
            u[k, c] = acc
    return u


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("ref_blocks", [False, True])
@pytest.mark.parametrize("gain_blocks", [False, True])
@pytest.mark.parametrize("per_uav", [False, True])
def test_restatement_helper_is_the_stated_loop(per_uav, gain_blocks, ref_blocks, f32):
    rng = np.random.default_rng(7 + per_uav + 2 * gain_blocks + 4 * ref_blocks + 8 * f32)
    B, count, wo, wc = 3, 5, 7, 4
    dt = np.float32 if f32 else np.float64
    cmd = rng.normal(size=(B, count, wc + 2)).astype(dt)  # (padded rows: the payload is the first wc columns)
    gains = rng.normal(size=(B if gain_blocks else 1, wc, wo) + ((count,) if per_uav else ())).astype(dt)
    refs = rng.normal(size=(B if ref_blocks else 1, 1 if per_uav == ref_blocks else count, wo + 1)).astype(dt)
    for b in range(B):
        obs = rng.normal(size=(count, wo)) * 10.0
        got = RF.restate_feedback(obs, cmd, gains, refs, b)
        assert got.shape == (count, wc) and got.dtype == np.float64
        assert same_bits(got, scalar_feedback(obs, cmd, gains, refs, b))


def test_a_zero_gain_does_not_mask_a_non_finite_residual():
    obs = np.array([[1.0, np.inf, 2.0], [1.0, 5.0, np.nan], [1.0, 2.0, 3.0]])
    cmd = np.array([[[0.5, -0.5]] * 3])
    gains = np.array([[[1.0, 0.0, 0.0], [0.0, 0.0, 2.0]]])  # payload 0 reads column 0 only, payload 1 column 2 only
    refs = np.zeros((1, 1, 3))
    u = RF.restate_feedback(obs, cmd, gains, refs)
    assert same_bits(u, scalar_feedback(obs, cmd, gains, refs, 0))
    assert np.isnan(u[0]).all(), "0 * inf is NaN: a zero gain does not mask a column"
    assert np.isnan(u[1]).all(), "0 * NaN is NaN"
    assert np.array_equal(u[2], [0.5 + 1.0 * (0.0 - 1.0), -0.5 + 2.0 * (0.0 - 3.0)])
    # the residual is ref - obs
    assert RF.restate_feedback(np.array([[2.0]]), np.zeros((1, 1, 1)), np.ones((1, 1, 1)), np.full((1, 1, 1), 5.0))[0, 0] == 3.0


def test_a_nan_observation_reaches_the_command_with_its_own_bits():
    """what the kernels pin (obs_row.h: mrs_obs_row_feedback): host arithmetic hands a NaN operand on with its sign and payload, so
    the restatement of a UAV whose state is NaN writes that NaN, and the GPU reference (computed on the host) compares bit for bit"""
    for nan_bits in (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000123):
        obs = np.array([[1.0, 0.0, 2.0]])
        obs.view(np.uint64)[0, 1] = nan_bits
        u = RF.restate_feedback(obs, np.array([[[0.5, -0.5]]]), np.array([[[1.0, -3.0, 0.0], [0.0, 2.0, 2.0]]]), np.ones((1, 1, 3)))
        assert (u.view(np.uint64) == nan_bits).all(), [hex(x) for x in u.view(np.uint64).ravel()]


def test_symbol_is_declared_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm
    assert hasattr(C.CDLL(swarm.LIB_PATH), "mrs_swarm_rollout_feedback_device")
    assert "mrs_swarm_rollout_feedback_device" in swarm.ABI_SYMBOLS
    assert callable(getattr(swarm.Swarm, "rollout_feedback_device", None))
    header = open(os.path.join(ROOT, "include", "mrs_swarm.h")).read()
    assert "int mrs_swarm_rollout_feedback_device(" in header and "UAV-MINOR" in header


def test_header_prototype_argtypes_and_method_agree(mrs):
    from mrs_multirotor_simulator_amd import swarm
    names, types = abi_prototype("mrs_swarm_rollout_feedback_device")
    assert names == NAMES
    ctype = dict(CTYPE, **{"double*": C.c_void_p})
    got = swarm.load_library().mrs_swarm_rollout_feedback_device.argtypes
    assert [ctype[t] for t in types] == list(got), (types, got)
    assert list(inspect.signature(swarm.Swarm.rollout_feedback_device).parameters) == ["self"] + NAMES[1:]
    # the cost call keeps its prototype: the new one shares its head up to the command stride and its tail from the cost groups on
    cost = swarm.load_library().mrs_swarm_rollout_cost_device.argtypes
    assert list(got[:11]) == list(cost[:11]) and list(got[18:]) == list(cost[11:])


def test_width_helpers_refuse_unknown_group_bits(mrs):
    from mrs_multirotor_simulator_amd import tensors as T
    assert T.gather_width(T.OBS_OMEGA) == 3 and T.gather_width(T.OBS_POS | T.OBS_VEL | T.OBS_ROT | T.OBS_OMEGA) == 18
    assert T.gather_width(T.OBS_ALL) == 36 and T.gather_width(0) == 0
    for bad in (0x100, T.OBS_ALL + 1, 1 << 31):
        with pytest.raises(Exception):
            T.gather_width(bad)
    assert [T.command_width(m, 8) for m in range(11)] == [0, 8, 4, 4, 10, 5, 4, 4, 4, 4, 4]


# a refused call reaches no library call, a well-formed one reaches rollout_feedback_device only
_Swarm = stand_in("rollout_cost_device", "rollout_feedback_device")


def test_rollout_feedback_refuses_before_the_library(monkeypatch):
    """CPU tensors dressed as cuda tensors (only .device is faked; nothing is launched)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64, f32 = _Swarm(), torch.float64, torch.float32
    fb, pos = T.OBS_POS | T.OBS_OMEGA, T.OBS_POS  # W_o = 6; cost columns: 3; mode 10 (POSITION_CMD): W_c = 4

    def z(*shape, dtype=f64, dev=0):
        return on(torch.zeros(*shape, dtype=dtype), dev)

    cmd, tg, wt, out = z(6, 10, 4), z(3, 10, 3), z(3, 3), z(10)  # B = 6, hold = 2: 12 steps, cost_every = 4: E = 3
    ok = dict(mode=10, commands=cmd, fb_groups=fb, gains=z(6, 4, 6, 10), refs=z(6, 10, 6), cost_groups=pos, targets=tg, weights=wt, out=out, hold=2,
              cost_every=4)
    cases = [
        (dict(gains=torch.zeros(6, 4, 6, 10, dtype=f64)), "gains is on cpu"),
        (dict(refs=torch.zeros(6, 10, 6, dtype=f64)), "is on cpu"),
        (dict(gains=z(6, 4, 6, 10, dev=1)), "the swarm lives on cuda:0"),
        (dict(gains=z(6, 4, 6, 10, dtype=f32)), "gains has dtype torch.float32, the commands torch.float64"),
        (dict(refs=z(6, 10, 6, dtype=f32)), "refs has dtype torch.float32, the commands torch.float64"),
        (dict(commands=z(6, 10, 4, dtype=f32)), "gains has dtype torch.float64, the commands torch.float32"),
        # a wrong Bg, wrong shapes
        (dict(gains=z(3, 4, 6, 10)), r"gains: expected a \[6 or 1, 4, 6, 10\]"),
        (dict(gains=z(2, 4, 6)), r"gains: expected a \[6 or 1, 4, 6\]"),
        (dict(gains=z(6, 10, 4, 6)), r"gains: expected a \[6 or 1, 4, 6, 10\]"),  # (a matrix per UAV row: not UAV-minor)
        (dict(gains=z(6, 6, 4)), r"gains: expected a \[6 or 1, 4, 6\]"),
        (dict(gains=z(4, 6)), "gains: expected a"),
        (dict(refs=z(3, 10, 6)), r"refs: expected a \[6 or 1, 10 or 1, >= 6\]"),
        (dict(refs=z(6, 10, 5)), r"refs: expected a \[6, 10 or 1, >= 6\]"),
        (dict(refs=z(6, 5, 6)), r"refs: expected a \[6, 10 or 1, >= 6\]"),
        (dict(refs=z(6, 1, 8)[:, :, :6]), "shared rows must be dense"),
        # non-dense gains
        (dict(gains=z(6, 10, 4, 6).permute(0, 2, 3, 1)), "gains must be dense"),
        (dict(gains=z(6, 4, 6, 20)[..., ::2]), "gains must be dense"),
        (dict(gains=z(6, 4, 8)[:, :, :6]), "gains must be dense"),
        # W_o = 0, a payload-less mode, the rates, the cost side
        (dict(fb_groups=0), "fb_groups must select at least one observation group"),
        (dict(mode=T.INPUT_UNKNOWN), "needs a mode with a payload"),
        (dict(hold=0), "hold must be at least 1"),
        (dict(cost_every=5), "cost_every must be at least 1 and divide the 12 steps"),
        (dict(targets=z(4, 10, 3)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(weights=z(2, 3)), r"weights: expected a \[3 or 1, >= 3\]"),
        (dict(out=z(10, dtype=f32)), "the cost vector is always torch.float64"),
        (dict(out=None, accumulate=True), "accumulate=True needs the `out` vector"),
        (dict(cost_groups=0), "cost_groups == 0 is a run without a cost"),
    ]

    def call(a):
        a = dict(a)
        return T.rollout_feedback(g, a.pop("mode"), a.pop("commands"), 0.001, a.pop("fb_groups"), a.pop("gains"), a.pop("refs"), **a)

    for change, msg in cases:
        with pytest.raises(ValueError, match=msg):
            call(dict(ok, **change))
    # well-formed calls pass every check of the tensor layer and reach rollout_feedback_device
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    for change in (dict(), dict(gains=z(1, 4, 6), refs=z(1, 1, 6)), dict(gains=z(1, 4, 6, 10), refs=z(6, 1, 6)), dict(gains=z(6, 4, 6), refs=z(1, 10, 9)[:, :, :6]),
                   dict(cost_groups=0, targets=None, weights=None, out=None), dict(targets=z(3, 1, 3), weights=z(1, 3), out=z(30)[5:15], accumulate=True)):
        with pytest.raises(AssertionError, match=r"\(rollout_feedback_device\)"):
            call(dict(ok, **change))


def test_strides_handed_to_the_library(monkeypatch):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    seen = []

    class Rec(_Swarm):
        def rollout_feedback_device(self, *a):
            seen.append(a)

    def z(*shape):
        return on(torch.zeros(*shape, dtype=torch.float64))

    cmd, fb = z(6, 10, 4), T.OBS_POS | T.OBS_OMEGA
    T.rollout_feedback(Rec(), 10, cmd, 0.001, fb, z(6, 4, 6, 10), z(6, 10, 9)[:, :, :6], T.OBS_POS, z(3, 10, 7)[:, :, :3], z(3, 8)[:, :3], hold=2,
                       cost_every=4, first=5, out=z(10))
    assert T.rollout_feedback(Rec(), 10, cmd, 0.001, fb, z(1, 4, 6), z(1, 1, 6), hold=2) is None
    assert all(len(s) == len(NAMES) - 1 for s in seen)
    a, b = (dict(zip(NAMES[1:], s)) for s in seen)
    assert (a["first"], a["count"], a["n_steps"], a["cmd_every"], a["cost_every"]) == (5, 10, 12, 2, 4)
    assert (a["gain_per_uav"], a["gain_blocks"], a["ref_stride"], a["ref_blocks"], a["fb_groups"]) == (1, 6, 9, 6, fb)
    assert (a["cost_groups"], a["target_stride"], a["weight_stride"], a["accumulate"]) == (T.OBS_POS, 7, 8, False)
    assert (b["gain_per_uav"], b["gain_blocks"], b["ref_stride"], b["ref_blocks"], b["cost_every"]) == (0, 1, 0, 1, 2)
    assert (b["cost_groups"], b["dev_target"], b["dev_weight"], b["dev_cost"]) == (0, 0, 0, 0)


def test_every_feedback_kernel_has_a_row():
    """one feedback kernel per cost kernel, with its shape, compiled by both step units behind the cost family"""
    import test_rollout_cost_gpu as RC
    k = rollout_kernels()
    k.check_family("_feedback", RF.FEEDBACK_KERNELS, RF, mirrors="_cost")
    assert set(k.families["_cost"]) == set(RC.ROLLOUT_COST_KERNELS)
    others = [n for f, fam in k.families.items() if f != "_feedback" for n in fam] + list(k.tick)
    assert not set(k.families["_feedback"]) & set(others)


def test_rollout_feedback_test_compiles(mrs, tmp_path):
    from mrs_multirotor_simulator_amd import swarm
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DMRS_NO_EIGEN", "-D__HIP_PLATFORM_AMD__", "-I",
                           os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "rollout_feedback_test.cpp"),
                           "-o", str(tmp_path / "rollout_feedback_test"), "-L", os.path.dirname(swarm.LIB_PATH), "-lmrs_swarm", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-lpthread"])
