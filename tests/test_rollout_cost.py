"""CPU-side checks of cost rollouts (include/mrs_swarm.h, "cost rollouts"): mrs_swarm_rollout_cost_device is exported and listed, its header
prototype, its ctypes argtypes and the parameters of Swarm.rollout_cost_device agree, tensors.rollout_cost refuses CPU tensors, wrong
dtypes, a wrong number of evaluations, target and weight shapes it cannot address, groups == 0, bad rates and accumulate without `out`
before the library is reached, a well-formed call reaches rollout_cost_device and nothing else, and tests/cpp/rollout_cost_test.cpp
compiles.  CPU tensors only: no pointer reaches the library.

The cost has kernels of its own (the _cost family of helpers.rollout_kernels): every one of them has a row in
test_rollout_cost_gpu.ROLLOUT_COST_KERNELS, one per rate kernel, and none of them belongs to one of the three families before it."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

import test_rollout_cost_gpu as RC
from helpers import CTYPE, ROOT, abi_prototype, fake_cuda, rollout_kernels, stand_in

NAMES = ["s", "first", "count", "mode", "dt", "n_steps", "cmd_every", "cost_every", "dev_cmd", "dtype", "cmd_stride", "groups", "dev_target",
         "target_stride", "dev_weight", "weight_stride", "dev_cost", "accumulate", "ext_stream"]


def test_symbol_is_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm
    assert hasattr(C.CDLL(swarm.LIB_PATH), "mrs_swarm_rollout_cost_device")
    assert "mrs_swarm_rollout_cost_device" in swarm.ABI_SYMBOLS
    assert callable(getattr(swarm.Swarm, "rollout_cost_device", None))


def test_header_prototype_argtypes_and_method_agree(mrs):
    from mrs_multirotor_simulator_amd import swarm
    names, types = abi_prototype("mrs_swarm_rollout_cost_device")
    assert names == NAMES
    ctype = dict(CTYPE, **{"double*": C.c_void_p})  # (the cost vector travels as an address, like every device pointer)
    got = swarm.load_library().mrs_swarm_rollout_cost_device.argtypes
    assert [ctype[t] for t in types] == list(got), (types, got)
    assert types[NAMES.index("dev_cost")] == "double*"
    # the method takes the prototype's parameters behind the handle, under the same names
    assert list(inspect.signature(swarm.Swarm.rollout_cost_device).parameters) == ["self"] + NAMES[1:]
    # the rate call keeps its prototype: the new one shares its head up to the groups
    rate = swarm.load_library().mrs_swarm_rollout_rate_device.argtypes
    assert list(got[:12]) == list(rate[:12])


# a refused call reaches no library call, a well-formed one reaches rollout_cost_device only
_Swarm = stand_in("rollout_device", "rollout_rate_device", "rollout_force_device", "rollout_cost_device")


def test_rollout_cost_refuses_before_the_library(monkeypatch):
    """CPU tensors dressed as cuda tensors (only .device is faked; nothing is launched)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64, f32, pos = _Swarm(), torch.float64, torch.float32, T.OBS_POS  # (mode 10: POSITION_CMD; OBS_POS: w = 3)

    def z(*shape, dtype=f64, dev=0):
        return on(torch.zeros(*shape, dtype=dtype), dev)

    cmd, tg, wt, out = z(6, 10, 4), z(3, 10, 3), z(3, 3), z(10)  # B = 6, hold = 2: 12 steps, cost_every = 4: E = 3
    kw = dict(hold=2, cost_every=4)
    cases = [
        # CPU tensors and other devices
        (dict(commands=torch.zeros(6, 10, 4, dtype=f64)), "is on cpu"),
        (dict(targets=torch.zeros(3, 10, 3, dtype=f64)), "is on cpu"),
        (dict(weights=torch.zeros(3, 3, dtype=f64)), "is on cpu"),
        (dict(out=torch.zeros(10, dtype=f64)), "is on cpu"),
        (dict(targets=z(3, 10, 3, dev=1)), "the swarm lives on cuda:0"),
        # dtypes
        (dict(commands=z(6, 10, 4, dtype=torch.float16)), "float32 or torch.float64"),
        (dict(targets=z(3, 10, 3, dtype=f32)), "targets has dtype torch.float32, the commands torch.float64"),
        (dict(weights=z(3, 3, dtype=f32)), "weights has dtype torch.float32, the commands torch.float64"),
        (dict(commands=z(6, 10, 4, dtype=f32)), "targets has dtype torch.float64, the commands torch.float32"),
        (dict(out=z(10, dtype=f32)), "the cost vector is always torch.float64"),
        # the number of evaluations, and the shapes
        (dict(targets=z(4, 10, 3)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(6, 10, 3)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(3, 10, 2)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(3, 5, 3)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(3, 11, 3)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(10, 3)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(3, 1, 5)[:, :, :3]), "targets: shared rows must be dense"),
        (dict(targets=z(3, 3, 2).transpose(1, 2)[:, :1]), "rows are not contiguous"),
        (dict(targets=z(3, 3, 10).transpose(1, 2)), "rows are not contiguous"),
        (dict(targets=z(6, 10, 3)[::2]), "step dimension is not dense"),
        (dict(weights=z(2, 3)), r"weights: expected a \[3 or 1, >= 3\]"),
        (dict(weights=z(4, 3)), r"weights: expected a \[3 or 1, >= 3\]"),
        (dict(weights=z(3)), r"weights: expected a \[3 or 1, >= 3\]"),
        (dict(weights=z(3, 2)), r">= 3\] matrix"),
        (dict(weights=z(3, 3).t()), "rows are not contiguous"),
        (dict(out=z(9)), "vector of 10 elements"),
        (dict(out=z(10, 2)), "vector of 10 elements"),
        (dict(out=z(20)[::2]), "not contiguous"),
        # groups, rates, accumulate
        (dict(groups=0), "at least one observation group"),
        (dict(hold=0), "hold must be at least 1"),
        (dict(cost_every=0), "cost_every must be at least 1 and divide the 12 steps"),
        (dict(cost_every=-4), "cost_every must be at least 1 and divide the 12 steps"),
        (dict(cost_every=5), "cost_every must be at least 1 and divide the 12 steps"),
        (dict(cost_every=24), "cost_every must be at least 1 and divide the 12 steps"),
        (dict(hold=3, cost_every=None, targets=z(3, 10, 3)), r"\[6, 10 or 1, >= 3\]"),  # cost_every defaults to hold: 18 steps, E = 6
        (dict(out=None, accumulate=True), "accumulate=True needs the `out` vector"),
        (dict(commands=[[[0.0] * 4] * 10] * 6), "commands must be"),
    ]
    for change, msg in cases:
        a = dict(dict(commands=cmd, groups=pos, targets=tg, weights=wt, out=out, accumulate=False), **kw)
        a.update(change)
        with pytest.raises(ValueError, match=msg):
            T.rollout_cost(g, 10, a.pop("commands"), 0.001, a.pop("groups"), a.pop("targets"), a.pop("weights"), **a)
    with pytest.raises(ValueError, match="actuator rows must be dense"):
        T.rollout_cost(g, T.ACTUATOR_CMD, z(6, 10, 6)[:, :, :4], 0.001, pos, tg, wt, out=out, **kw)
    # well-formed calls pass every check of the tensor layer and reach rollout_cost_device, whatever the rates are
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    for a in (dict(targets=tg, weights=wt, out=out, **kw), dict(targets=z(3, 1, 3), weights=z(1, 3), out=out, **kw),
              dict(targets=z(3, 10, 7)[:, :, :3], weights=z(3, 8)[:, :3], out=z(30)[5:15], accumulate=True, **kw),
              dict(targets=z(6, 10, 3), weights=z(6, 3), hold=1, cost_every=1, out=out), dict(targets=z(6, 10, 3), weights=z(1, 5), out=out)):
        with pytest.raises(AssertionError, match=r"\(rollout_cost_device\)"):
            T.rollout_cost(g, 10, cmd, 0.001, pos, a.pop("targets"), a.pop("weights"), **a)


def test_strides_handed_to_the_library(monkeypatch):
    """shared targets travel as target_stride 0, a single weight row as weight_stride 0, padded rows with their strides"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    seen = []

    class Rec(_Swarm):
        def rollout_cost_device(self, *a):
            seen.append(a)

    def z(*shape):
        return on(torch.zeros(*shape, dtype=torch.float64))

    cmd = z(6, 10, 4)
    T.rollout_cost(Rec(), 10, cmd, 0.001, T.OBS_POS, z(3, 10, 7)[:, :, :3], z(3, 8)[:, :3], hold=2, cost_every=4, first=5, out=z(10))
    T.rollout_cost(Rec(), 10, cmd, 0.001, T.OBS_POS, z(3, 1, 3), z(1, 8)[:, :3], hold=2, cost_every=4, out=z(10), accumulate=True)
    assert all(len(s) == len(NAMES) - 1 for s in seen)
    a, b = (dict(zip(NAMES[1:], s)) for s in seen)
    assert (a["first"], a["count"], a["n_steps"], a["cmd_every"], a["cost_every"]) == (5, 10, 12, 2, 4)
    assert (a["target_stride"], a["weight_stride"], a["accumulate"], a["groups"]) == (7, 8, False, T.OBS_POS)
    assert (b["target_stride"], b["weight_stride"], b["accumulate"]) == (0, 0, True)


def test_every_rollout_cost_kernel_has_a_row():
    """one cost kernel per rate kernel, with its shape and launch bounds, compiled by both step units behind the force family"""
    import test_rollout_rate_gpu as RR
    k = rollout_kernels()
    k.check_family("_cost", RC.ROLLOUT_COST_KERNELS, RC, mirrors="_rate")
    assert set(k.families["_rate"]) == set(RR.ROLLOUT_RATE_KERNELS)
    assert list(k.families).index("_force") < list(k.families).index("_cost")
    assert not set(k.families["_cost"]) & (set(k.families[""]) | set(k.families["_rate"]) | set(k.families["_force"]))


def test_restatement_helper_is_the_stated_loop():
    """test_rollout_cost_gpu.restate against the scalar loop of the ABI comment, with shared and per-UAV rows, FP32 inputs and a start"""
    import numpy as np
    rng = np.random.default_rng(5)
    E, count, w = 3, 4, 5
    rows = rng.normal(size=(E, count, w))
    for tg, wt, start in ((rng.normal(size=(E, count, w + 2)), rng.normal(size=(E, w + 1)), None),
                          (rng.normal(size=(E, 1, w)).astype(np.float32), rng.normal(size=(1, w)).astype(np.float32), rng.normal(size=count))):
        want = np.zeros(count)
        for k in range(count):
            c = 0.0 if start is None else float(start[k])
            for j in range(E):
                term = 0.0
                for col in range(w):
                    d = float(rows[j, k, col]) - float(tg[j, k if tg.shape[1] > 1 else 0, col])
                    term = term + (float(wt[j if wt.shape[0] > 1 else 0, col]) * d) * d
                c = c + term
            want[k] = c
        assert np.array_equal(RC.restate(rows, tg, wt, start).view(np.uint64), want.view(np.uint64))
    assert RC.cost_equal(np.array([1.0, np.nan]), np.array([1.0, -np.nan])) and not RC.cost_equal(np.array([1.0, 2.0]), np.array([1.0, np.nan]))
    assert not RC.cost_equal(np.array([0.0]), np.array([-0.0]))


def test_rollout_cost_test_compiles(mrs, tmp_path):
    from mrs_multirotor_simulator_amd import swarm
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DMRS_NO_EIGEN", "-D__HIP_PLATFORM_AMD__", "-I",
                           os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "rollout_cost_test.cpp"),
                           "-o", str(tmp_path / "rollout_cost_test"), "-L", os.path.dirname(swarm.LIB_PATH), "-lmrs_swarm", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-lpthread"])
