"""CPU-side checks of device-resident external forces (include/mrs_swarm.h, "device-resident external forces"):
mrs_swarm_apply_force_device and mrs_swarm_rollout_force_device are exported, listed and callable on Swarm, each header prototype equals
its ctypes argtypes and parameter names, tensors.rollout(forces=, force_hold=) and tensors.apply_force refuse bad tensors and rates before
the library is reached, a well-formed call with forces reaches rollout_force_device and nothing else, and
tests/cpp/rollout_force_test.cpp compiles.  CPU tensors only: no pointer reaches the library.

The forces have kernels of their own (the _force family of helpers.rollout_kernels): every one of them has a row in
test_rollout_force_gpu.ROLLOUT_FORCE_KERNELS and a rate counterpart, and the tables of the step, plain and rate kernels stay as they are."""
import ctypes as C
import os
import subprocess

import pytest

import test_rollout_force_gpu as RF
from helpers import CTYPE, ROOT, abi_prototype, fake_cuda, rollout_kernels, stand_in
from test_rollout_rate import NAMES as RATE_NAMES

# the rate call with force_every behind obs_every and dev_force, force_stride behind cmd_stride
NAMES = RATE_NAMES[:8] + ["force_every"] + RATE_NAMES[8:11] + ["dev_force", "force_stride"] + RATE_NAMES[11:]
APPLY_NAMES = ["s", "first", "count", "dev_force", "dtype", "stride", "ext_stream"]


def _prototype(name):
    names, types = abi_prototype(name)
    return names, [CTYPE[t] for t in types]


def test_symbols_are_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm
    for sym, method in (("mrs_swarm_apply_force_device", "apply_force_device"), ("mrs_swarm_rollout_force_device", "rollout_force_device")):
        assert hasattr(C.CDLL(swarm.LIB_PATH), sym), sym
        assert sym in swarm.ABI_SYMBOLS, sym
        assert callable(getattr(swarm.Swarm, method, None)), method


def test_header_prototypes_equal_the_argtypes(mrs):
    import inspect
    from mrs_multirotor_simulator_amd import swarm
    lib = swarm.load_library()
    names, types = _prototype("mrs_swarm_rollout_force_device")
    assert names == NAMES
    got = list(lib.mrs_swarm_rollout_force_device.argtypes)
    assert types == got, (types, got)
    # the rate call keeps its prototype: the new one is it with force_every behind obs_every and dev_force, force_stride behind cmd_stride
    rate = list(lib.mrs_swarm_rollout_rate_device.argtypes)
    assert got[:8] + got[9:12] + got[14:] == rate and got[8] == C.c_int32 and got[12:14] == [C.c_void_p, C.c_int32]
    names, types = _prototype("mrs_swarm_apply_force_device")
    assert names == APPLY_NAMES
    assert types == list(lib.mrs_swarm_apply_force_device.argtypes)
    # keyword names of the Swarm methods are the header's parameter names
    assert list(inspect.signature(swarm.Swarm.rollout_force_device).parameters)[1:] == NAMES[1:]
    assert list(inspect.signature(swarm.Swarm.apply_force_device).parameters)[1:] == APPLY_NAMES[1:]


_Swarm = stand_in("rollout_device", "rollout_rate_device", "rollout_force_device", "apply_force_device")


def test_rollout_refuses_bad_forces(monkeypatch):
    """CPU tensors dressed as cuda tensors (only .device is faked; nothing is launched)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64, pos = _Swarm(), torch.float64, T.OBS_POS  # (mode 10: POSITION_CMD)
    cmd = on(torch.zeros(5, 10, 4, dtype=f64))  # B = 5, hold = 2: 10 steps
    out = on(torch.zeros(5, 10, 3, dtype=f64))
    ok = on(torch.zeros(5, 10, 3, dtype=f64))
    cases = [
        (torch.zeros(5, 10, 3, dtype=f64), {}, "forces is on cpu"),                                     # CPU tensor
        (on(torch.zeros(5, 10, 3, dtype=f64), 1), {}, "forces is on cuda:1, the swarm lives on cuda:0"),  # another device
        (on(torch.zeros(5, 10, 3)), {}, "forces has dtype torch.float32, expected torch.float64"),       # not the commands' dtype
        (on(torch.zeros(5, 10, 2, dtype=f64)), {}, r"forces: expected a \[T, 10, >= 3\]"),               # narrower than 3
        (on(torch.zeros(10, 3, dtype=f64)), {}, r"forces: expected a \[T, 10, >= 3\]"),                  # no step dimension
        (on(torch.zeros(5, 9, 3, dtype=f64)), {}, r"forces: expected a \[T, 10, >= 3\]"),                # another count
        (on(torch.zeros(10, 5, 3, dtype=f64).transpose(0, 1)), {}, "forces: the step dimension is not dense"),
        (on(torch.zeros(10, 10, 3, dtype=f64)[::2]), {}, "forces: the step dimension is not dense"),
        (on(torch.zeros(5, 3, 10, dtype=f64).transpose(1, 2)), {}, "forces: rows are not contiguous"),
        ([[[0.0] * 3] * 10] * 5, {}, "forces: expected a torch.Tensor"),
        (ok, dict(force_hold=0), "force_hold must be at least 1"),
        (ok, dict(force_hold=-2), "force_hold must be at least 1"),
        (ok, dict(force_hold=1), "5 force blocks x force_hold must be the 10 steps"),                    # Bf * force_hold != steps
        (ok, dict(force_hold=5), "5 force blocks x force_hold must be the 10 steps"),
        (on(torch.zeros(3, 10, 3, dtype=f64)), {}, "3 force blocks x force_hold must be the 10 steps"),  # the default 10 // 3 does not fit
        (on(torch.zeros(20, 10, 3, dtype=f64)), {}, "force_hold must be at least 1"),                    # more blocks than steps
    ]
    for f, kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            T.rollout(g, 10, cmd, 0.001, pos, out=out, hold=2, forces=f, **kw)
    # a well-formed call passes every check of the tensor layer and reaches rollout_force_device, nothing else — also with
    # hold = obs_every = 1, where the unforced call runs the plain kernels
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    seen = []

    class Taking(_Swarm):
        def rollout_force_device(self, *a):
            seen.append(a)

    for kw, blocks, forces, want in ((dict(hold=2), 5, ok, (10, 2, 2, 2)), (dict(hold=2, force_hold=2), 5, ok, (10, 2, 2, 2)),
                                     (dict(hold=2, obs_every=5), 2, on(torch.zeros(10, 10, 5, dtype=f64)), (10, 2, 5, 1)),
                                     (dict(hold=1, obs_every=1), 5, on(torch.zeros(1, 10, 3, dtype=f64)), (5, 1, 1, 5)),
                                     (dict(), 5, ok, (5, 1, 1, 1))):
        del seen[:]
        T.rollout(Taking(), 10, cmd, 0.001, pos, out=on(torch.zeros(blocks, 10, 3, dtype=f64)), forces=forces, **kw)
        assert len(seen) == 1
        a = dict(zip(NAMES[1:], seen[0]))
        assert (a["n_steps"], a["cmd_every"], a["obs_every"], a["force_every"]) == want, (kw, a)
        assert a["dev_force"] == forces.data_ptr() and a["force_stride"] == forces.shape[2] and a["dev_cmd"] == cmd.data_ptr()
        with pytest.raises(AssertionError, match=r"\(rollout_force_device\)"):
            T.rollout(g, 10, cmd, 0.001, pos, out=on(torch.zeros(blocks, 10, 3, dtype=f64)), forces=forces, **kw)
    # without forces the function takes the paths it took: a stand-in without any force method is never asked for one
    RateSwarm = stand_in("rollout_device", "rollout_rate_device")
    with pytest.raises(AssertionError, match="rollout_rate_device"):
        T.rollout(RateSwarm(), 10, cmd, 0.001, pos, out=out, hold=2)
    with pytest.raises(AssertionError, match=r"\(rollout_device\)"):
        T.rollout(RateSwarm(), 10, cmd, 0.001, pos, out=out)


def test_apply_force_refuses_bad_tensors(monkeypatch):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64 = _Swarm(), torch.float64
    cases = [
        (torch.zeros(10, 3, dtype=f64), "is on cpu"),
        (on(torch.zeros(10, 3, dtype=f64), 1), "the swarm lives on cuda:0"),
        (on(torch.zeros(10, 3, dtype=torch.float16)), "float32 or torch.float64"),
        (on(torch.zeros(10, 2, dtype=f64)), r"\[10, >= 3\]"),
        (on(torch.zeros(5, 10, 3, dtype=f64)), r"rows must be a \[count, >= 3\]"),
        (on(torch.zeros(30, dtype=f64)), r"rows must be a \[count, >= 3\]"),
        (on(torch.zeros(3, 10, dtype=f64).transpose(0, 1)), "rows are not contiguous"),
        ([[0.0] * 3] * 10, r"rows must be a \[count, >= 3\]"),
    ]
    for rows, msg in cases:
        with pytest.raises(ValueError, match=msg):
            T.apply_force(g, rows)
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    for rows in (on(torch.zeros(10, 3, dtype=f64)), on(torch.zeros(10, 8)[:, :3])):  # (padded rows: the stride is the tensor's)
        with pytest.raises(AssertionError, match=r"\(apply_force_device\)"):
            T.apply_force(g, rows, first=7)


def test_every_rollout_force_kernel_has_a_row():
    """one force kernel per rate kernel, compiled by both step units behind the rate family and apart from the plain and the rate one"""
    k = rollout_kernels()
    k.check_family("_force", RF.ROLLOUT_FORCE_KERNELS, RF, mirrors="_rate")
    assert set(k.families["_rate"]) == set(RF.RR.ROLLOUT_RATE_KERNELS)
    assert not set(k.families["_force"]) & (set(k.families[""]) | set(k.families["_rate"]))


def test_rollout_force_test_compiles(mrs, tmp_path):
    from mrs_multirotor_simulator_amd import swarm
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DMRS_NO_EIGEN", "-D__HIP_PLATFORM_AMD__", "-I",
                           os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "rollout_force_test.cpp"),
                           "-o", str(tmp_path / "rollout_force_test"), "-L", os.path.dirname(swarm.LIB_PATH), "-lmrs_swarm", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-lpthread"])
