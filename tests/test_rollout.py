"""CPU-side checks of device-resident rollouts (include/mrs_swarm.h, "device-resident rollouts"): the call is exported and listed, the
header prototype and the ctypes argtypes agree, tensors.rollout refuses what the library must never see, every kernel of the plain
rollout family (helpers.rollout_kernels) has a row in test_rollout_gpu.ROLLOUT_KERNELS, and tests/cpp/rollout_test.cpp compiles.  CPU tensors only: no
pointer reaches the library."""
import ctypes as C
import os

import pytest

import test_rollout_gpu as R
from helpers import CTYPE, ROOT, abi_prototype, fake_cuda, rollout_kernels, stand_in


def test_symbol_is_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm
    assert hasattr(C.CDLL(swarm.LIB_PATH), "mrs_swarm_rollout_device")
    assert "mrs_swarm_rollout_device" in swarm.ABI_SYMBOLS


def test_header_prototype_equals_the_argtypes(mrs):
    from mrs_multirotor_simulator_amd import swarm
    names, types = abi_prototype("mrs_swarm_rollout_device")
    assert names == ["s", "first", "count", "mode", "dt", "n_steps", "dev_cmd", "dtype", "cmd_stride", "groups", "dev_obs",
                     "obs_stride", "ext_stream"]
    got = swarm.load_library().mrs_swarm_rollout_device.argtypes
    assert [CTYPE[t] for t in types] == list(got), (types, got)


_Swarm = stand_in("rollout_device")


def test_rollout_refuses_bad_tensors(monkeypatch):
    """CPU tensors dressed as cuda tensors (only .device is faked; nothing is launched)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64, pos = _Swarm(), torch.float64, T.OBS_POS  # (mode 10: POSITION_CMD)
    out = on(torch.zeros(5, 10, 3, dtype=f64))
    cases = [
        (torch.zeros(5, 10, 4, dtype=f64), out, "is on cpu"),                                   # CPU tensor
        (on(torch.zeros(5, 10, 4, dtype=f64), 1), out, "the swarm lives on cuda:0"),           # another device
        (on(torch.zeros(5, 10, 4, dtype=torch.float16)), out, "float32 or torch.float64"),     # dtype
        (on(torch.zeros(5, 10, 4)), out, "one dtype serves both"),                              # mismatched dtypes
        (on(torch.zeros(5, 10, 3, dtype=f64)), out, r">= 4\] tensor"),                         # too narrow
        (on(torch.zeros(10, 4, dtype=f64)), out, r"\[T, count, width\]"),                       # no step dimension
        (on(torch.zeros(5, 10, 4, dtype=f64)), on(torch.zeros(4, 10, 3, dtype=f64)), r"\[5, 10, >= 3\]"),  # out of other T
        (on(torch.zeros(5, 10, 4, dtype=f64)), on(torch.zeros(5, 10, 2, dtype=f64)), r">= 3\]"),  # out too narrow
        (on(torch.zeros(10, 5, 4, dtype=f64).transpose(0, 1)), out, "step dimension is not dense"),
        (on(torch.zeros(5, 10, 8, dtype=f64)[::2, :, :4]), out, "step dimension is not dense"),
        (on(torch.zeros(5, 4, 10, dtype=f64).transpose(1, 2)), out, "rows are not contiguous"),
        (on(torch.zeros(5, 10, 4, dtype=f64)), on(torch.zeros(5, 3, 10, dtype=f64).transpose(1, 2)), "rows are not contiguous"),
        (on(torch.zeros(5, 10, 4, dtype=f64)), torch.zeros(5, 10, 3, dtype=f64), "is on cpu"),  # out on the CPU
    ]
    for cmd, o, msg in cases:
        with pytest.raises(ValueError, match=msg):
            T.rollout(g, 10, cmd, 0.001, pos, out=o)
    with pytest.raises(ValueError, match="actuator rows must be dense"):
        T.rollout(g, T.ACTUATOR_CMD, on(torch.zeros(5, 10, 6, dtype=f64)[:, :, :4]), 0.001, pos, out=out)
    with pytest.raises(ValueError, match="commands must be"):
        T.rollout(g, 10, [[[0.0] * 4] * 10] * 5, 0.001, pos, out=out)


def test_every_rollout_kernel_has_a_row():
    """the first family: five kernels, a row each, and none of them a step-kernel line (test_step_variants_gpu's matrix stays as it is)"""
    rollout_kernels().check_family("", R.ROLLOUT_KERNELS, R)


def test_rollout_test_compiles(mrs, tmp_path):
    import subprocess
    from mrs_multirotor_simulator_amd import swarm
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DMRS_NO_EIGEN", "-D__HIP_PLATFORM_AMD__", "-I",
                           os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "rollout_test.cpp"),
                           "-o", str(tmp_path / "rollout_test"), "-L", os.path.dirname(swarm.LIB_PATH), "-lmrs_swarm", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-lpthread"])
