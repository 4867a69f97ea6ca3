"""CPU-side checks of control-rate rollouts (include/mrs_swarm.h, "control-rate rollouts"): mrs_swarm_rollout_rate_device is exported and
listed, its header prototype and ctypes argtypes agree, tensors.rollout refuses a bad hold, a bad observation rate and an `out` of the
undecimated size before the library is reached, everything test_rollout.test_rollout_refuses_bad_tensors refuses is still refused at
hold = 3, and tests/cpp/rollout_rate_test.cpp compiles.  CPU tensors only: no pointer reaches the library.

The rates have kernels of their own (the _rate family of helpers.rollout_kernels): every one of them has a row in
test_rollout_rate_gpu.ROLLOUT_RATE_KERNELS, and the five kernels of the plain family stay as test_rollout.py knows them.

The per-launch schedule (swarm_layout.h: mrs_ro_launch_sched, mrs_ro_due, mrs_ro_due_count) is checked against brute force by
tests/cpp/rollout_sched_test.cpp, on the host."""
import ctypes as C
import os
import subprocess

import pytest

import test_rollout_rate_gpu as RR
from helpers import CSRC, CTYPE, ROOT, abi_prototype, fake_cuda, rollout_kernels, stand_in

NAMES = ["s", "first", "count", "mode", "dt", "n_steps", "cmd_every", "obs_every", "dev_cmd", "dtype", "cmd_stride", "groups", "dev_obs",
         "obs_stride", "ext_stream"]


def test_symbol_is_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm
    assert hasattr(C.CDLL(swarm.LIB_PATH), "mrs_swarm_rollout_rate_device")
    assert "mrs_swarm_rollout_rate_device" in swarm.ABI_SYMBOLS
    assert callable(getattr(swarm.Swarm, "rollout_rate_device", None))


def test_header_prototype_equals_the_argtypes(mrs):
    from mrs_multirotor_simulator_amd import swarm
    names, types = abi_prototype("mrs_swarm_rollout_rate_device")
    assert names == NAMES
    got = swarm.load_library().mrs_swarm_rollout_rate_device.argtypes
    assert [CTYPE[t] for t in types] == list(got), (types, got)
    # the plain call keeps its prototype: the new one is it with the two rates behind n_steps
    plain = swarm.load_library().mrs_swarm_rollout_device.argtypes
    assert list(got[:6]) + list(got[8:]) == list(plain) and list(got[6:8]) == [C.c_int32, C.c_int32]


_Swarm = stand_in("rollout_device", "rollout_rate_device")  # neither rollout call of the library may be reached


def test_rollout_refuses_bad_rates(monkeypatch):
    """CPU tensors dressed as cuda tensors (only .device is faked; nothing is launched)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64, pos = _Swarm(), torch.float64, T.OBS_POS  # (mode 10: POSITION_CMD)
    cmd = on(torch.zeros(5, 10, 4, dtype=f64))  # B = 5

    def out(blocks):
        return on(torch.zeros(blocks, 10, 3, dtype=f64))

    cases = [
        (dict(hold=0), out(5), "hold must be at least 1"),
        (dict(hold=-2), out(5), "hold must be at least 1"),
        (dict(hold=2, obs_every=0), out(5), "obs_every must be at least 1 and divide"),
        (dict(hold=2, obs_every=-1), out(5), "obs_every must be at least 1 and divide"),
        (dict(obs_every=0), out(5), "obs_every must be at least 1 and divide"),
        (dict(hold=2, obs_every=3), out(3), "obs_every must be at least 1 and divide the 10 steps"),  # 3 does not divide 5 * 2
        (dict(hold=1, obs_every=2), out(2), "obs_every must be at least 1 and divide the 5 steps"),
        (dict(hold=4, obs_every=8), out(2), "obs_every must be at least 1 and divide the 20 steps"),
        (dict(hold=2, obs_every=5), out(10), r"\[2, 10, >= 3\]"),  # B * hold row blocks where B * hold // obs_every are due
        (dict(hold=2), out(10), r"\[5, 10, >= 3\]"),               # (obs_every defaults to hold)
        (dict(hold=3, obs_every=1), out(5), r"\[15, 10, >= 3\]"),  # B row blocks where B * hold are due
        (dict(hold=2, obs_every=10), out(2), r"\[1, 10, >= 3\]"),  # the terminal row block only
    ]
    for kw, o, msg in cases:
        with pytest.raises(ValueError, match=msg):
            T.rollout(g, 10, cmd, 0.001, pos, out=o, **kw)
    # groups == 0 has no `out`, but the rates are checked all the same
    with pytest.raises(ValueError, match="obs_every must be at least 1 and divide"):
        T.rollout(g, 10, cmd, 0.001, 0, hold=2, obs_every=4)
    # a well-formed call passes every check of the tensor layer: it is the stand-in's library call that raises (no GPU: no stream to ask for)
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    for kw, blocks, name in ((dict(hold=2, obs_every=5), 2, "rollout_rate_device"), (dict(hold=3), 5, "rollout_rate_device"),
                             (dict(obs_every=5), 1, "rollout_rate_device"), (dict(hold=1, obs_every=1), 5, r"\(rollout_device\)"),
                             (dict(), 5, r"\(rollout_device\)")):
        with pytest.raises(AssertionError, match=name):
            T.rollout(g, 10, cmd, 0.001, pos, out=out(blocks), **kw)


def test_rollout_refuses_bad_tensors_at_a_hold(monkeypatch):
    """the list of test_rollout.test_rollout_refuses_bad_tensors, at hold = 3 (obs_every = hold: `out` keeps its B row blocks)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64, pos = _Swarm(), torch.float64, T.OBS_POS
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
            T.rollout(g, 10, cmd, 0.001, pos, out=o, hold=3)
    with pytest.raises(ValueError, match="actuator rows must be dense"):
        T.rollout(g, T.ACTUATOR_CMD, on(torch.zeros(5, 10, 6, dtype=f64)[:, :, :4]), 0.001, pos, out=out, hold=3)
    with pytest.raises(ValueError, match="commands must be"):
        T.rollout(g, 10, [[[0.0] * 4] * 10] * 5, 0.001, pos, out=out, hold=3)


def test_every_rollout_rate_kernel_has_a_row():
    """one rate kernel per plain rollout kernel, compiled by both step units behind the plain family and apart from it"""
    k = rollout_kernels()
    k.check_family("_rate", RR.ROLLOUT_RATE_KERNELS, RR, mirrors="")
    assert set(k.families[""]) == set(RR.R.ROLLOUT_KERNELS) and not set(k.families[""]) & set(k.families["_rate"])


def test_schedule_division_is_exact():
    """RolloutRateDev's schedule: (x * M) >> 12 == x / P for every sub-step distance x < 64 and period P <= 64, with M as mrs_ro_sched
    (swarm_layout.h) computes it, and M - 1 fits its 12 bits"""
    src = open(os.path.join(CSRC, "swarm_layout.h")).read()
    assert "p == 1u ? 4096u : 4096u / p + 1u" in src and "(((w) >> 12) & 4095u) + 1u" in src
    for p in range(1, 65):
        m = 4096 if p == 1 else 4096 // p + 1
        assert m - 1 < 4096
        assert all((x * m) >> 12 == x // p for x in range(64)), p


def test_launch_schedule_against_brute_force(tmp_path):
    """tests/cpp/rollout_sched_test.cpp: every rate 1..70, launch start 0..448 and launch length 1..64, start and end schedules"""
    exe = str(tmp_path / "rollout_sched_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "rollout_sched_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "launches with due steps ok" in out.stdout, out.stdout + out.stderr
    # the hooks read the schedule through the text this program checked, not through a copy of it
    texts = rollout_kernels().texts
    assert all(" due(" not in t and "due_count(" not in t.replace("mrs_ro_due_count(", "") for t in texts.values())
    assert "mrs_ro_due(" in texts["rollout_device.inc"] and "mrs_ro_due_count(" in texts["rollout_rate_device.inc"]


def test_rollout_rate_test_compiles(mrs, tmp_path):
    from mrs_multirotor_simulator_amd import swarm
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DMRS_NO_EIGEN", "-D__HIP_PLATFORM_AMD__", "-I",
                           os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "rollout_rate_test.cpp"),
                           "-o", str(tmp_path / "rollout_rate_test"), "-L", os.path.dirname(swarm.LIB_PATH), "-lmrs_swarm", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-lpthread"])
