"""CPU-side checks of tick rollouts (include/mrs_swarm.h, "tick rollouts"): mrs_swarm_rollout_tick_device is exported and listed, its
header prototype is the one specified and agrees with the ctypes argtypes, tensors.rollout_ticks refuses CPU tensors, wrong dtypes,
crash rows that are not dense and wrong block counts before the library is reached, and tests/cpp/rollout_tick_test.cpp compiles.  CPU
tensors only: no pointer reaches the library.

The call has kernels of its own (the tick kernels of helpers.rollout_kernels): exactly four, each with a row in
test_rollout_tick_gpu.ROLLOUT_TICK_KERNELS and the shape of the single-GPU MRS_STEP_KERNEL_COLL line it mirrors; they belong to no
rollout family and are no step-kernel line, so the tables of the earlier tests stay as they are."""
import ctypes as C
import os
import re
import subprocess

import pytest

import test_rollout_tick_gpu as RT
from helpers import CSRC, CTYPE, ROOT, abi_prototype, fake_cuda, macro_lines, rollout_kernels, stand_in

NAMES = ["s", "first", "count", "mode", "dt", "n_ticks", "cmd_every", "obs_every", "dev_cmd", "dtype", "cmd_stride", "groups", "dev_obs",
         "obs_stride", "dev_crashed", "crash", "rebounce", "ext_stream"]
TYPES = dict(CTYPE, **{"uint8_t*": C.c_void_p})

# the tick kernel and the single-GPU *_coll kernel of step_device.inc it mirrors
MIRRORS = {
    "mrs_uav_rollout_tick_buf": "mrs_uav_step_coll_buf",
    "mrs_uav_model_rollout_tick_buf": "mrs_uav_model_step_coll_buf",
    "mrs_uav_rollout_tick": "mrs_uav_step_coll",
    "mrs_uav_rollout_tick_mixed": "mrs_uav_step_mixed_coll",
}


def test_symbol_is_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm, tensors
    assert hasattr(C.CDLL(swarm.LIB_PATH), "mrs_swarm_rollout_tick_device")
    assert "mrs_swarm_rollout_tick_device" in swarm.ABI_SYMBOLS
    assert callable(getattr(swarm.Swarm, "rollout_tick_device", None)) and callable(getattr(tensors, "rollout_ticks", None))


def test_header_prototype_equals_the_argtypes(mrs):
    from mrs_multirotor_simulator_amd import swarm
    names, types = abi_prototype("mrs_swarm_rollout_tick_device")
    assert names == NAMES
    got = swarm.load_library().mrs_swarm_rollout_tick_device.argtypes
    assert [TYPES[t] for t in types] == list(got), (types, got)
    # the control-rate call with the crash rows and the collision arguments between obs_stride and the stream
    rate = swarm.load_library().mrs_swarm_rollout_rate_device.argtypes
    assert list(got[:14]) + [got[-1]] == list(rate) and list(got[14:17]) == [C.c_void_p, C.c_int32, C.c_double]
    assert "src/multirotor_simulator.cpp:211-217" in open(os.path.join(ROOT, "include", "mrs_swarm.h")).read()


def test_every_rollout_tick_kernel_has_a_row_and_the_shape_of_its_mirror():
    k = rollout_kernels()
    assert len(k.tick) == 4, sorted(k.tick)
    k.check_table(k.tick, RT.ROLLOUT_TICK_KERNELS, RT, "tick")
    # (bounds, CASCADE, UNIFORM, ACC, SU) of the mirrored line, which is a single-GPU one (SHARD == false)
    coll = macro_lines(open(os.path.join(CSRC, "step_device.inc")).read(), "MRS_STEP_KERNEL_COLL")
    single = {n for n, v in coll.items() if v[-1] == "false"}
    assert single == set(MIRRORS.values()), sorted(single)
    assert set(k.tick) == set(MIRRORS)
    for name, args in k.tick.items():
        assert args == coll[MIRRORS[name]][:-1], (name, args, coll[MIRRORS[name]])
    # both step units compile the tick kernels last (rollout_kernels checks that the two include lists are one)
    assert k.files[-1] == "rollout_tick_device.inc" and k.order[-4:] == list(k.tick)


def test_no_other_kernel_lines_in_the_file():
    """the tick kernels are the only kernels of their file: no family, no shape and no step-kernel line, and no schedule words"""
    k = rollout_kernels()
    text = k.texts["rollout_tick_device.inc"]
    assert "MRS_STEP_KERNEL" not in text
    for macro in ("MRS_ROLLOUT_FAMILY", "MRS_ROLLOUT_SHAPE"):
        assert not re.search(rf"^\s*(#define\s+)?{macro}\(", text, flags=re.M), macro
    assert not set(k.tick) & {n for fam in k.families.values() for n in fam}
    assert "mrs_ro_sched" not in text and "MRS_RO_" not in text and "mrs_ro_" not in text, "one launch is one tick: no schedule words"


_Swarm = stand_in("rollout_tick_device")


def test_rollout_ticks_refuses_bad_tensors(monkeypatch):
    """CPU tensors dressed as cuda tensors (only .device is faked; nothing is launched)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64, pos = _Swarm(), torch.float64, T.OBS_POS  # (mode 10: POSITION_CMD)

    def cmd(**kw):
        return on(torch.zeros(6, 10, 4, dtype=kw.get("dtype", f64)), kw.get("index", 0))  # B = 6

    def out(blocks=6, width=3):
        return on(torch.zeros(blocks, 10, width, dtype=f64))

    def cr(blocks=6, rows=10, dtype=torch.bool):
        return on(torch.zeros(blocks, rows, dtype=dtype))

    cases = [
        (torch.zeros(6, 10, 4, dtype=f64), dict(out=out(), crashed=cr()), "is on cpu"),                    # CPU commands
        (cmd(index=1), dict(out=out(), crashed=cr()), "the swarm lives on cuda:0"),                        # another device
        (cmd(dtype=torch.float16), dict(out=out(), crashed=cr()), "float32 or torch.float64"),             # dtype
        (cmd(dtype=torch.float32), dict(out=out(), crashed=cr()), "one dtype serves both"),                # mismatched dtypes
        (on(torch.zeros(6, 10, 3, dtype=f64)), dict(out=out(), crashed=cr()), r">= 4\] tensor"),           # too narrow
        (on(torch.zeros(10, 4, dtype=f64)), dict(out=out(), crashed=cr()), r"\[T, count, width\]"),         # no tick dimension
        (cmd(), dict(out=torch.zeros(6, 10, 3, dtype=f64), crashed=cr()), "is on cpu"),                    # out on the CPU
        (cmd(), dict(out=out(5), crashed=cr()), r"\[6, 10, >= 3\]"),                                       # out of another block count
        (cmd(), dict(out=out(6, 2), crashed=cr()), r">= 3\]"),                                             # out too narrow
        (cmd(), dict(out=out(), crashed=torch.zeros(6, 10, dtype=torch.bool)), "crashed is on cpu"),       # crash rows on the CPU
        (cmd(), dict(out=out(), crashed=on(torch.zeros(6, 10, dtype=torch.bool), 1)), "crashed is on cuda:1"),
        (cmd(), dict(out=out(), crashed=cr(dtype=torch.int32)), "torch.bool or torch.uint8"),              # crash dtype
        (cmd(), dict(out=out(), crashed=cr(dtype=torch.float32)), "torch.bool or torch.uint8"),
        (cmd(), dict(out=out(), crashed=cr(5)), r"crashed: expected a \[6, 10\]"),                         # wrong block count
        (cmd(), dict(out=out(), crashed=cr(6, 11)), r"crashed: expected a \[6, 10\]"),                     # wrong row count
        (cmd(), dict(out=out(), crashed=on(torch.zeros(60, dtype=torch.bool))), r"crashed: expected a \[6, 10\]"),
        (cmd(), dict(out=out(), crashed=on(torch.zeros(6, 20, dtype=torch.bool)[:, ::2])), "not dense"),   # strided bytes
        (cmd(), dict(out=out(), crashed=on(torch.zeros(6, 12, dtype=torch.bool)[:, :10])), "not dense"),   # padded blocks
        (cmd(), dict(out=out(), crashed=on(torch.zeros(10, 6, dtype=torch.uint8).t())), "not dense"),      # transposed
        (cmd(), dict(out=out(), crashed=[[0] * 10] * 6), "crashed: expected a torch.Tensor"),
        (cmd(), dict(out=out(3), crashed=cr(6), hold=2, obs_every=4), r"crashed: expected a \[3, 10\]"),   # the decimated block count
        (cmd(), dict(out=out(12), crashed=cr(3), hold=2, obs_every=4), r"\[3, 10, >= 3\]"),
        (cmd(), dict(out=out(), crashed=cr(), hold=0), "hold must be at least 1"),
        (cmd(), dict(out=out(), crashed=cr(), hold=2, obs_every=0), "obs_every must be at least 1 and divide"),
        (cmd(), dict(out=out(), crashed=cr(), hold=2, obs_every=5), "obs_every must be at least 1 and divide the 12 ticks"),
    ]
    for c, kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            T.rollout_ticks(g, 10, c, 0.001, True, 100.0, pos, **kw)
    with pytest.raises(ValueError, match="actuator rows must be dense"):
        T.rollout_ticks(g, T.ACTUATOR_CMD, on(torch.zeros(6, 10, 6, dtype=f64)[:, :, :4]), 0.001, True, 100.0, pos, out=out(), crashed=cr())
    with pytest.raises(ValueError, match="commands must be"):
        T.rollout_ticks(g, 10, [[[0.0] * 4] * 10] * 6, 0.001, True, 100.0, pos, out=out(), crashed=cr())
    # a well-formed call passes every check of the tensor layer: it is the stand-in's library call that raises (no GPU: no stream to
    # ask for), with bool or uint8 crash rows, without crash rows and without observation rows
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    for kw in (dict(out=out(), crashed=cr()), dict(out=out(), crashed=cr(dtype=torch.uint8)), dict(out=out(), crashed=False),
               dict(out=out(3), crashed=cr(3), hold=2, obs_every=4), dict(out=out(1), crashed=cr(1), obs_every=6)):
        with pytest.raises(AssertionError, match="rollout_tick_device"):
            T.rollout_ticks(g, 10, cmd(), 0.001, True, 100.0, pos, **kw)
    with pytest.raises(AssertionError, match="rollout_tick_device"):
        T.rollout_ticks(g, 10, cmd(), 0.001, False, 100.0, 0, crashed=cr())


def test_block_helpers_against_their_statement(tmp_path):
    """tests/cpp/rollout_tick_blocks_test.cpp: every rate 1..12 and every n_ticks up to 48 that the rate divides, the blocks that start at
    and end with each tick (swarm_layout.h: mrs_tick_block_start, mrs_tick_block_end); the entry points use this text, not a copy"""
    exe = str(tmp_path / "rollout_tick_blocks_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "rollout_tick_blocks_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    n = sum(48 // every for every in range(1, 13))
    assert out.returncode == 0 and f"{n} schedules ok" in out.stdout, out.stdout + out.stderr
    io = open(os.path.join(CSRC, "device_io.hip")).read()
    assert "mrs_tick_block_start(t, a.cmd_every" in io and "mrs_tick_block_end(t, a.obs_every" in io
    assert "% cmd_every" not in io.replace("a.n_steps % a.cmd_every", "") and "% obs_every" not in io.replace("a.n_steps % a.obs_every", "")


def test_rollout_tick_test_compiles(mrs, tmp_path):
    from mrs_multirotor_simulator_amd import swarm
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DMRS_NO_EIGEN", "-D__HIP_PLATFORM_AMD__", "-I",
                           os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "rollout_tick_test.cpp"),
                           "-o", str(tmp_path / "rollout_tick_test"), "-L", os.path.dirname(swarm.LIB_PATH), "-lmrs_swarm", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-lpthread"])
