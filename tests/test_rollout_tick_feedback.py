"""CPU-side checks of feedback tick rollouts (include/mrs_swarm.h, "feedback tick rollouts"): mrs_swarm_rollout_tick_feedback_device is
exported and listed, its header prototype is the one specified and agrees with the ctypes argtypes and with
Swarm.rollout_tick_feedback_device, tensors.rollout_tick_feedback refuses bad tensors before the library is reached, and
tests/cpp/rollout_tick_feedback_test.cpp compiles.  CPU tensors only: no pointer reaches the library.

The call has kernels of its own: exactly four, each with a row in test_rollout_tick_feedback_gpu.ROLLOUT_TICK_FEEDBACK_KERNELS and the
shape of the single-GPU MRS_STEP_KERNEL_COLL line it mirrors; they belong to no rollout family, are no tick-rollout kernel and no
step-kernel line, and their tick family (_feedback) is defined behind rollout_cost_device.inc and in front of the cost tick family, so
the tables and positions of the earlier tests stay as they are."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import test_rollout_tick_feedback_gpu as RTF
from helpers import CSRC, CTYPE, ROOT, STEP_UNITS, abi_prototype, fake_cuda, macro_lines, rollout_kernels, stand_in

FILE = "rollout_tick_device.inc"  # the tick families share one file; this one is MRS_ROLLOUT_TICK_FAMILY(_feedback, ...)
NAMES = ["s", "first", "count", "mode", "dt", "n_ticks", "cmd_every", "cost_every", "dev_cmd", "dtype", "cmd_stride",
         "fb_groups", "dev_gain", "gain_per_uav", "gain_blocks", "dev_ref", "ref_stride", "ref_blocks",
         "cost_groups", "dev_target", "target_stride", "dev_weight", "weight_stride", "crash_cost", "dev_cost", "accumulate",
         "crash", "rebounce", "ext_stream"]

# the feedback tick kernel and the single-GPU *_coll kernel of step_device.inc it mirrors
MIRRORS = {
    "mrs_uav_rollout_tick_feedback_buf": "mrs_uav_step_coll_buf",
    "mrs_uav_model_rollout_tick_feedback_buf": "mrs_uav_model_step_coll_buf",
    "mrs_uav_rollout_tick_feedback": "mrs_uav_step_coll",
    "mrs_uav_rollout_tick_feedback_mixed": "mrs_uav_step_mixed_coll",
}


def test_symbol_is_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm, tensors
    assert hasattr(C.CDLL(swarm.LIB_PATH), "mrs_swarm_rollout_tick_feedback_device")
    assert "mrs_swarm_rollout_tick_feedback_device" in swarm.ABI_SYMBOLS
    assert callable(getattr(swarm.Swarm, "rollout_tick_feedback_device", None)) and callable(getattr(tensors, "rollout_tick_feedback", None))
    facade = open(os.path.join(ROOT, "include", "mrs_multirotor_simulator", "uav_system", "uav_system.hpp")).read()
    assert "void rolloutTickFeedbackDevice(" in facade


def test_header_prototype_argtypes_and_method_agree(mrs):
    from mrs_multirotor_simulator_amd import swarm, tensors
    text = open(os.path.join(ROOT, "include", "mrs_swarm.h")).read()
    names, types = abi_prototype("mrs_swarm_rollout_tick_feedback_device")
    assert names == NAMES
    ctype = dict(CTYPE, **{"double*": C.c_void_p})
    lib = swarm.load_library()
    got = list(lib.mrs_swarm_rollout_tick_feedback_device.argtypes)
    assert [ctype[t] for t in types] == got, (types, got)
    assert types[NAMES.index("dev_cost")] == "double*" and types[NAMES.index("crash_cost")] == "double"
    assert list(inspect.signature(swarm.Swarm.rollout_tick_feedback_device).parameters) == ["self"] + NAMES[1:]
    # the feedback rollout's prototype up to the weight stride, then the cost tick rollout's tail from the crash cost on
    fb, tc = list(lib.mrs_swarm_rollout_feedback_device.argtypes), list(lib.mrs_swarm_rollout_tick_cost_device.argtypes)
    assert got[:23] == fb[:23] and got[23:] == tc[16:]
    # the declaration comes behind the cost tick rollout's and cites the reference's tick and its collision pass
    block = text[text.index("feedback tick rollouts"):]
    assert text.index("int mrs_swarm_rollout_tick_cost_device(") < text.index("int mrs_swarm_rollout_tick_feedback_device(")
    assert "src/multirotor_simulator.cpp:211-217" in block and ":295-359" in block
    assert list(inspect.signature(tensors.rollout_tick_feedback).parameters) == [
        "swarm", "mode", "commands", "dt", "crash", "rebounce", "fb_groups", "gains", "refs", "cost_groups", "targets", "weights", "crash_cost",
        "first", "hold", "cost_every", "out", "accumulate"]


def test_every_kernel_has_a_row_and_the_shape_of_its_mirror():
    k = rollout_kernels()
    mine = k.tick_families["_feedback"]
    assert k.tick_types["_feedback"] == ("RolloutTickFeedbackDev", "RolloutTickFeedbackHook")
    assert len(mine) == 4 and set(mine) == set(MIRRORS), sorted(mine)
    k.check_table(mine, RTF.ROLLOUT_TICK_FEEDBACK_KERNELS, RTF, "feedback tick")
    coll = macro_lines(open(os.path.join(CSRC, "step_device.inc")).read(), "MRS_STEP_KERNEL_COLL")
    single = {n for n, v in coll.items() if v[-1] == "false"}
    assert single == set(MIRRORS.values()), sorted(single)
    for name, args in mine.items():
        assert args == coll[MIRRORS[name]][:-1], (name, args, coll[MIRRORS[name]])
    # and of the tick kernel and the cost tick kernel beside it
    assert {n.replace("_tick_feedback", "_tick"): v for n, v in mine.items()} == k.tick
    cost = k.tick_families["_cost"]
    assert {n.replace("_tick_feedback", "_tick_cost"): v for n, v in mine.items()} == cost
    # compiled by both step units, behind LaneObs and the feedback arithmetic's family, in front of the cost tick family and the tick family
    assert k.files.index("rollout_cost_device.inc") + 1 == k.files.index(FILE) == len(k.files) - 1
    assert list(k.tick_families) == ["_feedback", "_cost", ""] and k.order[-12:] == list(mine) + list(cost) + list(k.tick)
    # none of them is a kernel the earlier tables know
    assert not set(mine) & ({n for fam in k.families.values() for n in fam} | set(k.tick)) and not set(mine) & set(k.step_kernels) and not set(mine) & set(cost)
    for unit in STEP_UNITS:
        assert open(os.path.join(CSRC, unit)).read().count(f'#include "{FILE}"') == 1, unit
    build = open(os.path.join(os.path.dirname(CSRC), "build.py")).read()
    assert f'"{FILE}"' in build, "the source list that keys the build"


def test_no_other_kernel_lines_in_the_file():
    """no family, shape, tick-kernel, cost-tick-kernel or step-kernel line, and no schedule words: one launch is one tick"""
    k = rollout_kernels()
    text = k.texts[FILE]
    assert "MRS_STEP_KERNEL" not in text
    for macro in ("MRS_ROLLOUT_FAMILY", "MRS_ROLLOUT_SHAPE"):
        assert not re.search(rf"^\s*(#define\s+)?{macro}\(", text, flags=re.M), macro
        assert not macro_lines(text, macro), macro
    # one family line of its own, and the four shape lines of the family macro are every kernel line of the file
    assert len(re.findall(r"^MRS_ROLLOUT_TICK_FAMILY\(_feedback, ", text, flags=re.M)) == 1
    assert len(macro_lines(text, "MRS_ROLLOUT_TICK_SHAPE")) == 4 and text.count("MRS_ROLLOUT_TICK_SHAPE(") == 5
    assert "mrs_ro_sched" not in text and "MRS_RO_" not in text and "mrs_ro_" not in text, "no schedule words"
    assert text.count("__global__") == 1, "the shape macro is the only kernel definition"
    # the descriptor is a kernel argument behind CollDev, whose offset is pinned for every family; the header states the replay argument
    # and why the command may be formed ahead of the collision evaluation
    family = text[text.index("#define MRS_ROLLOUT_TICK_FAMILY("):text.index("MRS_ROLLOUT_TICK_FAMILY(_feedback")]
    assert "static_assert(offsetof(RolloutTickKernArgs<DevType>, cd) == offsetof(CollKernArgs, cd)" in family
    head = text.split("namespace {")[0]
    assert "no-op launch" in head and "MRS_COLLIDE_EVAL" in head and "F_FEXT" in head
    assert "mrs_obs_row_feedback(" in text and "mrs_obs_row_cost(" in text
    layout = open(os.path.join(CSRC, "swarm_layout.h")).read()
    body = layout[layout.index("struct RolloutTickFeedbackDev {"):]
    body = body[:body.index("};")]
    assert "sched" not in body and "_blk" not in body and "crash_cost" in body and "gain_col" in body
    # step_device.inc admits the hook on the tick shape by the trait its base declares, and names none of the tick hook types
    step = open(os.path.join(CSRC, "step_device.inc")).read()
    assert "RolloutTick" not in step
    assert "(HK::kOnCollKernels && NU == 1 && !MULTI && COLL && !SHARD)" in step
    base = text[text.index("struct RolloutTickHookBase {"):text.index("struct RolloutTickHook :")]
    assert "static constexpr bool kOnCollKernels = true;" in base
    assert "struct RolloutTickFeedbackHook : RolloutTickEvalHook<RolloutTickFeedbackDev>" in text
    assert "struct RolloutTickEvalHook : RolloutTickHookBase<Dev>" in text
    for other in ("step_device.inc", "rollout_device.inc"):  # every other hook says it does not: NoStepHook and the sub-step hooks' base
        assert open(os.path.join(CSRC, other)).read().count("static constexpr bool kOnCollKernels = false;") == 1, other


_Swarm = stand_in("rollout_feedback_device", "rollout_tick_cost_device", "rollout_tick_feedback_device")


def test_rollout_tick_feedback_refuses_bad_tensors(monkeypatch):
    """CPU tensors dressed as cuda tensors (only .device is faked; nothing is launched): the checks of rollout_feedback and of
    rollout_tick_cost"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64, f32 = _Swarm(), torch.float64, torch.float32
    fb, pos = T.OBS_POS | T.OBS_OMEGA, T.OBS_POS  # W_o = 6; cost columns: 3; mode 10 (POSITION_CMD): W_c = 4

    def z(*shape, dtype=f64, dev=0):
        return on(torch.zeros(*shape, dtype=dtype), dev)

    cmd, tg, wt, out = z(6, 10, 4), z(3, 10, 3), z(3, 3), z(10)  # B = 6, hold = 2: 12 ticks, cost_every = 4: E = 3
    ok = dict(mode=10, commands=cmd, fb_groups=fb, gains=z(6, 4, 6, 10), refs=z(6, 10, 6), cost_groups=pos, targets=tg, weights=wt, out=out, hold=2,
              cost_every=4)
    cases = [
        # CPU tensors and other devices
        (dict(commands=torch.zeros(6, 10, 4, dtype=f64)), "is on cpu"),
        (dict(gains=torch.zeros(6, 4, 6, 10, dtype=f64)), "gains is on cpu"),
        (dict(refs=torch.zeros(6, 10, 6, dtype=f64)), "is on cpu"),
        (dict(targets=torch.zeros(3, 10, 3, dtype=f64)), "is on cpu"),
        (dict(weights=torch.zeros(3, 3, dtype=f64)), "is on cpu"),
        (dict(out=torch.zeros(10, dtype=f64)), "is on cpu"),
        (dict(commands=z(6, 10, 4, dev=1)), "the swarm lives on cuda:0"),
        (dict(gains=z(6, 4, 6, 10, dev=1)), "the swarm lives on cuda:0"),
        (dict(refs=z(6, 10, 6, dev=1)), "the swarm lives on cuda:0"),
        (dict(targets=z(3, 10, 3, dev=1)), "the swarm lives on cuda:0"),
        (dict(out=z(10, dev=1)), "the swarm lives on cuda:0"),
        # dtypes
        (dict(commands=z(6, 10, 4, dtype=torch.float16)), "float32 or torch.float64"),
        (dict(gains=z(6, 4, 6, 10, dtype=f32)), "gains has dtype torch.float32, the commands torch.float64"),
        (dict(refs=z(6, 10, 6, dtype=f32)), "refs has dtype torch.float32, the commands torch.float64"),
        (dict(targets=z(3, 10, 3, dtype=f32)), "targets has dtype torch.float32, the commands torch.float64"),
        (dict(weights=z(3, 3, dtype=f32)), "weights has dtype torch.float32, the commands torch.float64"),
        (dict(commands=z(6, 10, 4, dtype=f32)), "gains has dtype torch.float64, the commands torch.float32"),
        (dict(out=z(10, dtype=f32)), "the cost vector is always torch.float64"),
        # commands
        (dict(commands=z(10, 4)), r"\[T, count, width\]"),
        (dict(commands=z(6, 10, 3)), r">= 4\] tensor"),
        (dict(commands=[[[0.0] * 4] * 10] * 6), "commands must be"),
        # a wrong Bg, wrong shapes, non-dense gains
        (dict(gains=z(3, 4, 6, 10)), r"gains: expected a \[6 or 1, 4, 6, 10\]"),
        (dict(gains=z(2, 4, 6)), r"gains: expected a \[6 or 1, 4, 6\]"),
        (dict(gains=z(6, 10, 4, 6)), r"gains: expected a \[6 or 1, 4, 6, 10\]"),  # (a matrix per UAV row: not UAV-minor)
        (dict(gains=z(6, 6, 4)), r"gains: expected a \[6 or 1, 4, 6\]"),
        (dict(gains=z(4, 6)), "gains: expected a"),
        (dict(gains=None), "gains: expected a"),
        (dict(gains=z(6, 10, 4, 6).permute(0, 2, 3, 1)), "gains must be dense"),
        (dict(gains=z(6, 4, 6, 20)[..., ::2]), "gains must be dense"),
        (dict(gains=z(6, 4, 8)[:, :, :6]), "gains must be dense"),
        (dict(refs=z(3, 10, 6)), r"refs: expected a \[6 or 1, 10 or 1, >= 6\]"),
        (dict(refs=z(6, 10, 5)), r"refs: expected a \[6, 10 or 1, >= 6\]"),
        (dict(refs=z(6, 5, 6)), r"refs: expected a \[6, 10 or 1, >= 6\]"),
        (dict(refs=None), r"refs: expected a \[6 or 1, 10 or 1, >= 6\]"),
        (dict(refs=z(6, 1, 8)[:, :, :6]), "shared rows must be dense"),
        # W_o = 0, a payload-less mode, the rates
        (dict(fb_groups=0), "fb_groups must select at least one observation group"),
        (dict(mode=T.INPUT_UNKNOWN), "needs a mode with a payload"),
        (dict(hold=0), "hold must be at least 1"),
        (dict(cost_every=0), "cost_every must be at least 1 and divide the 12 ticks"),
        (dict(cost_every=5), "cost_every must be at least 1 and divide the 12 ticks"),
        (dict(cost_every=24), "cost_every must be at least 1 and divide the 12 ticks"),
        (dict(hold=3, cost_every=None), r"\[6, 10 or 1, >= 3\]"),  # cost_every defaults to hold: 18 ticks, E = 6
        # the cost side
        (dict(targets=z(4, 10, 3)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(3, 10, 2)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=None), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(3, 1, 5)[:, :, :3]), "shared rows must be dense"),
        (dict(targets=z(3, 3, 10).transpose(1, 2)), "rows are not contiguous"),
        (dict(weights=z(2, 3)), r"weights: expected a \[3 or 1, >= 3\]"),
        (dict(weights=None), r"weights: expected a \[3 or 1, >= 3\]"),
        (dict(weights=z(3, 2)), r">= 3\] matrix"),
        (dict(out=z(9)), "vector of 10 elements"),
        (dict(out=z(20)[::2]), "not contiguous"),
        (dict(out=None, accumulate=True), "accumulate=True needs the `out` vector"),
        # cost_groups == 0 with tensors
        (dict(cost_groups=0), "cost_groups == 0 is the crash cost alone"),
        (dict(cost_groups=0, targets=None), "cost_groups == 0 is the crash cost alone"),
        (dict(cost_groups=0, weights=None), "cost_groups == 0 is the crash cost alone"),
        (dict(cost_groups=0, targets=None, weights=None, out=None, accumulate=True), "accumulate=True needs the `out` vector"),
        (dict(cost_groups=0, targets=None, weights=None, out=z(9)), "vector of 10 elements"),
    ]

    def call(a):
        a = dict(a)
        return T.rollout_tick_feedback(g, a.pop("mode"), a.pop("commands"), 0.001, True, 100.0, a.pop("fb_groups"), a.pop("gains"), a.pop("refs"), **a)

    for change, msg in cases:
        with pytest.raises(ValueError, match=msg):
            call(dict(ok, **change))
    with pytest.raises(ValueError, match="actuator rows must be dense"):
        call(dict(ok, mode=T.ACTUATOR_CMD, commands=z(6, 10, 6)[:, :, :4]))
    # well-formed calls pass every check of the tensor layer and reach rollout_tick_feedback_device and nothing else
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    for change in (dict(), dict(gains=z(1, 4, 6), refs=z(1, 1, 6)), dict(gains=z(1, 4, 6, 10), refs=z(6, 1, 6)), dict(gains=z(6, 4, 6), refs=z(1, 10, 9)[:, :, :6]),
                   dict(cost_groups=0, targets=None, weights=None, out=None), dict(cost_groups=0, targets=None, weights=None),
                   dict(targets=z(3, 1, 3), weights=z(1, 3), out=z(30)[5:15], accumulate=True)):
        with pytest.raises(AssertionError, match=r"\(rollout_tick_feedback_device\)"):
            call(dict(ok, **change))


def test_arguments_handed_to_the_library(monkeypatch):
    """per-UAV gains travel as gain_per_uav 1, shared rows as stride 0, one block as 1; the crash-only form has null target and weight
    pointers and the pure closed-loop run a null cost pointer too, and returns None"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    seen = []

    class Rec(_Swarm):
        def rollout_tick_feedback_device(self, *a):
            seen.append(a)

    def z(*shape):
        return on(torch.zeros(*shape, dtype=torch.float64))

    cmd, fb = z(6, 10, 4), T.OBS_POS | T.OBS_OMEGA
    out = z(10)
    assert T.rollout_tick_feedback(Rec(), 10, cmd, 0.001, True, 50.0, fb, z(6, 4, 6, 10), z(6, 10, 9)[:, :, :6], T.OBS_POS, z(3, 10, 7)[:, :, :3],
                                   z(3, 8)[:, :3], 2.5, hold=2, cost_every=4, first=5, out=out) is out
    assert T.rollout_tick_feedback(Rec(), 10, cmd, 0.001, False, 50.0, fb, z(1, 4, 6), z(1, 1, 6), hold=2) is None
    assert T.rollout_tick_feedback(Rec(), 10, cmd, 0.001, True, 50.0, fb, z(1, 4, 6), z(6, 1, 6), 0, None, None, 7.0, out=out, accumulate=True) is out
    assert all(len(s) == len(NAMES) - 1 for s in seen)
    a, b, c = (dict(zip(NAMES[1:], s)) for s in seen)
    assert (a["first"], a["count"], a["n_ticks"], a["cmd_every"], a["cost_every"]) == (5, 10, 12, 2, 4)
    assert (a["gain_per_uav"], a["gain_blocks"], a["ref_stride"], a["ref_blocks"], a["fb_groups"]) == (1, 6, 9, 6, fb)
    assert (a["cost_groups"], a["target_stride"], a["weight_stride"], a["accumulate"], a["crash_cost"], a["crash"], a["rebounce"]) == (T.OBS_POS, 7, 8, False, 2.5, True, 50.0)
    assert a["dev_cost"] == out.data_ptr()
    assert (b["gain_per_uav"], b["gain_blocks"], b["ref_stride"], b["ref_blocks"], b["cost_every"], b["crash"]) == (0, 1, 0, 1, 2, False)
    assert (b["cost_groups"], b["dev_target"], b["dev_weight"], b["dev_cost"], b["crash_cost"]) == (0, 0, 0, 0, 0.0)
    assert (c["cost_groups"], c["dev_target"], c["dev_weight"], c["dev_cost"], c["crash_cost"], c["accumulate"]) == (0, 0, 0, out.data_ptr(), 7.0, True)
    assert (c["ref_stride"], c["ref_blocks"], c["n_ticks"], c["cost_every"]) == (0, 6, 6, 1)


def test_rollout_tick_feedback_test_compiles(mrs, tmp_path):
    from mrs_multirotor_simulator_amd import swarm
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DMRS_NO_EIGEN", "-D__HIP_PLATFORM_AMD__", "-I",
                           os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "rollout_tick_feedback_test.cpp"),
                           "-o", str(tmp_path / "rollout_tick_feedback_test"), "-L", os.path.dirname(swarm.LIB_PATH), "-lmrs_swarm", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-lpthread"])
