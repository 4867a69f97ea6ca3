"""CPU-side checks of cost tick rollouts (include/mrs_swarm.h, "cost tick rollouts"): mrs_swarm_rollout_tick_cost_device is exported and
listed, its header prototype is the one specified and agrees with the ctypes argtypes and with Swarm.rollout_tick_cost_device,
tensors.rollout_tick_cost refuses bad tensors before the library is reached, test_rollout_tick_cost_gpu.restate_ticks is the stated loop,
and tests/cpp/rollout_tick_cost_test.cpp compiles.  CPU tensors only: no pointer reaches the library.

The call has kernels of its own: exactly four, each with a row in test_rollout_tick_cost_gpu.ROLLOUT_TICK_COST_KERNELS and the shape of
the single-GPU MRS_STEP_KERNEL_COLL line it mirrors; they belong to no rollout family, are no tick-rollout kernel and no step-kernel line,
and their tick family (_cost) is defined in front of the tick rollout's own, so the tables of the earlier tests stay as they are."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import test_rollout_tick_cost_gpu as RTC
from helpers import CSRC, CTYPE, ROOT, STEP_UNITS, abi_prototype, fake_cuda, macro_lines, rollout_kernels, stand_in

FILE = "rollout_tick_device.inc"  # the tick families share one file; this one is MRS_ROLLOUT_TICK_FAMILY(_cost, ...)
NAMES = ["s", "first", "count", "mode", "dt", "n_ticks", "cmd_every", "cost_every", "dev_cmd", "dtype", "cmd_stride", "groups", "dev_target",
         "target_stride", "dev_weight", "weight_stride", "crash_cost", "dev_cost", "accumulate", "crash", "rebounce", "ext_stream"]

# the cost tick kernel and the single-GPU *_coll kernel of step_device.inc it mirrors
MIRRORS = {
    "mrs_uav_rollout_tick_cost_buf": "mrs_uav_step_coll_buf",
    "mrs_uav_model_rollout_tick_cost_buf": "mrs_uav_model_step_coll_buf",
    "mrs_uav_rollout_tick_cost": "mrs_uav_step_coll",
    "mrs_uav_rollout_tick_cost_mixed": "mrs_uav_step_mixed_coll",
}


def test_symbol_is_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm, tensors
    assert hasattr(C.CDLL(swarm.LIB_PATH), "mrs_swarm_rollout_tick_cost_device")
    assert "mrs_swarm_rollout_tick_cost_device" in swarm.ABI_SYMBOLS
    assert callable(getattr(swarm.Swarm, "rollout_tick_cost_device", None)) and callable(getattr(tensors, "rollout_tick_cost", None))


def test_header_prototype_argtypes_and_method_agree(mrs):
    from mrs_multirotor_simulator_amd import swarm
    text = open(os.path.join(ROOT, "include", "mrs_swarm.h")).read()
    names, types = abi_prototype("mrs_swarm_rollout_tick_cost_device")
    assert names == NAMES
    ctype = dict(CTYPE, **{"double*": C.c_void_p})
    got = swarm.load_library().mrs_swarm_rollout_tick_cost_device.argtypes
    assert [ctype[t] for t in types] == list(got), (types, got)
    assert types[NAMES.index("dev_cost")] == "double*" and types[NAMES.index("crash_cost")] == "double"
    assert list(inspect.signature(swarm.Swarm.rollout_tick_cost_device).parameters) == ["self"] + NAMES[1:]
    # the cost rollout's prototype with the crash cost in front of dev_cost and the collision arguments in front of the stream
    cost = list(swarm.load_library().mrs_swarm_rollout_cost_device.argtypes)
    assert list(got[:16]) == cost[:16] and list(got[17:19]) == cost[16:18] and list(got[19:21]) == [C.c_int32, C.c_double] and got[-1] == cost[-1]
    # the declaration comes behind the tick rollout's and cites the reference's tick and its collision pass
    block = text[text.index("cost tick rollouts"):]
    assert text.index("int mrs_swarm_rollout_tick_device(") < text.index("int mrs_swarm_rollout_tick_cost_device(")
    assert "src/multirotor_simulator.cpp:211-217" in block and ":295-359" in block


def test_every_kernel_has_a_row_and_the_shape_of_its_mirror():
    k = rollout_kernels()
    mine = k.tick_families["_cost"]
    assert k.tick_types["_cost"] == ("RolloutTickCostDev", "RolloutTickCostHook")
    assert len(mine) == 4 and set(mine) == set(MIRRORS), sorted(mine)
    k.check_table(mine, RTC.ROLLOUT_TICK_COST_KERNELS, RTC, "cost tick")
    coll = macro_lines(open(os.path.join(CSRC, "step_device.inc")).read(), "MRS_STEP_KERNEL_COLL")
    single = {n for n, v in coll.items() if v[-1] == "false"}
    assert single == set(MIRRORS.values()), sorted(single)
    for name, args in mine.items():
        assert args == coll[MIRRORS[name]][:-1], (name, args, coll[MIRRORS[name]])
    # and of the tick kernel beside it
    assert {n.replace("_tick_cost", "_tick"): v for n, v in mine.items()} == k.tick
    # compiled by both step units (rollout_kernels checks that the two include lists are one), behind LaneObs and in front of the tick
    # rollout's own family, which stays last
    assert k.files.index("rollout_cost_device.inc") < k.files.index(FILE) == len(k.files) - 1
    assert list(k.tick_families)[-2:] == ["_cost", ""] and k.order[-8:] == list(mine) + list(k.tick)
    # none of them is a kernel the earlier tables know
    assert not set(mine) & ({n for fam in k.families.values() for n in fam} | set(k.tick)) and not set(mine) & set(k.step_kernels)
    for unit in STEP_UNITS:
        assert open(os.path.join(CSRC, unit)).read().count(f'#include "{FILE}"') == 1, unit


def test_no_other_kernel_lines_in_the_file():
    """no family, shape, tick-kernel or step-kernel line, and no schedule words: one launch is one tick"""
    k = rollout_kernels()
    text = k.texts[FILE]
    assert "MRS_STEP_KERNEL" not in text
    for macro in ("MRS_ROLLOUT_FAMILY", "MRS_ROLLOUT_SHAPE"):
        assert not re.search(rf"^\s*(#define\s+)?{macro}\(", text, flags=re.M), macro
    # one family line of its own, and the four shape lines of the family macro are every kernel line of the file
    assert len(re.findall(r"^MRS_ROLLOUT_TICK_FAMILY\(_cost, ", text, flags=re.M)) == 1
    assert len(macro_lines(text, "MRS_ROLLOUT_TICK_SHAPE")) == 4 and text.count("MRS_ROLLOUT_TICK_SHAPE(") == 5
    assert "mrs_ro_sched" not in text and "MRS_RO_" not in text and "mrs_ro_" not in text, "no schedule words"
    assert text.count("__global__") == 1, "the shape macro is the only kernel definition"
    # the descriptor is a kernel argument behind CollDev, whose offset is pinned for every family, and the header states the replay argument
    family = text[text.index("#define MRS_ROLLOUT_TICK_FAMILY("):text.index("MRS_ROLLOUT_TICK_FAMILY(_feedback")]
    assert "static_assert(offsetof(RolloutTickKernArgs<DevType>, cd) == offsetof(CollKernArgs, cd)" in family
    assert "no-op launch" in text.split("namespace {")[0]
    layout = open(os.path.join(CSRC, "swarm_layout.h")).read()
    body = layout[layout.index("struct RolloutTickCostDev {"):]
    body = body[:body.index("};")]
    assert "sched" not in body and "crash_cost" in body


_Swarm = stand_in("rollout_tick_device", "rollout_cost_device", "rollout_tick_cost_device")


def test_rollout_tick_cost_refuses_bad_tensors(monkeypatch):
    """CPU tensors dressed as cuda tensors (only .device is faked; nothing is launched)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64, f32, pos = _Swarm(), torch.float64, torch.float32, T.OBS_POS  # (mode 10: POSITION_CMD; OBS_POS: w = 3)

    def z(*shape, dtype=f64, dev=0):
        return on(torch.zeros(*shape, dtype=dtype), dev)

    cmd, tg, wt, out = z(6, 10, 4), z(3, 10, 3), z(3, 3), z(10)  # B = 6, hold = 2: 12 ticks, cost_every = 4: E = 3
    kw = dict(hold=2, cost_every=4)
    cases = [
        # CPU tensors and other devices
        (dict(commands=torch.zeros(6, 10, 4, dtype=f64)), "is on cpu"),
        (dict(targets=torch.zeros(3, 10, 3, dtype=f64)), "is on cpu"),
        (dict(weights=torch.zeros(3, 3, dtype=f64)), "is on cpu"),
        (dict(out=torch.zeros(10, dtype=f64)), "is on cpu"),
        (dict(commands=z(6, 10, 4, dev=1)), "the swarm lives on cuda:0"),
        (dict(targets=z(3, 10, 3, dev=1)), "the swarm lives on cuda:0"),
        (dict(out=z(10, dev=1)), "the swarm lives on cuda:0"),
        # dtypes
        (dict(commands=z(6, 10, 4, dtype=torch.float16)), "float32 or torch.float64"),
        (dict(targets=z(3, 10, 3, dtype=f32)), "targets has dtype torch.float32, the commands torch.float64"),
        (dict(weights=z(3, 3, dtype=f32)), "weights has dtype torch.float32, the commands torch.float64"),
        (dict(commands=z(6, 10, 4, dtype=f32)), "targets has dtype torch.float64, the commands torch.float32"),
        (dict(out=z(10, dtype=f32)), "the cost vector is always torch.float64"),
        # block counts, shapes and strides
        (dict(commands=z(10, 4)), r"\[T, count, width\]"),
        (dict(commands=z(6, 10, 3)), r">= 4\] tensor"),
        (dict(targets=z(4, 10, 3)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(12, 10, 3)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(3, 10, 2)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(3, 11, 3)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(10, 3)), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=None), r"targets: expected a \[3, 10 or 1, >= 3\]"),
        (dict(targets=z(3, 1, 5)[:, :, :3]), "shared rows must be dense"),
        (dict(targets=z(3, 3, 10).transpose(1, 2)), "rows are not contiguous"),
        (dict(targets=z(6, 10, 3)[::2]), "step dimension is not dense"),
        (dict(weights=z(2, 3)), r"weights: expected a \[3 or 1, >= 3\]"),
        (dict(weights=z(3)), r"weights: expected a \[3 or 1, >= 3\]"),
        (dict(weights=None), r"weights: expected a \[3 or 1, >= 3\]"),
        (dict(weights=z(3, 2)), r">= 3\] matrix"),
        (dict(weights=z(3, 3).t()), "rows are not contiguous"),
        (dict(out=z(9)), "vector of 10 elements"),
        (dict(out=z(20)[::2]), "not contiguous"),
        # groups == 0 with tensors, rates, accumulate
        (dict(groups=0), "groups == 0 is the crash cost alone"),
        (dict(groups=0, targets=None), "groups == 0 is the crash cost alone"),
        (dict(groups=0, weights=None), "groups == 0 is the crash cost alone"),
        (dict(hold=0), "hold must be at least 1"),
        (dict(cost_every=0), "cost_every must be at least 1 and divide the 12 ticks"),
        (dict(cost_every=5), "cost_every must be at least 1 and divide the 12 ticks"),
        (dict(cost_every=24), "cost_every must be at least 1 and divide the 12 ticks"),
        (dict(hold=3, cost_every=None), r"\[6, 10 or 1, >= 3\]"),  # cost_every defaults to hold: 18 ticks, E = 6
        (dict(out=None, accumulate=True), "accumulate=True needs the `out` vector"),
        (dict(commands=[[[0.0] * 4] * 10] * 6), "commands must be"),
    ]
    for change, msg in cases:
        a = dict(dict(commands=cmd, groups=pos, targets=tg, weights=wt, out=out, accumulate=False), **kw)
        a.update(change)
        with pytest.raises(ValueError, match=msg):
            T.rollout_tick_cost(g, 10, a.pop("commands"), 0.001, True, 100.0, a.pop("groups"), a.pop("targets"), a.pop("weights"), 1000.0, **a)
    with pytest.raises(ValueError, match="actuator rows must be dense"):
        T.rollout_tick_cost(g, T.ACTUATOR_CMD, z(6, 10, 6)[:, :, :4], 0.001, True, 100.0, pos, tg, wt, out=out, **kw)
    # well-formed calls pass every check of the tensor layer and reach rollout_tick_cost_device and nothing else
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    for a in (dict(groups=pos, targets=tg, weights=wt, out=out, **kw), dict(groups=pos, targets=z(3, 1, 3), weights=z(1, 3), out=out, **kw),
              dict(groups=pos, targets=z(3, 10, 7)[:, :, :3], weights=z(3, 8)[:, :3], out=z(30)[5:15], accumulate=True, **kw),
              dict(groups=pos, targets=z(6, 10, 3), weights=z(6, 3), hold=1, cost_every=1, out=out),
              dict(groups=0, targets=None, weights=None, out=out, **kw)):
        with pytest.raises(AssertionError, match=r"\(rollout_tick_cost_device\)"):
            T.rollout_tick_cost(g, 10, cmd, 0.001, False, 100.0, a.pop("groups"), a.pop("targets"), a.pop("weights"), 0.1, **a)


def test_arguments_handed_to_the_library(monkeypatch):
    """shared targets travel as target_stride 0, a single weight row as weight_stride 0, the crash-only form as null pointers"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    seen = []

    class Rec(_Swarm):
        def rollout_tick_cost_device(self, *a):
            seen.append(a)

    def z(*shape):
        return on(torch.zeros(*shape, dtype=torch.float64))

    cmd = z(6, 10, 4)
    T.rollout_tick_cost(Rec(), 10, cmd, 0.001, True, 50.0, T.OBS_POS, z(3, 10, 7)[:, :, :3], z(3, 8)[:, :3], 2.5, hold=2, cost_every=4, first=5,
                        out=z(10))
    T.rollout_tick_cost(Rec(), 10, cmd, 0.001, False, 50.0, T.OBS_POS, z(3, 1, 3), z(1, 8)[:, :3], hold=2, cost_every=4, out=z(10), accumulate=True)
    T.rollout_tick_cost(Rec(), 10, cmd, 0.001, True, 50.0, 0, None, None, 7.0, out=z(10))
    assert all(len(s) == len(NAMES) - 1 for s in seen)
    a, b, c = (dict(zip(NAMES[1:], s)) for s in seen)
    assert (a["first"], a["count"], a["n_ticks"], a["cmd_every"], a["cost_every"]) == (5, 10, 12, 2, 4)
    assert (a["target_stride"], a["weight_stride"], a["accumulate"], a["groups"], a["crash_cost"], a["crash"], a["rebounce"]) == (7, 8, False, T.OBS_POS, 2.5, True, 50.0)
    assert (b["target_stride"], b["weight_stride"], b["accumulate"], b["crash_cost"], b["crash"]) == (0, 0, True, 0.0, False)
    assert (c["groups"], c["dev_target"], c["dev_weight"], c["n_ticks"], c["cost_every"], c["crash_cost"]) == (0, 0, 0, 6, 1, 7.0)


def test_restatement_helper_is_the_stated_loop():
    """restate_ticks against the scalar loop of the ABI comment: shared and per-UAV rows, FP32 inputs, a start, the crash-only form, and
    crash costs that are 0, negative and non-finite (the add is performed whenever the byte is set)"""
    rng = np.random.default_rng(7)
    E, count, w = 4, 5, 3
    rows = rng.normal(size=(E, count, w))
    cr = rng.integers(0, 2, size=(E, count)).astype(bool)
    cr[:, 0] = False
    cr[:, 1] = True
    for tg, wt, start, cc in ((rng.normal(size=(E, count, w + 2)), rng.normal(size=(E, w + 1)), None, 1000.0),
                              (rng.normal(size=(E, 1, w)).astype(np.float32), rng.normal(size=(1, w)).astype(np.float32), rng.normal(size=count), 0.1),
                              (None, None, None, -3.5), (None, None, rng.normal(size=count), np.inf),
                              (rng.normal(size=(E, count, w)), rng.normal(size=(1, w)), np.full(count, -0.0), 0.0)):
        want = np.zeros(count)
        for k in range(count):
            c = 0.0 if start is None else float(start[k])
            for j in range(E):
                if tg is not None:
                    term = 0.0
                    for col in range(w):
                        d = float(rows[j, k, col]) - float(tg[j, k if tg.shape[1] > 1 else 0, col])
                        term = term + (float(wt[j if wt.shape[0] > 1 else 0, col]) * d) * d
                    c = c + term
                if cr[j, k]:
                    c = c + cc
            want[k] = c
        got = RTC.restate_ticks(rows if tg is not None else None, cr, tg, wt, cc, start)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (cc, got, want)
    # -0.0 + 0.0 is +0.0: a crashed UAV's add of a zero crash cost shows in the sign bit of a -0.0 start, an uncrashed one keeps it
    z = RTC.restate_ticks(None, np.array([[True, False]]), None, None, 0.0, np.array([-0.0, -0.0]))
    assert list(np.signbit(z)) == [False, True]


def test_rollout_tick_cost_test_compiles(mrs, tmp_path):
    from mrs_multirotor_simulator_amd import swarm
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DMRS_NO_EIGEN", "-D__HIP_PLATFORM_AMD__", "-I",
                           os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "rollout_tick_cost_test.cpp"),
                           "-o", str(tmp_path / "rollout_tick_cost_test"), "-L", os.path.dirname(swarm.LIB_PATH), "-lmrs_swarm", "-L", "/opt/rocm/lib",
                           "-lamdhip64", "-lpthread"])
