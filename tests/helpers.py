"""Shared scenario builders for the parity tests: the same calls are issued to the CPU oracle
(oracle/oracle_swarm.py — test infrastructure) and to the product (mrs_multirotor_simulator_amd.Swarm).  Further down, what the
CPU-side test files share: the prototypes of include/mrs_swarm.h (abi_prototype), CPU tensors dressed as cuda tensors (fake_cuda), a
swarm whose library calls may not be reached (stand_in), and the rollout kernels as the sources define them (rollout_kernels)."""
import ctypes as C
import os
import re

import numpy as np

from mrs_multirotor_simulator_amd import airframes
from oracle import oracle_swarm as O

# tolerance of BASELINE.json's north_star: state L-inf <= 1e-6 relative, FP64
RTOL_NORTH_STAR = 1e-6
# what the LITERAL kernel actually achieves against the scalar oracle (libm sin/cos may differ by an ulp)
RTOL_LITERAL = 1e-11
# FAST kernel (FMA contraction, reciprocals) vs oracle over short horizons
RTOL_FAST = 1e-8


def oracle_params(name, **kw):
    p = O.ModelParams()
    O.lib().orc_model_params_default(p)
    airframes.fill_params(p, name, **kw)
    O.lib().orc_calculate_inertia(p)
    O.lib().orc_scale_allocation(p)
    return p


def reference_kdtree(name, pos):
    """The reference's own kd-tree (nanoflann, squared radius 3.0, leaf size 10) on the stored scenario `name`: (offsets, idx, d2)
    in the order its radius search hands the neighbours out, from tests/golden/reference_kdtree_scenarios.npz
    (tests/golden/make_golden.py:kdtree_scenarios).  The stored points must be `pos` bit for bit; where oracle/_ref is built, the
    library itself must still return the stored lists."""
    key = re.sub(r"[^0-9A-Za-z]+", "_", name)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_kdtree_scenarios.npz"))
    assert np.array_equal(g[f"{key}_points"], pos), f"{name}: the stored scenario no longer matches the test's points"
    off, idx, d2 = g[f"{key}_offsets"], g[f"{key}_indices"], g[f"{key}_d2"]
    if O.ref_lib() is not None:
        lo, li, ld = O.ref_radius_neighbours(pos, 3.0, 10)
        assert np.array_equal(lo, off) and np.array_equal(li, idx) and np.array_equal(ld, d2), f"{name}: live kd-tree != stored lists"
    return off, idx, d2


def to_product_params(M, p):
    return M.ModelParams.from_buffer_copy(bytes(p))


from mrs_multirotor_simulator_amd.synthetic import random_rotations, random_state, tilted_rotations  # noqa: E402,F401  (shared with bench.py)


class Pair:
    """An oracle swarm and a product swarm driven in lockstep."""

    def __init__(self, M, n, arith=0):
        self.M, self.n = M, n
        self.o = O.OracleSwarm(n)
        self.g = M.Swarm(n, arith=arith)

    def both(self, name, *a, **kw):
        getattr(self.o, name)(*a, **kw)
        getattr(self.g, name)(*a, **kw)

    def construct(self, first, count, airframe, pos=None, heading=None, **kw):
        po = oracle_params(airframe, **kw)
        self.o.construct(first, count, po, pos, heading)
        self.g.construct(first, count, to_product_params(self.M, po), pos, heading)
        # UavSystemRos init order: controller params set after construction (src/uav_system_ros.cpp:109-157)
        for nm in ("set_mixer_params", "set_rate_params", "set_attitude_params", "set_velocity_params", "set_position_params"):
            self.both(nm, first, count)
        return po

    def set_state(self, first, count, st):
        self.both("set_state", first, count, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])

    def step(self, dt, n=1):
        self.o.step_n(dt, n)
        self.g.step_n(dt, n)

    def compare(self, rtol, what="", fields=("x", "v", "v_prev", "R", "omega", "motor_rpm"), mask=None):
        """mask: boolean per UAV — only these rows are compared (campaigns that have to leave diverging closed loops out)"""
        a, b = self.g.get_state(), self.o.get_state()
        a["imu"], b["imu"] = self.g.get_imu(), self.o.get_imu()
        a["pid"], b["pid"] = self.g.get_pid(), self.o.get_pid()
        if mask is not None:
            a, b = {k: v[mask] for k, v in a.items()}, {k: v[mask] for k, v in b.items()}
        worst = 0.0
        for k in tuple(fields) + ("imu", "pid"):
            worst = max(worst, assert_close(a[k], b[k], rtol, f"{what}:{k}"))
        # north_star's measure is the state-vector L-inf of each UAV, not of the swarm: a UAV near the origin must not hide
        # behind the coordinates of one 500 m away
        self.worst_uav = assert_close_per_uav(a, b, rtol, what)
        return worst


def rel_linf(a, b):
    """max |a-b| / max(|b|) over the array (L-inf relative); NaN patterns must match exactly."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), "NaN pattern differs"
    ia, ib = np.isinf(a), np.isinf(b)
    assert np.array_equal(ia, ib) and np.array_equal(a[ia], b[ib]), "inf pattern differs"
    m = ~(na | ia)
    if not m.any():
        return 0.0
    scale = np.max(np.abs(b[m]))
    diff = np.max(np.abs(a[m] - b[m]))
    return 0.0 if diff == 0 else diff / max(scale, 1e-300)


# per-UAV measures -------------------------------------------------------------------------------------------------
STATE_FIELDS = ("x", "v", "R", "omega", "motor_rpm")  # MultirotorModel::State, multirotor_model.hpp:90-98 (v_prev is a copy of v)
# below these magnitudes a field is compared absolutely (a hovering UAV has v = omega = 0 exactly: no relative measure exists there)
FIELD_FLOOR = {"x": 1.0, "v": 1.0, "v_prev": 1.0, "R": 1.0, "omega": 1.0, "motor_rpm": 1000.0, "imu": 9.81, "pid": 1.0, "f": 1.0}


def per_uav_linf(a, b, fields=STATE_FIELDS):
    """Two per-UAV relative L-inf errors of a state dict `a` against the reference `b` (arrays [n, ...]):
      state : max_c |a_c - b_c| / max(||state_i||_inf, 1)   — the whole state vector of UAV i (north_star, literally)
      field : max over fields of  max_c |a_c - b_c| / max(||field_i||_inf, floor_field)   — every field on its own scale (stricter:
              the rpm entries ~4000 do not set the scale for R or omega)
    NaN / inf patterns must match exactly.  Returns (state_err[n], field_err[n])."""
    n = len(np.asarray(b[fields[0]]))
    num_state, den_state, field_err = np.zeros(n), np.ones(n), np.zeros(n)
    for k in fields:
        x, y = np.asarray(a[k], dtype=np.float64).reshape(n, -1), np.asarray(b[k], dtype=np.float64).reshape(n, -1)
        bad = ~np.isfinite(y)
        assert np.array_equal(np.isnan(x), np.isnan(y)), f"{k}: NaN pattern differs"
        assert np.array_equal(x[bad & ~np.isnan(y)], y[bad & ~np.isnan(y)]), f"{k}: inf pattern differs"
        d = np.where(bad, 0.0, np.abs(np.where(bad, 0.0, x) - np.where(bad, 0.0, y))).max(axis=1)
        m = np.where(bad, 0.0, np.abs(y)).max(axis=1)
        num_state, den_state = np.maximum(num_state, d), np.maximum(den_state, m)
        field_err = np.maximum(field_err, d / np.maximum(m, FIELD_FLOOR.get(k, 1.0)))
    return num_state / den_state, field_err


def assert_close_per_uav(a, b, rtol, what="", fields=STATE_FIELDS):
    """every UAV's own state vector within rtol (both measures of per_uav_linf); returns (worst UAV, its field error)"""
    se, fe = per_uav_linf(a, b, fields)
    i = int(np.argmax(fe))
    assert fe[i] <= rtol, (f"{what}: UAV {i} is off by {fe[i]:.3e} > {rtol:.1e} relative to its own fields "
                           f"(state-vector measure {se[i]:.3e}; worst state-vector UAV {int(np.argmax(se))}: {se.max():.3e})")
    assert se.max() <= rtol
    return i, float(fe[i])


def assert_close(a, b, rtol, what=""):
    e = rel_linf(a, b)
    assert e <= rtol, f"{what}: relative L-inf error {e:.3e} > {rtol:.1e}"
    return e


# the C ABI as include/mrs_swarm.h declares it ----------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"mrs_swarm_t*": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
         "double": C.c_double}


def abi_header():
    """include/mrs_swarm.h without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrs_swarm.h")).read(), flags=re.S)


def abi_prototype(name):
    """(parameter names, C types) of the prototype `int name(...);` in include/mrs_swarm.h, a pointer's star written with its type"""
    m = re.search(r"int\s+" + name + r"\(([^)]*)\);", abi_header())
    assert m, f"prototype of {name}"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    types = [re.match(r"(.*?)\s*\b\w+$", p).group(1).replace(" *", "*") for p in params]
    return [p.rsplit(" ", 1)[-1].lstrip("*") for p in params], types


# the tensor layer without a GPU ------------------------------------------------------------------------------------------------
class _Dev:
    def __init__(self, index):
        self.type, self.index = "cuda", index

    def __str__(self):
        return f"cuda:{self.index}"


def fake_cuda(monkeypatch):
    """on(t, index=0): the CPU tensor `t` dressed as a tensor on cuda:index.  Only .device is faked, so nothing can be launched; a
    tensor made from a dressed one (a slice, a view) says cuda:0."""
    import torch

    class Fake(torch.Tensor):
        pass

    def on(t, index=0):
        f = t.as_subclass(Fake)
        f._fake_dev = _Dev(index)
        return f

    monkeypatch.setattr(Fake, "device", property(lambda self: getattr(self, "_fake_dev", _Dev(0))), raising=False)
    return on


def stand_in(*methods):
    """A class that stands in for a Swarm of 100 UAVs on cuda:0 where no library call may be reached: each of the named methods raises
    AssertionError("the call reached the library (<name>)"), and a method that is not named does not exist.  A subclass overrides
    the calls it wants to take."""
    def refuse(name):
        def method(self, *a):
            raise AssertionError(f"the call reached the library ({name})")
        return method

    return type("StandIn", (), dict({m: refuse(m) for m in methods}, n=100, device=lambda self: 0))


# the rollout kernels, as the sources define them -------------------------------------------------------------------------------
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mrs_multirotor_simulator_amd", "csrc")
STEP_UNITS = ("step_kernel_fast.hip", "step_kernel_literal.hip")
ROLLOUT_FAMILIES = ["", "_rate", "_force", "_cost", "_feedback"]  # the infixes of the MRS_ROLLOUT_FAMILY lines, in definition order


def macro_lines(text, macro):
    """{kernel: [bounds, argument, ...]} of the `macro(kernel, (bounds), ...)` instantiation lines of a source text, in order"""
    out = {}
    for line in text.splitlines():
        m = re.match(rf"{macro}\(\s*([\w#]+)\s*,\s*(\(.*?\))\s*,\s*(.*?)\)\s*\\?$", line.strip())
        if m:
            out[m.group(1)] = [m.group(2).replace(" ", "")] + [a.strip() for a in m.group(3).split(",")]
    return out


class RolloutKernels:
    """The rollout kernels both step units compile, from the sources: every MRS_ROLLOUT_FAMILY(infix, descriptor, hook) line of the
    included rollout files times the MRS_ROLLOUT_SHAPE lines of that macro, and likewise every MRS_ROLLOUT_TICK_FAMILY line times the
    MRS_ROLLOUT_TICK_SHAPE lines.
      families : {infix: {kernel: [bounds, CASCADE, UNIFORM, BUF]}}, infixes and kernels in definition order
      types    : {infix: (descriptor, hook)}
      tick_families, tick_types : the same of the tick families, {kernel: [bounds, CASCADE, UNIFORM, ACC, SU]}
      tick     : the kernels of the tick family without an infix (the tick rollout's own)
      order    : every kernel name in definition order
      files    : the rollout files in include order; texts : {file: text}"""

    def __init__(self):
        lists = []
        for unit in STEP_UNITS:
            text = open(os.path.join(CSRC, unit)).read()
            lists.append(re.findall(r'^#include "(\w+\.inc)"$', text, flags=re.M))
            assert text.rstrip().endswith('#include "%s"' % lists[-1][-1]), unit
        assert lists[0] == lists[1], "both step units compile the same files in the same order"
        assert lists[0][0] == "step_device.inc"
        self.files = [f for f in lists[0] if f.startswith("rollout_")]
        assert self.files == lists[0][1:], "the rollout files come behind step_device.inc, and nothing else does"
        self.texts = {f: open(os.path.join(CSRC, f)).read() for f in self.files}
        shapes = macro_lines(self.texts["rollout_device.inc"], "MRS_ROLLOUT_SHAPE")
        assert all(v[-2:] == ["DevType", "HookType"] for v in shapes.values()), shapes
        tick_shapes = macro_lines(self.texts["rollout_tick_device.inc"], "MRS_ROLLOUT_TICK_SHAPE")
        assert all(v[-2:] == ["DevType", "HookType"] for v in tick_shapes.values()), tick_shapes
        self.families, self.types, self.tick_families, self.tick_types, self.order = {}, {}, {}, {}, []
        for f in self.files:
            for infix, dev, hook in re.findall(r"^MRS_ROLLOUT_FAMILY\((\w*), (\w+), (\w+)\)$", self.texts[f], flags=re.M):
                assert infix not in self.families, infix
                self.types[infix] = (dev, hook)
                self.families[infix] = {k.replace("##infix##", infix).replace("##infix", infix): v[:-2] for k, v in shapes.items()}
                self.order += list(self.families[infix])
            for infix, dev, hook in re.findall(r"^MRS_ROLLOUT_TICK_FAMILY\((\w*), (\w+), (\w+)\)$", self.texts[f], flags=re.M):
                assert infix not in self.tick_families, infix
                self.tick_types[infix] = (dev, hook)
                self.tick_families[infix] = {k.replace("##infix##", infix).replace("##infix", infix): v[:-2] for k, v in tick_shapes.items()}
                self.order += list(self.tick_families[infix])
        self.tick = self.tick_families[""]
        step = open(os.path.join(CSRC, "step_device.inc")).read()
        self.step_kernels = re.findall(r"MRS_STEP_KERNEL\w*\(\s*(\w+)", step)

    def check_table(self, names, table, module, what):
        """the kernels `names` and the rows of a *_KERNELS table of a GPU test module correspond, every row names tests of that
        module, and none of the kernels is compiled twice or is a step-kernel line of step_device.inc"""
        names, rows = set(names), set(table)
        assert not names - rows, f"{what} kernels without a row: {sorted(names - rows)}"
        assert not rows - names, f"rows naming {what} kernels that are no longer compiled: {sorted(rows - names)}"
        for kernel, where in table.items():
            assert where, kernel
            for w in where:
                assert callable(getattr(module, w.split("[")[0], None)), f"{kernel}: {w} is no test of {module.__name__}"
        assert len(self.order) == len(set(self.order)), "a rollout kernel is defined twice"
        assert "rollout" not in " ".join(self.step_kernels) and not set(self.order) & set(self.step_kernels)
        assert not any("MRS_STEP_KERNEL" in t for t in self.texts.values()), "the step-kernel table of test_step_kernel_table stays as it is"

    def check_family(self, infix, table, module, mirrors=None):
        """family `infix` is five kernels with a row each in `table`; it comes behind the family `mirrors` (an infix) and has its
        shapes, launch bounds included, kernel for kernel"""
        fam = self.families[infix]
        assert len(fam) == 5, sorted(fam)
        self.check_table(fam, table, module, f"rollout{infix}")
        assert list(self.families) == ROLLOUT_FAMILIES, "the families, in the order the later ones build on the earlier"
        if mirrors is not None:
            assert ROLLOUT_FAMILIES.index(mirrors) < ROLLOUT_FAMILIES.index(infix)
            assert {k.replace("rollout" + infix, "rollout" + mirrors): v for k, v in fam.items()} == self.families[mirrors]


_rollout_kernels = []


def rollout_kernels():
    if not _rollout_kernels:
        _rollout_kernels.append(RolloutKernels())
    return _rollout_kernels[0]
