"""CPU-side checks of the obstacle contacts (include/mrs_swarm.h, "obstacle contacts"): the numpy restatement the GPU tests compare bits
against (restate_contacts below, built on signed_distances and the world rule of test_obstacles.py) is checked on its own with known
answers at the exact threshold and against a scalar definition; the restatement alone asserts what the fixture scene covers; the symbol
is exported and listed, header prototype, ctypes argtypes and method signature agree, the header's value is the Python one, the unit
and its header are in the build lists; the tensor wrapper refuses bad arguments before the library is reached; and the fold over the
cell walk (csrc/obstacle_contact.h) passes tests/cpp/obstacle_contact_math_test.cpp under the address and undefined-behaviour
sanitizers, where its results for the points listed here equal the restatement's bits.  No pointer reaches the library."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import CTYPE, abi_header, abi_prototype, fake_cuda, stand_in
from test_obstacles import ALL_WORLDS, BOX, CYLINDER, OBSTACLE, SPHERE, fixture_scene, obstacles, same_bits, signed_distances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mrs_swarm_obstacle_contacts_device"
AIRFRAMES = ("x500", "f550", "t650")
MARGINS = (0.0, 0.25, 1.0)
TYPES = dict(CTYPE, **{"double*": C.c_void_p, "int32_t*": C.c_void_p, "uint8_t*": C.c_void_p})


# ---- the numpy restatement (used by test_obstacle_contacts_gpu.py) ----

def body_radius(name):
    """rad = arm_length + prop_radius of an airframe, one FP64 addition"""
    from mrs_multirotor_simulator_amd.airframes import AIRFRAMES as A
    return np.float64(A[name]["arm_length"]) + np.float64(A[name]["prop_radius"])


def fixture_radii(n=3072):
    """rad [n] of the fixture scene's UAVs: x500 / f550 / t650 in thirds, as scene_swarm of test_obstacles_gpu.py constructs them"""
    third = n // 3
    return np.concatenate([np.full(third, body_radius("x500")), np.full(third, body_radius("f550")), np.full(n - 2 * third, body_radius("t650"))])


@np.errstate(all="ignore")
def restate_contacts(pos, worlds, obst, rad, margin):
    """The contract of mrs_swarm_obstacle_contacts_device for every UAV: thr = rad + margin (one FP64 addition; rad [n] or a scalar), the
    touching set C = the obstacles that apply (ALL_WORLDS, or the UAV's label; worlds None: all 0) with sd < thr, empty for a non-finite
    position.  Returns a dict: hit [n] uint8, count [n] int32 (uncapped), index [n] int32 (the lexicographic minimum of (sd, j); -1:
    none), sd [n] (that distance; +inf: none), thr [n]."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    n, M = len(pos), len(obst)
    worlds = np.zeros(n, np.int32) if worlds is None else np.asarray(worlds).astype(np.int32)
    thr = np.broadcast_to(np.asarray(rad, np.float64), (n,)) + np.float64(margin)
    out = dict(hit=np.zeros(n, np.uint8), count=np.zeros(n, np.int32), index=np.full(n, -1, np.int32), sd=np.full(n, np.inf), thr=thr)
    if M == 0 or n == 0:
        return out
    sd, _ = signed_distances(pos, obst)
    applies = ((obst["flags"] & ALL_WORLDS) != 0)[None, :] | (obst["world"][None, :] == worlds[:, None])
    touch = applies & (sd < thr[:, None]) & np.isfinite(pos).all(axis=1)[:, None]
    count = touch.sum(axis=1)
    best = np.argmin(np.where(touch, sd, np.inf), axis=1)  # the first minimum: ties, and -0.0 == +0.0, go to the lower index
    hit = count > 0
    out["hit"], out["count"] = hit.astype(np.uint8), count.astype(np.int32)
    out["index"] = np.where(hit, best, -1).astype(np.int32)
    out["sd"] = np.where(hit, sd[np.arange(n), best], np.inf)
    return out


def cost_after(cost, res, hit_cost):
    """what the call leaves in dev_cost: cost + hit_cost (one FP64 addition) where the UAV touches, the element as it was elsewhere — NaN
    payloads included, so compare with same_bits"""
    cost = np.asarray(cost, np.float64)
    with np.errstate(all="ignore"):
        return np.where(res["hit"] != 0, cost + np.float64(hit_cost), cost)


_ref = {}


def fixture_contacts(margin, labels=True):
    """the restatement of the fixture scene at `margin`, computed once and shared (never written to)"""
    key = (float(margin), labels)
    if key not in _ref:
        pos, worlds, ob = fixture_scene()
        _ref[key] = restate_contacts(pos, worlds if labels else None, ob, fixture_radii(len(pos)), margin)
        for a in _ref[key].values():
            a.setflags(write=False)
    return _ref[key]


# ---- tests: the restatement ----

def one(p, ob, rad, margin, worlds=None):
    return restate_contacts(np.atleast_2d(np.asarray(p, np.float64)), worlds, ob, rad, margin)


def test_restatement_at_the_exact_threshold_per_kind():
    """sd == thr misses, one nextafter closer hits, with thr = fl(rad + margin) formed in that order; every number below is exact"""
    rad = body_radius("x500")
    assert rad == np.float64(0.25) + np.float64(0.15) and rad == 0.4
    sets = [obstacles([(SPHERE, (0.0, 0.0, 0.0), (1.0, 0, 0))]), obstacles([(BOX, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))]),
            obstacles([(CYLINDER, (0.0, 0.0, 0.0), (1.0, 0, np.inf))])]
    for nice in (0.5, 0.75, 1.5):  # margins for which thr is a short binary fraction: a UAV at 1 + thr is exactly thr from the surface
        margin = np.float64(nice) - rad
        thr = rad + margin
        at = 1.0 + thr
        assert thr == nice and at - 1.0 == thr and margin > 0, nice
        closer = np.nextafter(at, 0.0)
        for ob in sets:
            r = one((at, 0.0, 0.0), ob, rad, margin)
            assert r["hit"][0] == 0 and r["count"][0] == 0 and r["index"][0] == -1 and r["sd"][0] == np.inf and r["thr"][0] == thr
            r = one((closer, 0.0, 0.0), ob, rad, margin)
            assert r["hit"][0] == 1 and r["count"][0] == 1 and r["index"][0] == 0 and r["sd"][0] == closer - 1.0 < thr
    # the order of the two additions matters: (arm + prop) + margin, not arm + (prop + margin)
    arm, prop, margin = np.float64(0.27), np.float64(0.11), np.float64(0.1)
    assert (arm + prop) + margin != arm + (prop + margin)
    assert one((0, 0, 0), sets[0], arm + prop, margin)["thr"][0] == (arm + prop) + margin
    # per-UAV radii: the same point touches with the larger airframe only
    p = np.array([[1.5, 0.0, 0.0], [1.5, 0.0, 0.0]])
    r = restate_contacts(p, None, sets[0], np.array([body_radius("x500"), body_radius("t650")]), 0.0)
    assert list(r["hit"]) == [0, 1] and body_radius("x500") < 0.5 < body_radius("t650")


def test_restatement_ties_overlaps_worlds_and_non_finite():
    rad = body_radius("x500")
    # two obstacles at equal sd: the lower index; the nearer one whatever its index; the count is not capped
    ob = obstacles([(SPHERE, (5.0, 0.0, 0.0), (1.0, 0, 0)), (BOX, (2.0, 0.0, 0.0), (0.5, 0.5, 0.5)), (SPHERE, (5.0, 0.0, 0.0), (1.0, 0, 0)),
                    (BOX, (2.0, 0.0, 0.0), (0.5, 0.5, 0.5))])
    r = one((0.0, 0.0, 0.0), ob, rad, 10.0)
    assert r["count"][0] == 4 and r["index"][0] == 1 and r["sd"][0] == 1.5
    assert one((0.0, 0.0, 0.0), ob[[0, 2]], rad, 10.0)["index"][0] == 0
    # -0.0 against +0.0: on the surface of a box sd = sqrt(0) + min(max(-0.0 ...)): the tie goes to the lower index, with its own zero
    zeros = obstacles([(SPHERE, (0.0, 0.0, 0.0), (1.0, 0, 0)), (BOX, (2.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    sd, _ = signed_distances(np.array([[1.0, 0.0, 0.0]]), zeros)
    assert (sd == 0.0).all()
    r = one((1.0, 0.0, 0.0), zeros, rad, 0.0)
    assert r["count"][0] == 2 and r["index"][0] == 0 and same_bits(r["sd"], sd[:, 0])
    r = one((1.0, 0.0, 0.0), zeros[::-1], rad, 0.0)
    assert r["index"][0] == 0 and same_bits(r["sd"], sd[:, 1])
    # inside overlapping solids: the deepest first
    deep = obstacles([(SPHERE, (0.0, 0.0, 0.0), (1.0, 0, 0)), (SPHERE, (0.0, 0.0, 0.0), (3.0, 0, 0)), (BOX, (0.0, 0.0, 0.0), (2.0, 2.0, 2.0))])
    r = one((0.5, 0.0, 0.0), deep, rad, 0.0)
    assert r["count"][0] == 3 and r["index"][0] == 1 and r["sd"][0] == -2.5
    # worlds
    ob = obstacles([(SPHERE, (0, 0, 0), (1.0, 0, 0), 0), (SPHERE, (0, 0, 0), (2.0, 0, 0), 5), (SPHERE, (0, 0, 0), (0.5, 0, 0), -3, ALL_WORLDS)])
    r = restate_contacts(np.zeros((3, 3)), [0, 5, 9], ob, rad, 0.0)
    assert list(r["count"]) == [2, 2, 1] and list(r["index"]) == [0, 1, 2] and list(r["sd"]) == [-1.0, -2.0, -0.5]
    assert list(restate_contacts(np.zeros((3, 3)), None, ob, rad, 0.0)["count"]) == [2, 2, 2]
    # non-finite positions, a NaN threshold, an empty set: nothing touches
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.0, 0.0, 0.0]])
    r = restate_contacts(bad, None, deep, rad, 0.0)
    assert list(r["hit"]) == [0, 0, 0, 1] and list(r["index"][:3]) == [-1] * 3 and (r["sd"][:3] == np.inf).all() and (r["count"][:3] == 0).all()
    r = restate_contacts(bad, None, deep, np.nan, 0.0)
    assert (r["hit"] == 0).all() and (r["index"] == -1).all()
    e = restate_contacts(bad, None, np.zeros(0, OBSTACLE), rad, 0.0)
    assert (e["hit"] == 0).all() and (e["index"] == -1).all() and (e["sd"] == np.inf).all() and e["hit"].dtype == np.uint8
    # the cost: one addition where touching, the element (a NaN payload included) untouched elsewhere
    payload = np.array([0x7FF8000000001234], np.uint64).view(np.float64)[0]
    cost = np.array([payload, payload, 1.5, -0.0])
    r = restate_contacts(bad, None, deep, rad, 0.0)
    after = cost_after(cost, r, 2.25)
    assert same_bits(after[:3], cost[:3]) and after[3] == 2.25 and not same_bits(after[:1], [np.nan])


def test_restatement_equals_a_scalar_definition():
    """the vectorised restatement against one (UAV, obstacle) pair at a time in Python floats, on a slice of the fixture"""
    pos, worlds, ob = fixture_scene()
    rad = fixture_radii(len(pos))
    sel = np.r_[0:40, 64:100, 198:204, 1000:1040, 2040:2060, 3000:3072]

    def mx(a, b):
        return b if a < b else a

    def mn(a, b):
        return b if b < a else a

    touching = 0
    for margin in MARGINS:
        res = fixture_contacts(margin)
        for i in sel:
            p = [float(v) for v in pos[i]]
            thr = float(rad[i]) + margin
            hits = []
            if all(math.isfinite(v) for v in p):
                for j, o in enumerate(ob):
                    if not (o["flags"] & ALL_WORLDS) and o["world"] != worlds[i]:
                        continue
                    dx, dy, dz = (p[a] - float(o["c"][a]) for a in range(3))
                    h = [float(v) for v in o["h"]]
                    if o["kind"] == SPHERE:
                        sd = math.sqrt(((dx * dx) + dy * dy) + dz * dz) - h[0]
                    elif o["kind"] == BOX:
                        a0, a1, a2 = abs(dx) - h[0], abs(dy) - h[1], abs(dz) - h[2]
                        m0, m1, m2 = mx(a0, 0.0), mx(a1, 0.0), mx(a2, 0.0)
                        sd = math.sqrt(((m0 * m0) + m1 * m1) + m2 * m2) + mn(mx(a0, mx(a1, a2)), 0.0)
                    else:
                        ar, az = math.sqrt((dx * dx) + dy * dy) - h[0], abs(dz) - h[2]
                        sd = math.sqrt((mx(ar, 0.0) * mx(ar, 0.0)) + mx(az, 0.0) * mx(az, 0.0)) + mn(mx(ar, az), 0.0)
                    if sd < thr:
                        hits.append((sd, j))
            hits.sort()
            assert res["count"][i] == len(hits) and res["hit"][i] == (1 if hits else 0), (margin, i)
            assert res["index"][i] == (hits[0][1] if hits else -1), (margin, i)
            assert same_bits(res["sd"][i:i + 1], [hits[0][0] if hits else np.inf]), (margin, i)
            touching += bool(hits)
    assert touching > 100


def test_fixture_coverage():
    pos, worlds, ob = fixture_scene()
    n = len(pos)
    rad = fixture_radii(n)
    assert n == 3072 and len(ob) == 384 and sorted(set(rad)) == sorted(body_radius(a) for a in AIRFRAMES)
    want = {0.0: (586, 125, 28), 0.25: (721, 164, 33), 1.0: (1186, 388, 40)}
    for margin in MARGINS:
        r = fixture_contacts(margin)
        assert (int(r["hit"].sum()), int((r["count"] > 1).sum()), int(r["count"].max())) == want[margin], margin
        assert (r["hit"] == (r["count"] > 0)).all() and ((r["index"] >= 0) == (r["hit"] != 0)).all() and (np.isinf(r["sd"]) == (r["hit"] == 0)).all()
    r0 = fixture_contacts(0.0)
    assert int((r0["sd"] < 0).sum()) == 392, "UAVs inside a solid"
    touched = ob["kind"][r0["index"][r0["hit"] != 0]]
    # every kind is touched (as the nearest obstacle, or at all), and every airframe touches
    sd, _ = signed_distances(pos, ob)
    applies = ((ob["flags"] & ALL_WORLDS) != 0)[None, :] | (ob["world"][None, :] == worlds[:, None])
    with np.errstate(invalid="ignore"):
        touch = applies & (sd < rad[:, None]) & np.isfinite(pos).all(axis=1)[:, None]
    per_kind = [int(touch[:, ob["kind"] == kind].any(axis=1).sum()) for kind in (SPHERE, BOX, CYLINDER)]
    assert per_kind == [146, 184, 416] and set(touched) == {SPHERE, BOX, CYLINDER}
    third = n // 3
    assert [int(r0["hit"][a * third:(a + 1) * third].sum()) for a in range(3)] == [260, 152, 174]
    # the airframe matters: at least one UAV's decision differs between the smallest and the largest of the three radii
    small, large = min(body_radius(a) for a in AIRFRAMES), max(body_radius(a) for a in AIRFRAMES)
    a, b = restate_contacts(pos, worlds, ob, small, 0.0), restate_contacts(pos, worlds, ob, large, 0.0)
    assert small < large and (a["hit"] != b["hit"]).sum() >= 1 and (a["hit"] <= b["hit"]).all()
    # the labels matter, and the non-finite positions touch nothing at any margin
    assert (fixture_contacts(0.0, labels=False)["count"] != r0["count"]).sum() > 50
    bad = ~np.isfinite(pos).all(axis=1)
    assert bad.sum() == 2
    for margin in MARGINS:
        r = fixture_contacts(margin)
        assert (r["hit"][bad] == 0).all() and (r["count"][bad] == 0).all() and (r["index"][bad] == -1).all()


# ---- tests: the ABI ----

def test_symbol_is_declared_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import build, swarm, tensors
    L = C.CDLL(swarm.LIB_PATH)
    header = abi_header()
    assert re.search(r"\bint\s+" + NAME + r"\(", header)
    assert hasattr(L, NAME) and NAME in swarm.ABI_SYMBOLS and swarm.ABI_SYMBOLS.count(NAME) == 1
    assert callable(getattr(swarm.Swarm, "obstacle_contacts_device", None)) and callable(getattr(tensors, "obstacle_contacts", None))
    m = re.search(r"\bMRS_CONTACT_CRASH\s*=\s*1\s*<<\s*0\b", header)
    assert m and swarm.CONTACT_CRASH == tensors.CONTACT_CRASH == 1
    assert ("obstacle_contact.hip", "off") in build.UNITS and "obstacle_contact.h" in build.DEPS
    for f in ("obstacle_contact.hip", "obstacle_contact.h"):
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    facade = open(os.path.join(ROOT, "include", "mrs_multirotor_simulator", "uav_system", "uav_system.hpp")).read()
    assert re.search(r"\bobstacleContactsDevice\(", facade)


def test_header_prototype_argtypes_and_method_agree(mrs):
    from mrs_multirotor_simulator_amd import swarm, tensors
    L = swarm.load_library()
    names = ["s", "first", "count", "margin", "flags", "dev_hit", "dev_index", "dev_sd", "dev_count", "dev_cost", "hit_cost", "ext_stream"]
    got_names, types = abi_prototype(NAME)
    assert got_names == names
    assert types == ["mrs_swarm_t*", "int32_t", "int32_t", "double", "uint32_t", "uint8_t*", "int32_t*", "double*", "int32_t*", "double*", "double",
                     "void*"]
    got = [C.c_void_p if issubclass(a, C._Pointer) else a for a in getattr(L, NAME).argtypes]
    assert [TYPES[t] for t in types] == got
    assert list(inspect.signature(swarm.Swarm.obstacle_contacts_device).parameters) == ["self"] + names[1:]
    sig = inspect.signature(tensors.obstacle_contacts)
    assert list(sig.parameters) == ["swarm", "margin", "crash", "first", "count", "hit", "index", "sd", "counts", "cost", "hit_cost"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(margin=0.0, crash=False, first=0, count=None, hit=None, index=None, sd=None, counts=None, cost=None, hit_cost=0.0)


# ---- tests: the tensor layer without a GPU ----

_Swarm = stand_in("obstacle_contacts_device")


def test_wrapper_refuses_before_the_library(monkeypatch):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64, i32, u8 = _Swarm(), torch.float64, torch.int32, torch.uint8
    cases = [
        (dict(hit=torch.zeros(100, dtype=u8)), "is on cpu"),
        (dict(hit=on(torch.zeros(100, dtype=u8), 1)), "the swarm lives on cuda:0"),
        (dict(hit=on(torch.zeros(100, dtype=torch.bool))), "hit has dtype torch.bool, expected torch.uint8"),
        (dict(hit=on(torch.zeros(99, dtype=u8))), "expected a vector of 100 elements"),
        (dict(hit=on(torch.zeros(200, dtype=u8)[::2])), "vector is not contiguous"),
        (dict(hit=3), "hit must be True, None or"),
        (dict(index=on(torch.zeros(100, dtype=torch.int64))), "index has dtype torch.int64, expected torch.int32"),
        (dict(index=on(torch.zeros(100, 1, dtype=i32))), "expected a vector of 100 elements"),
        (dict(sd=on(torch.zeros(100, dtype=torch.float32))), "sd has dtype torch.float32, expected torch.float64"),
        (dict(sd=torch.zeros(100, dtype=f64)), "is on cpu"),
        (dict(counts=on(torch.zeros(101, dtype=i32))), "expected a vector of 100 elements"),
        (dict(counts=on(torch.zeros(100, dtype=u8))), "counts has dtype torch.uint8, expected torch.int32"),
        (dict(cost=on(torch.zeros(100, dtype=torch.float32))), "always torch.float64"),
        (dict(cost=on(torch.zeros(100, dtype=f64), 1)), "the swarm lives on cuda:0"),
        (dict(cost=on(torch.zeros(200, dtype=f64)[::2])), "vector is not contiguous"),
        (dict(cost=on(torch.zeros(90, dtype=f64))), "expected a vector of 100 elements"),
        (dict(cost=[0.0] * 100), "cost must be a torch.float64"),
        (dict(cost=on(torch.zeros(100, dtype=f64)), hit_cost=float("nan")), "hit_cost must be finite"),
        (dict(cost=on(torch.zeros(100, dtype=f64)), hit_cost=float("inf")), "hit_cost must be finite"),
        (dict(margin=-0.5), "margin must be a finite number >= 0"),
        (dict(margin=float("nan")), "margin must be a finite number >= 0"),
        (dict(margin=float("inf")), "margin must be a finite number >= 0"),
        (dict(margin="wide"), "margin must be a finite number >= 0"),
        (dict(first=10, count=50, hit=on(torch.zeros(90, dtype=u8))), "expected a vector of 50 elements"),
        (dict(first=60, count=50), "do not fit a swarm of 100 UAVs"),
        (dict(first=-1, count=5), "do not fit a swarm of 100 UAVs"),
        (dict(hit=None), "nothing to do"),
        (dict(hit=False, index=None, crash=False), "nothing to do"),
    ]
    for kw, msg in cases:
        args = dict(hit=on(torch.zeros(kw.get("count", 100), dtype=u8)))
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            T.obstacle_contacts(g, **args)
    monkeypatch.setattr(T, "_stream", lambda dev: 1234)
    for kw in (dict(hit=on(torch.zeros(100, dtype=u8))), dict(crash=True), dict(cost=on(torch.zeros(100, dtype=f64)), hit_cost=5.0),
               dict(counts=on(torch.zeros(100, dtype=i32)), margin=0.25)):
        with pytest.raises(AssertionError, match="obstacle_contacts_device"):
            T.obstacle_contacts(g, **kw)
    calls = []

    class Taking(_Swarm):
        def obstacle_contacts_device(self, *a):
            calls.append(a)

    hit, index, sd, counts, cost = (on(torch.zeros(60, dtype=d)) for d in (u8, i32, f64, i32, f64))
    got = T.obstacle_contacts(Taking(), 0.25, True, 7, 60, hit, index, sd, counts, cost, 3.5)
    assert calls[-1] == (7, 60, 0.25, T.CONTACT_CRASH, hit.data_ptr(), index.data_ptr(), sd.data_ptr(), counts.data_ptr(), cost.data_ptr(), 3.5, 1234)
    assert all(a is b for a, b in zip(got, (hit, index, sd, counts)))
    got = T.obstacle_contacts(Taking(), crash=True)  # the mark alone: no output, the whole swarm, margin 0
    assert calls[-1] == (0, 100, 0.0, T.CONTACT_CRASH, 0, 0, 0, 0, 0, 0.0, 1234) and got == (None, None, None, None)
    got = T.obstacle_contacts(Taking(), counts=on(torch.zeros(100, dtype=i32)), hit_cost=float("nan"))  # (hit_cost without cost is not looked at)
    assert calls[-1][3] == 0 and calls[-1][4:7] == (0, 0, 0) and calls[-1][7] != 0 and calls[-1][8:10] == (0, 0.0) and got[3] is not None
    n_calls = len(calls)
    assert T.obstacle_contacts(Taking(), first=100, count=0, crash=True) == (None, None, None, None) and len(calls) == n_calls  # nothing to ask


# ---- tests: the C++ programs ----

_math_exe = []


def build_math_test():
    """tests/cpp/obstacle_contact_math_test.cpp: the host compiler, no contraction, address and undefined-behaviour sanitizers"""
    if not _math_exe:
        exe = os.path.join(ROOT, "tests", "cpp", "obstacle_contact_math_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "obstacle_contact_math_test.cpp"), "-o", exe])
        _math_exe.append(exe)
    return _math_exe[0]


def listed_points():
    """the points the sanitizer program is asked about: (pos [n, 3], worlds [n], rad [n], margin, obstacles) — a slice of the fixture with
    its airframes, and hand-placed x500s at the exact thresholds of all three kinds, on surfaces, inside overlaps, far away and not finite"""
    pos, worlds, ob = fixture_scene()
    sel = np.r_[0:96, 190:210, 1000:1100, 2040:2140, 3000:3072]
    rad = body_radius("x500")
    extra_ob = obstacles([(SPHERE, (100.0, 0.0, 0.0), (1.0, 0, 0), 0, ALL_WORLDS), (BOX, (120.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0, ALL_WORLDS),
                          (CYLINDER, (140.0, 0.0, 0.0), (1.0, 0, np.inf), 0, ALL_WORLDS), (BOX, (122.0, 0.0, 0.0), (1.0, 1.0, 1.0), 5)])
    margin = float(np.float64(0.75) - rad)  # thr = 0.75: the first two points of each kind are exactly at thr and one ulp inside
    at = 1.0 + (rad + np.float64(margin))
    assert at == 1.75
    hand = []
    for cx in (100.0, 120.0, 140.0):
        hand += [[cx + at, 0.0, 0.0], [cx + np.nextafter(at, 0.0), 0.0, 0.0], [cx + 1.0, 0.0, 0.0], [cx, 0.25, 0.5]]
    hand += [[121.0, 0.0, 0.0], [140.5, 0.0, 1e30], [1e9, -1e9, 1e7], [-5000.0, 0.0, 3.0], [np.nan, 0.0, 0.0], [100.0, np.inf, 0.0], [100.0, 0.0, -np.inf]]
    hand = np.array(hand)
    p = np.concatenate([pos[sel], hand])
    w = np.concatenate([worlds[sel], np.where(np.arange(len(hand)) % 2 == 0, 0, 5)]).astype(np.int32)
    r = np.concatenate([fixture_radii(len(pos))[sel], np.full(len(hand), rad)])
    return p, w, r, margin, np.concatenate([ob, extra_ob])


def test_fold_over_the_cell_walk_under_sanitizers():
    """random sets with huge boxes, pillars without ends, far points and per-point thresholds <= R against brute force, inside the program;
    then the listed points: the program's results equal the numpy restatement's bits"""
    p, w, rad, margin, ob = listed_points()
    res = restate_contacts(p, w, ob, rad, margin)
    assert res["hit"].sum() > 60 and (res["count"] > 1).sum() > 10 and (res["hit"] == 0).sum() > 100
    n = len(p)
    with tempfile.TemporaryDirectory() as d:
        set_path, pts_path, out_path = (os.path.join(d, f) for f in ("set.bin", "points.bin", "out.bin"))
        np.ascontiguousarray(ob, OBSTACLE).tofile(set_path)
        rows = np.zeros(n, np.dtype([("p", "f8", 3), ("thr", "f8"), ("world", "u4"), ("pad", "u4")]))
        rows["p"], rows["thr"], rows["world"] = p, res["thr"], w.astype(np.uint32)
        rows.tofile(pts_path)
        out = subprocess.run([build_math_test(), set_path, pts_path, out_path], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("functions", "random", "coarsened", "listed", "all"):
            assert f"ok {tag}" in out.stdout, out.stdout
        assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
        got = np.fromfile(out_path, np.dtype([("sd", "f8"), ("index", "i4"), ("count", "i4")]))
    assert len(got) == n
    assert np.array_equal(got["count"], res["count"]) and np.array_equal(got["index"], res["index"]) and same_bits(got["sd"], res["sd"])


def test_contact_test_compiles(mrs):
    """tests/cpp/obstacle_contact_test.cpp builds against the facade and the HIP runtime (run on the GPU by test_obstacle_contacts_gpu.py)"""
    from test_device_io_gpu import build_cpp
    assert os.path.exists(build_cpp("obstacle_contact_test"))
