"""The line-of-sight neighbours without a GPU (mrs_swarm_nearest_visible_device): the numpy restatement of the contract that
test_nearest_visible_gpu.py compares the kernel with, its known answers, a geometric check of it that owes nothing to the ray formulas,
what the fixture scene holds, the pure functions of csrc/sight_math.h as a stand-alone program under the sanitizers, the ABI, the tensor
wrapper's refusals and the C++ facade's test program."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import abi_header, abi_prototype, fake_cuda, stand_in
from test_nearest import _d2, nearest_ref
from test_obstacles import ALL_WORLDS, BOX, CYLINDER, OBSTACLE, SPHERE, fixture_scene, obstacles, same_bits, signed_distances
from test_range_scan import ROOT, TYPES, gate, ray

NAME = "mrs_swarm_nearest_visible_device"
SCENE_RADIUS, SCENE_K = 6.0, 8
NO_OBSTACLES = np.zeros(0, OBSTACLE)


# ---- the numpy restatement (used by test_nearest_visible_gpu.py) ----

def sight_direction(dx, d2):
    """(d, u): d = sqrt(d2), u = dx / d, three separately rounded divisions"""
    with np.errstate(all="ignore"):
        d = np.sqrt(d2)
        return d, dx / d[:, None]


@np.errstate(all="ignore")
def hidden_pairs(pos, worlds, ob, pi, pj, d2, radius, chunk=20000):
    """[P] bool: is candidate pj[p] hidden from observer pi[p] — some obstacle that applies to the observer's world and passes gate(o, p_i,
    radius) has ray(o, p_i, u) < d, strictly; d2 == 0 is visible with no test"""
    hid = np.zeros(len(pi), bool)
    if len(ob) == 0 or len(pi) == 0:
        return hid
    obs, inv = np.unique(pi, return_inverse=True)
    A = gate(pos[obs], ob, radius) & (((ob["flags"] & ALL_WORLDS) != 0)[None, :] | (ob["world"][None, :] == worlds[obs][:, None]))
    for a in range(0, len(pi), chunk):
        sl = slice(a, min(a + chunk, len(pi)))
        d, u = sight_direction(pos[pj[sl]] - pos[pi[sl]], d2[sl])
        pp, oo = np.nonzero(A[inv[sl]])
        t = ray(pos[pi[sl]][pp], u[pp][:, None, :], ob[oo])[:, 0]
        hides = (t < d[pp]) & (d2[sl][pp] != 0.0)
        hid[a + pp[hides]] = True
    return hid


@np.errstate(all="ignore")
def restate_visible(pos, worlds, ob, first, count, k, radius, chunk=256):
    """The contract of mrs_swarm_nearest_visible_device for observers [first, first + count): a dict of index [count, k] (-1: empty), d2
    [count, k] (0: empty), counts, visible and hidden [count], and pairs = (pi, pj, d2, hid), every candidate pair of the range.
    Candidates as nearest (j != i, finite, equal label, d2 < radius * radius with _d2 of test_nearest.py); the first k visible ones by
    ascending (d2, j), the order of nearest_ref."""
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    worlds = np.zeros(n, np.int32) if worlds is None else np.asarray(worlds).astype(np.int32)
    rr = np.float64(radius) * np.float64(radius)
    fin = np.isfinite(pos).all(axis=1)
    pis, pjs, d2s = [], [], []
    for a in range(first, first + count, chunk):
        q = np.arange(a, min(a + chunk, first + count))
        d2 = _d2(pos[q][:, None, :], pos[None, :, :])
        cand = (d2 < rr) & (q[:, None] != np.arange(n)[None, :]) & fin[None, :] & fin[q][:, None] & (worlds[q][:, None] == worlds[None, :])
        r, j = np.nonzero(cand)
        pis.append(q[r]), pjs.append(j), d2s.append(d2[r, j])
    pi, pj, d2 = (np.concatenate(v) if v else np.zeros(0, t) for v, t in ((pis, np.int64), (pjs, np.int64), (d2s, np.float64)))
    hid = hidden_pairs(pos, worlds, ob, pi, pj, d2, radius)
    row = pi - first
    out = dict(index=np.full((count, k), -1, np.int64), d2=np.zeros((count, k)), pairs=(pi, pj, d2, hid),
               visible=np.bincount(row[~hid], minlength=count).astype(np.int64), hidden=np.bincount(row[hid], minlength=count).astype(np.int64))
    out["counts"] = np.minimum(out["visible"], k)
    vi, vj, vd = pi[~hid], pj[~hid], d2[~hid]
    o = np.lexsort((vj, vd, vi))  # (the order of nearest_ref)
    vi, vj, vd = vi[o], vj[o], vd[o]
    vrow = vi - first
    rank = np.arange(len(vrow)) - np.searchsorted(vrow, np.arange(count), "left")[vrow] if len(vrow) else np.zeros(0, np.int64)
    sel = rank < k
    out["index"][vrow[sel], rank[sel]] = vj[sel]
    out["d2"][vrow[sel], rank[sel]] = vd[sel]
    return out


_scene = {}


def scene_visible(k=SCENE_K, radius=SCENE_RADIUS):
    """the restatement of the fixture scene, computed once per (k, radius) and shared (never written to)"""
    if (k, radius) not in _scene:
        pos, worlds, ob = fixture_scene()
        res = restate_visible(pos, worlds, ob, 0, len(pos), k, radius)
        for a in list(res.values())[:2] + list(res["pairs"]) + [res["visible"], res["hidden"], res["counts"]]:
            a.setflags(write=False)
        _scene[(k, radius)] = res
    return _scene[(k, radius)]


# ---- tests: the restatement ----

def sees(p, q, ob, radius=10.0, worlds=None, more=()):
    """does the UAV at p see the one at q (a swarm of these two and `more`)"""
    pos = np.array([p, q] + list(more), np.float64)
    res = restate_visible(pos, worlds, ob, 0, 1, 4, radius)
    assert res["visible"][0] + res["hidden"][0] == len(pos) - 1 or worlds is not None
    return 1 in res["index"][0]


def test_restatement_known_answers():
    O = (0.0, 0.0, 0.0)
    box = obstacles([(BOX, (5.0, 0, 0), (1.0, 1.0, 1.0))])
    assert sees(O, (4.0, 0, 0), box)  # t == d == 4: on the surface
    assert not sees(O, (np.nextafter(4.0, 5.0), 0, 0), box)
    assert sees(O, (3.0, 0, 0), box) and not sees(O, (7.0, 0, 0), box) and sees(O, (0, 7.0, 0), box) and sees(O, (-7.0, 0, 0), box)
    sph = obstacles([(SPHERE, (5.0, 0, 0), (1.0, 0, 0))])  # t = 24 / (5 + 1) = 4
    assert sees(O, (4.0, 0, 0), sph) and not sees(O, (np.nextafter(4.0, 5.0), 0, 0), sph) and not sees(O, (8.0, 0, 0), sph)
    assert sees(O, (8.0, 2.0, 0), sph)  # passes beside it
    pil = obstacles([(CYLINDER, (5.0, 0, 100.0), (1.0, 0, np.inf))])  # a pillar: no ends, whatever its centre's height
    assert sees(O, (4.0, 0, 0), pil) and not sees(O, (np.nextafter(4.0, 5.0), 0, 0), pil) and not sees((0, 0, -50.0), (8.0, 0, -50.0), pil)
    assert sees(O, (0, 0, 9.0), pil)
    cyl = obstacles([(CYLINDER, (5.0, 0, 0), (1.0, 0, 2.0))])
    assert not sees(O, (8.0, 0, 0), cyl) and sees((0, 0, 2.5), (8.0, 0, 2.5), cyl)  # over the top
    # inside a solid: a coincident pair sees each other, anything else is hidden (t == 0 < d)
    inside = (5.25, 0.5, -0.5)
    assert sees(inside, inside, box) and not sees(inside, (9.0, 0, 0), box) and not sees(inside, (5.5, 0.5, -0.5), box)
    assert not sees(O, inside, box)  # and a target inside is hidden from outside
    # worlds: an obstacle of another world hides nothing, an ALL_WORLDS one hides in every world
    w5 = obstacles([(BOX, (5.0, 0, 0), (1.0, 1.0, 1.0), 5)])
    aw = obstacles([(BOX, (5.0, 0, 0), (1.0, 1.0, 1.0), 77, ALL_WORLDS)])
    assert sees(O, (7.0, 0, 0), w5) and not sees(O, (7.0, 0, 0), w5, worlds=[5, 5]) and not sees(O, (7.0, 0, 0), aw)
    assert not sees(O, (7.0, 0, 0), aw, worlds=[5, 5]) and not sees(O, (3.0, 0, 0), NO_OBSTACLES, worlds=[0, 5])
    # the gate is part of the contract: a wall further than the radius on an axis hides nothing (no target within the radius is behind it)
    assert sees(O, (3.9, 0, 0), box, radius=3.95)
    # selection: the first k VISIBLE by (d2, j); hidden ones take no slot and are counted, uncapped
    pos = np.array([O, (7.0, 0, 0), (0, 3.0, 0), (0, -3.0, 0), (6.5, 0, 0), (0, 0, 2.0), (0, 0, 2.0)], np.float64)
    res = restate_visible(pos, None, box, 0, 1, 2, 10.0)
    assert list(res["index"][0]) == [5, 6] and res["visible"][0] == 4 and res["hidden"][0] == 2 and res["counts"][0] == 2
    res = restate_visible(pos, None, box, 0, 7, 6, 10.0)
    assert list(res["index"][0]) == [5, 6, 2, 3, -1, -1] and list(res["d2"][0]) == [4.0, 4.0, 9.0, 9.0, 0.0, 0.0]
    assert list(res["index"][5][:1]) == [6] and res["d2"][5][0] == 0.0 and res["counts"][5] == 4 and res["hidden"][5] == 2
    nan = pos.copy()
    nan[0, 1] = np.nan
    res = restate_visible(nan, None, box, 0, 2, 2, 10.0)
    assert res["counts"][0] == 0 and res["hidden"][0] == 0 and 0 not in res["index"][1]


def test_restatement_without_obstacles_is_nearest():
    pos, worlds, ob = fixture_scene()
    for k in (1, 8, 32):
        got = restate_visible(pos, None, NO_OBSTACLES, 100, 400, k, SCENE_RADIUS)
        idx, cnt, dd = nearest_ref(pos, 100, 400, k, SCENE_RADIUS)
        assert np.array_equal(got["index"], idx) and np.array_equal(got["counts"], cnt) and same_bits(got["d2"], dd)
        assert not got["hidden"].any() and (got["visible"] >= cnt).all()
    far = ob.copy()
    far["c"] = far["c"] + 1000.0
    got = restate_visible(pos, worlds, far, 0, 300, 8, SCENE_RADIUS)
    none = restate_visible(pos, worlds, NO_OBSTACLES, 0, 300, 8, SCENE_RADIUS)
    assert np.array_equal(got["index"], none["index"]) and not got["hidden"].any()


def test_fixture_scene_conditions():
    """what the fixture scene must hold at 6 m and k = 8 for the GPU comparison to mean something (measured: 0.349, 1895, 394, 1398, 53)"""
    pos, worlds, ob = fixture_scene()
    res = scene_visible()
    pi, pj, d2, hid = res["pairs"]
    plain = restate_visible(pos, worlds, NO_OBSTACLES, 0, len(pos), SCENE_K, SCENE_RADIUS)
    differ = (plain["index"] != res["index"]).any(axis=1).sum()
    blind = ((res["hidden"] > 0) & (res["visible"] == 0)).sum()
    print("hidden share", hid.mean(), "rows that differ", differ, "blind", blind, "visible > k", (res["visible"] > SCENE_K).sum(),
          "largest hidden", res["hidden"].max())
    assert 0.2 < hid.mean() < 0.5
    assert differ >= 1000
    assert blind >= 300
    assert (res["visible"] > SCENE_K).sum() >= 1000
    assert res["hidden"].max() > 32
    assert res["counts"][200] == 0 and res["counts"][201] == 0 and not np.isin([200, 201], res["index"]).any()


def test_geometric_check_independent_of_the_ray_formulas():
    """Sight lines of the fixture scene no longer than 4 m, of every 32nd observer, sampled at 2049 points (step <= 1.96 mm, both ends
    included) against the signed distances of test_obstacles.py for the obstacles that apply to the observer and pass its gate: a
    sample with sd < -1e-6 implies hidden; hidden implies a sample with sd < +1e-3 (the line enters a solid at some t_e < d, the nearest
    sample is within half a step of that surface point, and sd is 1-Lipschitz)."""
    pos, worlds, ob = fixture_scene()
    pi, pj, d2, hid = scene_visible()["pairs"]
    keep = np.flatnonzero((pi % 32 == 0) & (d2 <= 16.0) & (d2 > 0))
    pi, pj, hid = pi[keep], pj[keep], hid[keep]
    assert len(pi) > 300 and hid.sum() > 60 and (~hid).sum() > 60
    A = gate(pos[pi], ob, SCENE_RADIUS) & (((ob["flags"] & ALL_WORLDS) != 0)[None, :] | (ob["world"][None, :] == worlds[pi][:, None]))
    frac = np.arange(2049) / 2048.0
    lowest = np.full(len(pi), np.inf)
    for o in range(len(ob)):
        pp = np.flatnonzero(A[:, o])
        if not len(pp):
            continue
        pts = pos[pi[pp]][:, None, :] + frac[None, :, None] * (pos[pj[pp]] - pos[pi[pp]])[:, None, :]
        sd = signed_distances(pts.reshape(-1, 3), ob[o:o + 1])[0].reshape(len(pp), -1).min(axis=1)
        lowest[pp] = np.minimum(lowest[pp], sd)
    assert hid[lowest < -1e-6].all(), np.flatnonzero(~hid & (lowest < -1e-6))[:5]
    assert (lowest[hid] < 1e-3).all(), lowest[hid].max()
    assert (lowest < -1e-6).sum() > 60


# ---- tests: the pure functions of csrc/sight_math.h, stand-alone under the sanitizers ----

CASE = np.dtype([("o", OBSTACLE), ("p", "f8", 3), ("q", "f8", 3), ("radius", "f8"), ("d2a", "f8"), ("d2b", "f8"), ("ja", "i4"), ("jb", "i4"),
                 ("pad", "f8")])
_math_exe = []


def build_math_test():
    """tests/cpp/sight_math_test.cpp: the host compiler, no contraction, address and undefined-behaviour sanitizers (the command of
    test_range_scan.build_math_test)"""
    if not _math_exe:
        exe = os.path.join(ROOT, "tests", "cpp", "sight_math_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "sight_math_test.cpp"), "-o", exe])
        _math_exe.append(exe)
    return _math_exe[0]


def test_pure_functions_equal_the_restatement_bit_for_bit():
    assert CASE.itemsize == 152
    pos, worlds, ob = fixture_scene()
    pi, pj, d2, hid = scene_visible()["pairs"]
    rng = np.random.default_rng(17)
    # (observer, target) pairs of the scene, each with three obstacles: two of those nearest to the sight line's midpoint, one arbitrary
    pick = rng.choice(len(pi), 8000, replace=False)
    mid = 0.5 * (pos[pi[pick]] + pos[pj[pick]])
    near = np.argsort(((mid[:, None, :] - np.nan_to_num(ob["c"], posinf=0.0)[None]) ** 2)[..., :2].sum(axis=-1), axis=1)[:, :2]
    oo = np.concatenate([near[:, 0], near[:, 1], rng.integers(0, len(ob), len(pick))])
    c = np.zeros(3 * len(pick), CASE)
    c["o"], c["p"], c["q"], c["radius"] = ob[oo], np.tile(pos[pi[pick]], (3, 1)), np.tile(pos[pj[pick]], (3, 1)), SCENE_RADIUS
    vals = np.array([0.0, 1.5, 1.5, 2.0, 36.0, np.inf])
    c["d2a"], c["d2b"] = vals[rng.integers(0, len(vals), len(c))], vals[rng.integers(0, len(vals), len(c))]
    c["ja"], c["jb"] = rng.integers(0, 5, len(c)), rng.integers(0, 5, len(c))
    c["jb"][::9] = 0x7FFFFFFF
    box, sph = obstacles([(BOX, (5.0, 0, 0), (1.0, 1.0, 1.0))])[0], obstacles([(SPHERE, (5.0, 0, 0), (1.0, 0, 0))])[0]
    pil = obstacles([(CYLINDER, (5.0, 0, 100.0), (1.0, 0, np.inf))])[0]
    exact = [(o, (0, 0, 0), (x, 0, 0), 10.0) for o in (box, sph, pil) for x in (4.0, np.nextafter(4.0, 5.0))]
    exact += [(box, (5.25, 0.5, -0.5), (9.0, 0, 0), 10.0), (box, (0, 0, 0), (3.9, 0, 0), 3.95), (box, (0, 0, 0), (np.nan, 0, 0), 10.0)]
    ex = np.zeros(len(exact), CASE)
    for k, (o, p, q, rad) in enumerate(exact):
        ex[k]["o"], ex[k]["p"], ex[k]["q"], ex[k]["radius"] = o, p, q, rad
    cases = np.concatenate([c, ex])
    assert len(cases) >= 20000
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cases.bin")
        cases.tofile(path)
        out = subprocess.run([build_math_test(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and f"ok {len(cases)} cases" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines()[:len(cases)]]
    got = np.array([[int(v, 16) for v in row[:5]] for row in rows], np.uint64).view(np.float64)
    with np.errstate(all="ignore"):
        dx = cases["q"] - cases["p"]
        want_d2 = _d2(cases["p"], cases["q"])
        want_d, want_u = sight_direction(dx, want_d2)
        assert same_bits(got[:, 0], want_d2) and same_bits(got[:, 1], want_d) and same_bits(got[:, 2:], want_u)
        want_g = np.array([gate(cases["p"][k:k + 1], cases["o"][k:k + 1], cases["radius"][k])[0, 0] for k in range(len(cases))])
        t = ray(cases["p"], want_u[:, None, :], cases["o"])[:, 0]
        want_h = want_g & (t < want_d)
        want_b = (cases["d2a"] < cases["d2b"]) | ((cases["d2a"] == cases["d2b"]) & (cases["ja"] < cases["jb"]))
    assert np.array_equal(np.array([int(row[5]) for row in rows]), want_g.astype(int))
    assert np.array_equal(np.array([int(row[6]) for row in rows]), want_h.astype(int))
    assert np.array_equal(np.array([int(row[7]) for row in rows]), want_b.astype(int))
    assert list(want_h[-9:]) == [False, True, False, True, False, True, True, False, False]
    kinds = cases["o"]["kind"]
    for kd in (SPHERE, BOX, CYLINDER):  # all three kinds among the hiding obstacles and among the gate-passers that do not hide
        assert (want_h & (kinds == kd)).sum() > 100 and (want_g & ~want_h & (kinds == kd)).sum() > 100, kd
    assert (~want_g).sum() > 1000 and (want_b & (cases["d2a"] == cases["d2b"])).sum() > 100 and (~want_b & (cases["d2a"] == cases["d2b"])).sum() > 100


# ---- tests: the ABI ----

def test_symbol_is_declared_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import build, swarm, tensors
    L = C.CDLL(swarm.LIB_PATH)
    assert re.search(r"\bint\s+" + NAME + r"\(", abi_header())
    assert hasattr(L, NAME) and NAME in swarm.ABI_SYMBOLS
    assert callable(getattr(swarm.Swarm, "nearest_visible_device", None)) and callable(getattr(tensors, "nearest_visible", None))
    assert ("nearest_visible.hip", "off") in build.UNITS and {"sight_math.h", "nn_slot.h", "nn_hash.h", "range_scan_math.h"} <= set(build.DEPS)
    facade = open(os.path.join(ROOT, "include", "mrs_multirotor_simulator", "uav_system", "uav_system.hpp")).read()
    assert re.search(r"\bnearestVisibleDevice\(", facade)
    csrc = os.path.join(ROOT, "mrs_multirotor_simulator_amd", "csrc")
    nearest = open(os.path.join(csrc, "nearest.hip")).read()
    assert "void write_slot(" not in nearest and "void write_slot(" in open(os.path.join(csrc, "nn_slot.h")).read()  # one definition


def test_header_prototype_argtypes_and_method_agree(mrs):
    from mrs_multirotor_simulator_amd import swarm
    L = swarm.load_library()
    names = ["s", "first", "count", "k", "radius", "fields", "dev_rows", "dtype", "stride", "dev_index", "index_stride", "dev_count",
             "dev_visible", "dev_hidden", "ext_stream"]
    got_names, types = abi_prototype(NAME)
    assert got_names == names
    got = [C.c_void_p if issubclass(a, C._Pointer) else a for a in getattr(L, NAME).argtypes]
    assert [TYPES[t] for t in types] == got, types
    assert list(inspect.signature(swarm.Swarm.nearest_visible_device).parameters) == ["self"] + names[1:]
    near_names, near_types = abi_prototype("mrs_swarm_nearest_device")  # the arguments of nearest, two vectors more
    assert names[:12] == near_names[:12] and types[:12] == near_types[:12] and types[12:14] == ["int32_t*", "int32_t*"]


# ---- tests: the tensor layer without a GPU ----

def test_nearest_visible_refuses_before_the_library(mrs, monkeypatch):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, i32 = stand_in("nearest_visible_device", "nearest_device")(), torch.int32
    cases = [
        (dict(out=torch.zeros(100, 32)), "is on cpu"),
        (dict(out=on(torch.zeros(100, 32), 1)), "the swarm lives on cuda:0"),
        (dict(out=on(torch.zeros(100, 31))), r"expected a \[100, >= 32\] matrix"),
        (dict(out=on(torch.zeros(100, 32, dtype=torch.float16))), "dtype must be torch.float32 or torch.float64"),
        (dict(out=on(torch.zeros(100, 64)[:, ::2])), "rows are not contiguous"),
        (dict(index=on(torch.zeros(100, 7, dtype=i32))), r"expected a \[100, >= 8\] matrix"),
        (dict(index=on(torch.zeros(100, 8, dtype=torch.int64))), "expected torch.int32"),
        (dict(counts=on(torch.zeros(99, dtype=i32))), "100"),
        (dict(counts=on(torch.zeros(100, dtype=torch.int64))), "counts has dtype"),
        (dict(visible=on(torch.zeros(100, dtype=torch.int64))), "visible has dtype"),
        (dict(visible=torch.zeros(100, dtype=i32)), "is on cpu"),
        (dict(visible=3), "visible must be True, None or a"),
        (dict(hidden=on(torch.zeros(99, dtype=i32))), "100"),
        (dict(hidden=on(torch.zeros(100, dtype=i32), 1)), "the swarm lives on cuda:0"),
        (dict(hidden="all"), "hidden must be True, None or a"),
        (dict(first=10, count=50, hidden=on(torch.zeros(90, dtype=i32))), "50"),
        (dict(first=60, count=50), "do not fit a swarm of 100"),
    ]
    for kw, msg in cases:
        args = dict(out=on(torch.zeros(100, 32)), index=on(torch.zeros(100, 8, dtype=i32)), counts=on(torch.zeros(100, dtype=i32)),
                    visible=on(torch.zeros(100, dtype=i32)), hidden=on(torch.zeros(100, dtype=i32)))
        if "count" in kw:
            c = kw["count"]
            args = dict(out=on(torch.zeros(c, 32)), index=on(torch.zeros(c, 8, dtype=i32)), counts=on(torch.zeros(c, dtype=i32)),
                        visible=on(torch.zeros(c, dtype=i32)), hidden=on(torch.zeros(c, dtype=i32)))
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            T.nearest_visible(g, 8, 5.0, **args)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "far"):
        with pytest.raises(ValueError, match="radius must be a finite number > 0"):
            T.nearest_visible(g, 8, bad, out=on(torch.zeros(100, 32)))
    with pytest.raises(ValueError, match="nothing to do"):
        T.nearest_visible(g, 8, 5.0, fields=0, index=False, counts=False, visible=None, hidden=None)
    with pytest.raises(mrs.MrsError, match="k must be in"):  # (mrs_nearest_width: host only, no GPU)
        T.nearest_visible(g, 33, 5.0, out=on(torch.zeros(100, 200)))
    monkeypatch.setattr(T, "_stream", lambda dev: 1234)
    full = dict(out=on(torch.zeros(100, 32)), index=on(torch.zeros(100, 8, dtype=i32)), counts=on(torch.zeros(100, dtype=i32)),
                visible=on(torch.zeros(100, dtype=i32)), hidden=on(torch.zeros(100, dtype=i32)))
    with pytest.raises(AssertionError, match="nearest_visible_device"):
        T.nearest_visible(g, 8, np.float32(5.0), **full)
    calls = []

    class Taking(stand_in("nearest_device")):
        def nearest_visible_device(self, *a):
            calls.append(a)

    out, index = on(torch.zeros(60, 140, dtype=torch.float64)), on(torch.zeros(60, 11, dtype=i32))
    counts, visible, hidden = (on(torch.zeros(60, dtype=i32)) for _ in range(3))
    r, ix, c, v, h = T.nearest_visible(Taking(), 8, 12.5, fields=T.NN_ALL, first=7, count=60, out=out, index=index, counts=counts, visible=visible,
                                       hidden=hidden)
    assert calls[-1] == (7, 60, 8, 12.5, T.NN_ALL, out.data_ptr(), T.DTYPE_F64, 140, index.data_ptr(), 11, counts.data_ptr(), visible.data_ptr(),
                         hidden.data_ptr(), 1234)
    assert r.shape == (60, 104) and ix.shape == (60, 8) and c is counts and v is visible and h is hidden
    r, ix, c, v, h = T.nearest_visible(Taking(), 8, 3.0, fields=0, index=False, counts=counts[:60], visible=None, hidden=None, count=60)
    assert r is None and ix is None and v is None and h is None and calls[-1][4:10] == (0, 0, T.DTYPE_F32, 0, 0, 0) and calls[-1][11:13] == (0, 0)


def test_nearest_visible_test_compiles(mrs):
    """tests/cpp/nearest_visible_test.cpp builds against the facade and the HIP runtime (run on the GPU by test_nearest_visible_gpu.py)"""
    from test_device_io_gpu import build_cpp
    assert os.path.exists(build_cpp("nearest_visible_test"))
