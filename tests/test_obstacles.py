"""CPU-side checks of the static obstacles (include/mrs_swarm.h, "static obstacles"): the numpy restatement the GPU tests compare bits
against (restate_obstacles below) is checked on its own with known answers; the fixture scene of the GPU tests is built here and the
restatement alone asserts its coverage; the symbols are exported and listed, header prototypes, ctypes argtypes and method signatures
agree, the header's values are the Python ones; the tensor wrappers refuse bad arguments before the library is reached and hand strides
through; and the host-side grid builder (csrc/obstacle_grid.h) passes tests/cpp/obstacle_grid_test.cpp under the address and
undefined-behaviour sanitizers.  No pointer reaches the library."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import CTYPE, abi_header, abi_prototype, fake_cuda, stand_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERE, BOX, CYLINDER = 0, 1, 2
ALL_WORLDS = 1
ON_REL, ON_REL_BODY, ON_DIST = 1, 2, 4
HINGE2, INVERSE, COUNT = 0, 1, 2
OBSTACLE = np.dtype([("kind", "i4"), ("world", "i4"), ("flags", "u4"), ("reserved", "u4"), ("c", "f8", 3), ("h", "f8", 3)])
TYPES = dict(CTYPE, **{"double*": C.c_void_p, "int32_t*": C.c_void_p, "const mrs_obstacle_t*": C.c_void_p, "mrs_obstacle_t*": C.c_void_p,
                       "mrs_obstacle_stats_t*": C.c_void_p, "const mrs_swarm_t*": C.c_void_p})
FIXTURE_RADIUS = 3.0


# ---- the numpy restatement (used by test_obstacles_gpu.py) ----

def obstacles(rows):
    """an OBSTACLE array from (kind, centre, sizes[, world[, flags]]) tuples"""
    out = np.zeros(len(rows), OBSTACLE)
    for j, row in enumerate(rows):
        out[j]["kind"], out[j]["c"], out[j]["h"] = row[0], row[1], row[2]
        out[j]["world"] = row[3] if len(row) > 3 else 0
        out[j]["flags"] = row[4] if len(row) > 4 else 0
    return out


def _mx(a, b):
    return np.where(a < b, b, a)


def _mn(a, b):
    return np.where(b < a, b, a)


@np.errstate(all="ignore")
def signed_distances(pos, obst):
    """(sd [n, M], rel [n, M, 3]) of every UAV against every obstacle: the stated arithmetic, every operation a separately rounded numpy
    FP64 one, the three kinds selected by where"""
    pos = np.asarray(pos, np.float64)
    d = pos[:, None, :] - obst["c"][None, :, :]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    h = obst["h"][None, :, :]
    zero = np.float64(0.0)
    # sphere
    r = h[..., 0]
    rho = np.sqrt(((dx * dx) + dy * dy) + dz * dz)
    sd_s = rho - r
    t = np.where(rho > r, r / rho - 1.0, zero)
    rel_s = np.stack([t * dx, t * dy, t * dz], -1)
    # box
    a = np.abs(d) - h
    m = _mx(a, zero)
    sd_b = np.sqrt(((m[..., 0] * m[..., 0]) + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]) + _mn(_mx(a[..., 0], _mx(a[..., 1], a[..., 2])), zero)
    rel_b = _mn(_mx(d, -h), h) - d
    # cylinder
    hz = h[..., 2]
    rho = np.sqrt((dx * dx) + dy * dy)
    ar, az = rho - r, np.abs(dz) - hz
    mr, mz = _mx(ar, zero), _mx(az, zero)
    sd_c = np.sqrt((mr * mr) + mz * mz) + _mn(_mx(ar, az), zero)
    t = np.where(rho > r, r / rho - 1.0, zero)
    rel_c = np.stack([t * dx, t * dy, _mn(_mx(dz, -hz), hz) - dz], -1)
    kind = obst["kind"][None, :]
    sd = np.where(kind == SPHERE, sd_s, np.where(kind == BOX, sd_b, sd_c))
    rel = np.where((kind == SPHERE)[..., None], rel_s, np.where((kind == BOX)[..., None], rel_b, rel_c))
    return sd, rel


@np.errstate(all="ignore")
def restate_obstacles(pos, R, worlds, obst, k, radius):
    """The contract of mrs_swarm_nearest_obstacles_device for every UAV: the obstacles that apply to it (ALL_WORLDS, or its label) with
    sd < radius, the first k by ascending (sd, obstacle index).  pos [n, 3]; R [n, 3, 3] or None (identity); worlds [n] or None (all 0).
    Returns a dict: found [n] (uncapped), count [n] = min(found, k), index [n, k] (-1: empty slot), sd [n, k], rel and rel_body
    [n, k, 3] (zeros in empty slots)."""
    pos = np.asarray(pos, np.float64)
    n, M = len(pos), len(obst)
    worlds = np.zeros(n, np.int32) if worlds is None else np.asarray(worlds).astype(np.int32)
    out = dict(found=np.zeros(n, np.int64), count=np.zeros(n, np.int64), index=np.full((n, k), -1, np.int64), sd=np.zeros((n, k)),
               rel=np.zeros((n, k, 3)), rel_body=np.zeros((n, k, 3)))
    if M == 0 or n == 0:
        return out
    sd, rel = signed_distances(pos, obst)
    applies = ((obst["flags"] & ALL_WORLDS) != 0)[None, :] | (obst["world"][None, :] == worlds[:, None])
    hit = applies & (sd < np.float64(radius)) & np.isfinite(pos).all(axis=1)[:, None]
    found = hit.sum(axis=1)
    order = np.argsort(np.where(hit, sd, np.inf), axis=1, kind="stable")[:, :k]  # ties (and -0.0 == +0.0) stay in index order
    kk = order.shape[1]
    live = np.arange(kk)[None, :] < np.minimum(found, k)[:, None]
    rows = np.arange(n)[:, None]
    out["found"], out["count"] = found, np.minimum(found, k)
    out["index"][:, :kk] = np.where(live, order, -1)
    out["sd"][:, :kk] = np.where(live, sd[rows, order], 0.0)
    v = np.where(live[..., None], rel[rows, order], 0.0)
    out["rel"][:, :kk] = v
    if R is None:
        R = np.broadcast_to(np.eye(3), (n, 3, 3))
    R = np.asarray(R, np.float64).reshape(n, 3, 3)
    body = np.stack([(R[:, None, 0, c] * v[..., 0] + R[:, None, 1, c] * v[..., 1]) + R[:, None, 2, c] * v[..., 2] for c in range(3)], -1)
    out["rel_body"][:, :kk] = np.where(live[..., None], body, 0.0)  # (an empty slot is +0.0, whatever R holds)
    return out


def restate_rows(res, fields, dtype=np.float64):
    """the [n, k * w] row block of `fields` from a restate_obstacles result: the fields of a slot concatenated in bit order"""
    parts = [res[name] if name != "sd" else res["sd"][..., None] for bit, name in ((ON_REL, "rel"), (ON_REL_BODY, "rel_body"), (ON_DIST, "sd"))
             if fields & bit]
    n, k = res["index"].shape
    if not parts:
        return np.zeros((n, 0), dtype)
    return np.concatenate(parts, axis=-1).reshape(n, -1).astype(dtype)


@np.errstate(all="ignore")
def restate_cost(res, k, radius, kind, weight):
    """term [n] of mrs_swarm_obstacle_cost_device from a restate_obstacles result of the same k: +0.0, then one FP64 addition per listed
    obstacle, nearest first"""
    n = len(res["found"])
    radius, weight = np.float64(radius), np.float64(weight)
    term = np.zeros(n)
    for m in range(k):
        if kind == HINGE2:
            g = radius - res["sd"][:, m]
            new = term + (weight * g) * g
        else:
            assert kind == COUNT
            new = term + weight
        term = np.where(m < res["count"], new, term)
    return term


def add_bits(c, term):
    """what the call leaves in dev_cost: c + term, one FP64 addition (c = +0.0 without accumulate)"""
    with np.errstate(all="ignore"):
        return (np.zeros_like(term) if c is None else np.asarray(c, np.float64)) + term


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32 or b.dtype == np.float32:
        return a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


# ---- the fixture scene of the GPU tests ----

_fixture = []


def fixture_scene():
    """(pos [n, 3], worlds [n], obstacles [M]) with n = 3072 <= 4096 UAVs and M = 384 <= 512 obstacles over a 60 x 60 x 20 m volume: a
    third of the obstacles in world 0, a third in world 5, a third ALL_WORLDS; UAVs labelled 0 or 5; a dense cluster of 40 overlapping
    all-worlds obstacles with 64 UAVs in it (found > 32); UAVs at the centres of obstacles of every kind; two non-finite UAVs.  Built
    once and never written to."""
    if _fixture:
        return _fixture[0]
    rng = np.random.default_rng(2024)
    n, M = 3072, 384
    kind = np.arange(M) % 3
    c = np.stack([rng.uniform(-30, 30, M), rng.uniform(-30, 30, M), rng.uniform(0, 20, M)], axis=1)
    h = rng.uniform(0.3, 2.5, (M, 3))
    h[(kind == CYLINDER) & (np.arange(M) % 2 == 0), 2] = np.inf  # every other cylinder is a pillar without ends
    ob = np.zeros(M, OBSTACLE)
    ob["kind"], ob["c"], ob["h"] = kind, c, h
    group = (np.arange(M) // 3) % 3
    ob["world"] = np.where(group == 1, 5, 0)
    ob["flags"] = np.where(group == 2, ALL_WORLDS, 0)
    ob["world"][group == 2] = 77  # (ignored under ALL_WORLDS)
    cl = slice(M - 40, M)  # the cluster: 40 all-worlds obstacles of all kinds within 1.5 m of (12, -9, 6)
    ob["c"][cl] = np.array([12.0, -9.0, 6.0]) + rng.uniform(-1.5, 1.5, (40, 3))
    ob["flags"][cl] = ALL_WORLDS
    pos = np.stack([rng.uniform(-33, 33, n), rng.uniform(-33, 33, n), rng.uniform(-2, 22, n)], axis=1)
    pos[:64] = np.array([12.0, -9.0, 6.0]) + rng.uniform(-2.0, 2.0, (64, 3))
    pos[64:64 + 90] = ob["c"][:90] + rng.uniform(-0.1, 0.1, (90, 3))  # inside obstacles of every kind and world
    worlds = np.where(rng.uniform(size=n) < 0.5, 0, 5).astype(np.int32)
    pos[200] = [np.nan, 1.0, 2.0]
    pos[201] = [3.0, 4.0, np.inf]
    for a in (pos, worlds, ob):
        a.setflags(write=False)
    _fixture.append((pos, worlds, ob))
    return _fixture[0]


def grid_of(obst, radius):
    """what csrc/obstacle_grid.h builds for a set and a radius, from tests/cpp/obstacle_grid_test.cpp: dict of dims, cells, items, longest, edge"""
    exe = build_grid_test()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "set.bin")
        np.ascontiguousarray(obst, OBSTACLE).tofile(path)
        out = subprocess.run([exe, path, repr(float(radius))], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"grid dims (\d+) (\d+) (\d+) cells (\d+) items (\d+) longest (\d+) edge (\S+)", out.stdout)
    assert m, out.stdout
    return dict(dims=tuple(int(m.group(i)) for i in (1, 2, 3)), cells=int(m.group(4)), items=int(m.group(5)), longest=int(m.group(6)),
                edge=float(m.group(7)))


_grid_exe = []


def build_grid_test():
    """tests/cpp/obstacle_grid_test.cpp: the host compiler, no contraction, address and undefined-behaviour sanitizers"""
    if not _grid_exe:
        exe = os.path.join(ROOT, "tests", "cpp", "obstacle_grid_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "obstacle_grid_test.cpp"), "-o", exe])
        _grid_exe.append(exe)
    return _grid_exe[0]


# ---- tests: the restatement ----

def one(p, ob, k=4, radius=2.0, worlds=None, R=None):
    return restate_obstacles(np.atleast_2d(np.asarray(p, np.float64)), R, worlds, ob, k, radius)


def test_restatement_known_answers_per_kind():
    inf = np.inf
    sph = obstacles([(SPHERE, (1.0, 2.0, 3.0), (1.0, 0, 0))])
    # outside: 3-4-5 triangle from the centre; sd = 5 - 1, t = 1/5 - 1
    r = one((4.0, 2.0, 7.0), sph, radius=4.5)
    t = 1.0 / 5.0 - 1.0
    assert r["found"][0] == 1 and r["index"][0, 0] == 0 and r["sd"][0, 0] == 4.0 and same_bits(r["rel"][0, 0], [t * 3.0, t * 0.0, t * 4.0])
    assert np.allclose(np.array([4.0, 2.0, 7.0]) + r["rel"][0, 0], [1.6, 2.0, 3.8], atol=1e-15)  # the closest point of the sphere
    r = one((2.0, 2.0, 3.0), sph)  # on the surface: sd 0, rel 0 (rho > r is false)
    assert r["sd"][0, 0] == 0.0 and same_bits(r["rel"][0, 0], [0.0, 0.0, 0.0])
    r = one((1.25, 2.0, 3.0), sph)  # inside
    assert r["sd"][0, 0] == -0.75 and same_bits(r["rel"][0, 0], [0.0, 0.0, 0.0])
    box = obstacles([(BOX, (0.0, 0.0, 0.0), (1.0, 2.0, 3.0))])
    r = one((4.0, 0.5, 7.0), box, radius=6.0)  # outside, beyond two faces: sqrt(3^2 + 4^2)
    assert r["sd"][0, 0] == 5.0 and same_bits(r["rel"][0, 0], [-3.0, 0.0, -4.0])
    r = one((-1.0, 0.5, 0.0), box)  # on a face
    assert r["sd"][0, 0] == 0.0 and same_bits(r["rel"][0, 0], [0.0, 0.0, 0.0])
    r = one((0.25, 0.5, -1.0), box)  # inside: the nearest face is x (0.75 away)
    assert r["sd"][0, 0] == -0.75 and same_bits(r["rel"][0, 0], [0.0, 0.0, 0.0])
    cyl = obstacles([(CYLINDER, (0.0, 0.0, 1.0), (1.0, 0, 2.0))])
    r = one((4.0, 0.0, 7.0), cyl, radius=6.0)  # beyond the rim: sqrt(3^2 + 4^2)
    assert r["sd"][0, 0] == 5.0 and same_bits(r["rel"][0, 0], [(1.0 / 4.0 - 1.0) * 4.0, (1.0 / 4.0 - 1.0) * 0.0, -4.0])
    r = one((0.0, 3.0, 1.5), cyl, radius=6.0)  # beside the wall
    assert r["sd"][0, 0] == 2.0 and same_bits(r["rel"][0, 0], [(1.0 / 3.0 - 1.0) * 0.0, (1.0 / 3.0 - 1.0) * 3.0, 0.0])
    r = one((0.0, 0.5, 5.0), cyl, radius=6.0)  # above the cap
    assert r["sd"][0, 0] == 2.0 and same_bits(r["rel"][0, 0], [0.0, 0.0, -2.0])
    r = one((1.0, 0.0, 1.0), cyl)  # on the wall
    assert r["sd"][0, 0] == 0.0 and same_bits(r["rel"][0, 0], [0.0, 0.0, 0.0])
    r = one((0.5, 0.0, 2.5), cyl)  # inside: both the wall and the cap are 0.5 away
    assert r["sd"][0, 0] == -0.5 and same_bits(r["rel"][0, 0], [0.0, 0.0, 0.0])
    pillar = obstacles([(CYLINDER, (0.0, 0.0, 0.0), (1.0, 0, inf))])
    for z in (-1e30, -7.0, 0.0, 1e30):
        r = one((0.0, 3.0, z), pillar, radius=2.5)
        assert r["found"][0] == 1 and r["sd"][0, 0] == 2.0 and same_bits(r["rel"][0, 0], [(1.0 / 3.0 - 1.0) * 0.0, (1.0 / 3.0 - 1.0) * 3.0, 0.0]), z
        assert one((0.25, 0.0, z), pillar)["sd"][0, 0] == -0.75
    # the body frame: R^T rel, a quarter turn about z
    R = np.array([[[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]])
    r = one((4.0, 0.5, 7.0), box, radius=6.0, R=R)
    assert same_bits(r["rel_body"][0, 0], [(0.0 * -3.0 + 1.0 * 0.0) + 0.0 * -4.0, (-1.0 * -3.0 + 0.0 * 0.0) + 0.0 * -4.0, -4.0])
    # rows: bit order, FP32 as the cast
    assert same_bits(restate_rows(r, ON_DIST | ON_REL)[0, :4], list(r["rel"][0, 0]) + [5.0])
    assert restate_rows(r, ON_REL_BODY | ON_DIST, np.float32).dtype == np.float32 and restate_rows(r, 0).shape == (1, 0)
    assert restate_rows(r, 7).shape == (1, 4 * 7) and (restate_rows(r, 7)[0, 7:] == 0).all() and (r["index"][0] == [0, -1, -1, -1]).all()


def test_restatement_threshold_ties_and_order():
    # a UAV at exactly sd == radius is excluded, one nextafter closer is included (all three kinds; the numbers are exact)
    sets = [obstacles([(SPHERE, (0.0, 0.0, 0.0), (1.0, 0, 0))]), obstacles([(BOX, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))]),
            obstacles([(CYLINDER, (0.0, 0.0, 0.0), (1.0, 0, np.inf))])]
    for ob in sets:
        at, closer = 3.5, np.nextafter(3.5, 0.0)
        assert one((at, 0.0, 0.0), ob, radius=2.5)["found"][0] == 0
        r = one((closer, 0.0, 0.0), ob, radius=2.5)
        assert r["found"][0] == 1 and r["sd"][0, 0] == closer - 1.0 < 2.5
        assert one((at, 0.0, 0.0), ob, radius=np.nextafter(2.5, 3.0))["found"][0] == 1
    # two identical obstacles list in index order; the nearer one first whatever its index
    ob = obstacles([(SPHERE, (5.0, 0.0, 0.0), (1.0, 0, 0)), (BOX, (2.0, 0.0, 0.0), (0.5, 0.5, 0.5)), (SPHERE, (5.0, 0.0, 0.0), (1.0, 0, 0)),
                    (BOX, (2.0, 0.0, 0.0), (0.5, 0.5, 0.5))])
    r = one((0.0, 0.0, 0.0), ob, k=3, radius=10.0)
    assert r["found"][0] == 4 and r["count"][0] == 3 and list(r["index"][0]) == [1, 3, 0] and list(r["sd"][0]) == [1.5, 1.5, 4.0]
    assert list(one((0.0, 0.0, 0.0), ob, k=8, radius=10.0)["index"][0]) == [1, 3, 0, 2, -1, -1, -1, -1]
    # negative distances order before positive ones: the deepest obstacle first
    deep = obstacles([(SPHERE, (0.0, 0.0, 0.0), (1.0, 0, 0)), (SPHERE, (0.0, 0.0, 0.0), (3.0, 0, 0)), (BOX, (0.0, 0.0, 0.0), (2.0, 2.0, 2.0))])
    r = one((0.5, 0.0, 0.0), deep, k=4, radius=0.25)
    assert list(r["index"][0]) == [1, 2, 0, -1] and list(r["sd"][0]) == [-2.5, -1.5, -0.5, 0.0]
    # worlds: the label must match unless the obstacle carries ALL_WORLDS; every label is 0 unless given
    ob = obstacles([(SPHERE, (0, 0, 0), (1.0, 0, 0), 0), (SPHERE, (0, 0, 0), (1.0, 0, 0), 5), (SPHERE, (0, 0, 0), (1.0, 0, 0), -3, ALL_WORLDS)])
    p = np.zeros((3, 3))
    r = restate_obstacles(p, None, [0, 5, 9], ob, 4, 1.0)
    assert [list(row[:2]) for row in r["index"]] == [[0, 2], [1, 2], [2, -1]] and list(r["found"]) == [2, 2, 1]
    assert list(restate_obstacles(p, None, None, ob, 4, 1.0)["found"]) == [2, 2, 2]
    # a non-finite UAV has no obstacles and adds +0.0; an empty set gives empty rows
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.0, 0.0, 0.0]])
    r = restate_obstacles(bad, None, None, deep, 2, 5.0)
    assert list(r["found"]) == [0, 0, 0, 3] and (r["index"][:3] == -1).all() and same_bits(r["sd"][:3], np.zeros((3, 2)))
    for kind in (HINGE2, COUNT):
        term = restate_cost(r, 2, 5.0, kind, 1.5)
        assert same_bits(term[:3], np.zeros(3)) and term[3] > 0
    assert same_bits(add_bits(np.array([-0.0]), np.array([0.0])), [0.0])
    e = restate_obstacles(p, None, None, np.zeros(0, OBSTACLE), 3, 5.0)
    assert (e["found"] == 0).all() and (e["index"] == -1).all() and e["rel"].shape == (3, 3, 3)
    # the cost: HINGE2 grows the deeper the UAV is inside; COUNT counts the listed ones
    r = one((0.5, 0.0, 0.0), deep, k=2, radius=0.25)
    assert restate_cost(r, 2, 0.25, HINGE2, 2.0)[0] == (0.0 + (2.0 * 2.75) * 2.75) + (2.0 * 1.75) * 1.75
    assert restate_cost(r, 2, 0.25, COUNT, 0.3)[0] == 0.3 + 0.3 and r["found"][0] == 3


def test_restatement_equals_a_scalar_definition():
    """the vectorised restatement against one (UAV, obstacle) pair at a time in Python floats, on a slice of the fixture"""
    import math
    pos, worlds, ob = fixture_scene()
    sel = np.r_[0:40, 64:100, 198:204, 1000:1040]
    k, radius = 8, FIXTURE_RADIUS
    res = restate_obstacles(pos[sel], None, worlds[sel], ob, k, radius)

    def mx(a, b):
        return b if a < b else a

    def mn(a, b):
        return b if b < a else a

    for row, i in enumerate(sel):
        p = [float(v) for v in pos[i]]
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
                if sd < radius:
                    hits.append((sd, j))
        hits.sort()
        assert res["found"][row] == len(hits), i
        assert list(res["index"][row]) == [j for _, j in hits[:k]] + [-1] * (k - min(k, len(hits))), i
        assert same_bits(res["sd"][row, :min(k, len(hits))], [s for s, _ in hits[:k]]), i


def test_fixture_coverage():
    pos, worlds, ob = fixture_scene()
    n, M = len(pos), len(ob)
    assert n <= 4096 and M <= 512 and OBSTACLE.itemsize == 64
    res = restate_obstacles(pos, None, worlds, ob, 8, FIXTURE_RADIUS)
    found, sd = res["found"], res["sd"]
    inside = res["index"][(sd < 0) & (res["index"] >= 0)]
    assert set(ob["kind"][inside]) == {SPHERE, BOX, CYLINDER}, "every kind has UAVs inside it"
    for kind in (SPHERE, BOX, CYLINDER):
        assert (ob["kind"][inside] == kind).sum() >= 10
    assert (found > 32).sum() >= 20 and (found > 8).sum() >= 60 and (found == 0).sum() >= 300, "found > k for k = 1, 8, 32, and UAVs without obstacles"
    assert 0.2 < ((found > 0) & (found <= 8)).mean()
    assert set(np.unique(worlds)) == {0, 5} and (worlds == 0).sum() > 1000 and (worlds == 5).sum() > 1000
    flags, w = ob["flags"], ob["world"]
    assert ((flags == 0) & (w == 0)).sum() > 50 and ((flags == 0) & (w == 5)).sum() > 50 and (flags == ALL_WORLDS).sum() > 50
    listed = res["index"][res["index"] >= 0]
    assert ((ob["flags"][listed] == 0) & (ob["world"][listed] == 5)).any() and (ob["flags"][listed] == ALL_WORLDS).any()
    # the labels matter: without them the lists differ
    assert (restate_obstacles(pos, None, None, ob, 8, FIXTURE_RADIUS)["found"] != found).sum() > 100
    assert (~np.isfinite(pos).all(axis=1)).sum() == 2 and (found[~np.isfinite(pos).all(axis=1)] == 0).all()
    assert np.isinf(ob["h"][:, 2]).sum() > 30
    grid = grid_of(ob, FIXTURE_RADIUS)
    assert all(d > 1 for d in grid["dims"]) and grid["cells"] > 100, grid  # several cells per axis
    assert grid["edge"] == 2 * FIXTURE_RADIUS and grid["longest"] < M
    small = grid_of(ob[:5], FIXTURE_RADIUS * 40)
    assert small["dims"] == (1, 1, 1) and small["items"] == 5  # the one-cell case of the GPU tests
    assert grid_of(ob, 0.75)["dims"] != grid["dims"]  # another radius, another grid


# ---- tests: the ABI ----

NEW_SYMBOLS = ["mrs_swarm_set_obstacles", "mrs_swarm_get_obstacles", "mrs_swarm_obstacle_stats", "mrs_obstacle_width",
               "mrs_swarm_nearest_obstacles_device", "mrs_swarm_obstacle_cost_device"]


def test_symbols_are_declared_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm, tensors
    L = C.CDLL(swarm.LIB_PATH)
    header = abi_header()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert hasattr(L, name) and name in swarm.ABI_SYMBOLS, name
    for method in ("set_obstacles", "get_obstacles", "obstacle_stats", "nearest_obstacles_device", "obstacle_cost_device"):
        assert callable(getattr(swarm.Swarm, method, None)), method
    for fn in ("set_obstacles", "nearest_obstacles", "obstacle_cost", "obstacle_width"):
        assert callable(getattr(tensors, fn, None)), fn


def test_header_prototypes_argtypes_and_methods_agree(mrs):
    from mrs_multirotor_simulator_amd import swarm
    L = swarm.load_library()
    want = {
        "mrs_swarm_set_obstacles": ["s", "count", "obstacles"],
        "mrs_swarm_get_obstacles": ["s", "capacity", "out", "count"],
        "mrs_swarm_obstacle_stats": ["s", "stats"],
        "mrs_obstacle_width": ["fields", "k", "width"],
        "mrs_swarm_nearest_obstacles_device": ["s", "first", "count", "k", "radius", "fields", "dev_rows", "dtype", "stride", "dev_index",
                                               "index_stride", "dev_count", "ext_stream"],
        "mrs_swarm_obstacle_cost_device": ["s", "first", "count", "k", "radius", "kind", "weight", "dev_cost", "accumulate", "dev_found",
                                           "ext_stream"],
    }
    for name, names in want.items():
        got_names, types = abi_prototype(name)
        assert got_names == names, name
        got = [C.c_void_p if issubclass(a, C._Pointer) else a for a in getattr(L, name).argtypes]  # (a typed pointer is a pointer)
        assert [TYPES[t] for t in types] == got, (name, types)
    for method, name in (("nearest_obstacles_device", "mrs_swarm_nearest_obstacles_device"), ("obstacle_cost_device", "mrs_swarm_obstacle_cost_device")):
        params = list(inspect.signature(getattr(swarm.Swarm, method)).parameters)
        assert params == ["self"] + want[name][1:], method
    # the nearest-obstacle call has the prototype of the nearest-neighbour call, the cost call that of the proximity cost without eps
    assert abi_prototype("mrs_swarm_nearest_obstacles_device") == abi_prototype("mrs_swarm_nearest_device")
    pn, pt = abi_prototype("mrs_swarm_proximity_cost_device")
    cut = pn.index("eps")
    assert abi_prototype("mrs_swarm_obstacle_cost_device") == (pn[:cut] + pn[cut + 1:], pt[:cut] + pt[cut + 1:])


def test_struct_layouts_and_header_values(mrs):
    from mrs_multirotor_simulator_amd import swarm, tensors
    assert C.sizeof(swarm.Obstacle) == 64 == swarm.OBSTACLE_DTYPE.itemsize and swarm.OBSTACLE_DTYPE == OBSTACLE
    assert C.sizeof(swarm.ObstacleStats) == 64
    for (name, ctype), (dname, (ddtype, off)) in zip(swarm.Obstacle._fields_, sorted(swarm.OBSTACLE_DTYPE.fields.items(), key=lambda f: f[1][1])):
        assert name == dname and getattr(swarm.Obstacle, name).offset == off and C.sizeof(ctype) == ddtype.itemsize, name
    header = abi_header()
    m = re.search(r"typedef struct \{([^}]*)\} mrs_obstacle_t;", header)
    fields = re.findall(r"(\w+)(?:\[3\])?\s*[,;]", m.group(1))
    assert fields == ["kind", "world", "flags", "reserved", "c", "h"]
    vals = {k: int(eval(v.replace("u", ""))) for k, v in re.findall(r"\b(MRS_(?:OBST|ON)_[A-Z0-9_]+)\s*=\s*([0-9<u ]+)", header)}
    assert vals == {"MRS_OBST_SPHERE": 0, "MRS_OBST_BOX": 1, "MRS_OBST_CYLINDER": 2, "MRS_OBST_ALL_WORLDS": 1, "MRS_OBST_MAX": 1 << 20,
                    "MRS_OBST_MAX_K": 32, "MRS_ON_REL": 1, "MRS_ON_REL_BODY": 2, "MRS_ON_DIST": 4, "MRS_ON_ALL": 7}
    for name, v in vals.items():
        assert getattr(swarm, name[4:]) == getattr(tensors, name[4:]) == v, name
    assert (SPHERE, BOX, CYLINDER, ALL_WORLDS) == (swarm.OBST_SPHERE, swarm.OBST_BOX, swarm.OBST_CYLINDER, swarm.OBST_ALL_WORLDS)
    assert (ON_REL, ON_REL_BODY, ON_DIST) == (swarm.ON_REL, swarm.ON_REL_BODY, swarm.ON_DIST)


def test_obstacle_width_is_host_only(mrs):
    from mrs_multirotor_simulator_amd import swarm
    assert swarm.obstacle_width(0, 5) == 0
    assert [swarm.obstacle_width(f, 1) for f in (ON_REL, ON_REL_BODY, ON_DIST, 7)] == [3, 3, 1, 7]
    assert swarm.obstacle_width(ON_REL | ON_DIST, 8) == 32 and swarm.obstacle_width(7, 32) == 224
    for fields, k in ((8, 1), (0x17, 4), (7, 0), (7, 33), (7, -1), (0, 0)):
        with pytest.raises(mrs.MrsError, match="error 1:"):
            swarm.obstacle_width(fields, k)


# ---- tests: the tensor layer without a GPU ----

_Swarm = stand_in("nearest_obstacles_device", "obstacle_cost_device", "set_obstacles")


def test_obstacle_cost_refuses_before_the_library(monkeypatch):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64, i32 = _Swarm(), torch.float64, torch.int32
    cases = [
        (dict(out=torch.zeros(100, dtype=f64)), "is on cpu"),
        (dict(out=on(torch.zeros(100, dtype=f64), 1)), "the swarm lives on cuda:0"),
        (dict(out=on(torch.zeros(100, dtype=torch.float32))), "always torch.float64"),
        (dict(out=on(torch.zeros(99, dtype=f64))), "expected a vector of 100 elements"),
        (dict(out=on(torch.zeros(200, dtype=f64)[::2])), "vector is not contiguous"),
        (dict(out=None, accumulate=True), "accumulate=True needs the `out` vector"),
        (dict(found=torch.zeros(100, dtype=i32)), "is on cpu"),
        (dict(found=on(torch.zeros(100, dtype=torch.int64))), "expected torch.int32"),
        (dict(found=on(torch.zeros(101, dtype=i32))), "expected a vector of 100 elements"),
        (dict(found=3), "expected a torch.Tensor"),
        (dict(kind=T.PROX_INVERSE), "PROX_INVERSE is not an obstacle cost kind"),
        (dict(first=10, count=50, out=on(torch.zeros(90, dtype=f64))), "expected a vector of 50 elements"),
    ]
    for kw, msg in cases:
        args = dict(out=on(torch.zeros(kw.get("count", 100), dtype=f64)))
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            T.obstacle_cost(g, 5.0, **args)
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    for kw in (dict(), dict(accumulate=True), dict(found=on(torch.zeros(100, dtype=i32))), dict(kind=T.PROX_COUNT, k=32)):
        with pytest.raises(AssertionError, match="obstacle_cost_device"):
            T.obstacle_cost(g, 5.0, out=on(torch.zeros(100, dtype=f64)), **kw)


def test_nearest_obstacles_refuses_and_hands_strides_through(mrs, monkeypatch):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f32, i32 = _Swarm(), torch.float32, torch.int32
    k, fields = 4, T.ON_REL | T.ON_DIST  # 16 elements per row
    cases = [
        (dict(out=torch.zeros(100, 16)), "is on cpu"),
        (dict(out=on(torch.zeros(100, 16), 1)), "the swarm lives on cuda:0"),
        (dict(out=on(torch.zeros(100, 15))), r"expected a \[100, >= 16\] matrix"),
        (dict(out=on(torch.zeros(99, 16))), r"expected a \[100, >= 16\] matrix"),
        (dict(out=on(torch.zeros(100, 16, dtype=torch.float16))), "dtype must be torch.float32 or torch.float64"),
        (dict(out=on(torch.zeros(100, 32)[:, ::2])), "rows are not contiguous"),
        (dict(index=on(torch.zeros(100, 3, dtype=i32))), r"expected a \[100, >= 4\] matrix"),
        (dict(index=on(torch.zeros(100, 4, dtype=torch.int64))), "expected torch.int32"),
        (dict(counts=on(torch.zeros(100, dtype=torch.int64))), "expected torch.int32"),
        (dict(counts=on(torch.zeros(101, dtype=i32))), "expected a vector of 100 elements"),
    ]
    def outputs(rows=100, width=16, iw=k, dtype=f32):
        return dict(out=on(torch.zeros(rows, width, dtype=dtype)), index=on(torch.zeros(rows, iw, dtype=i32)), counts=on(torch.zeros(rows, dtype=i32)))

    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            T.nearest_obstacles(g, k, 5.0, fields, **dict(outputs(), **kw))
    with pytest.raises(mrs.MrsError, match="error 1:"):  # (the width comes from the library's host-only helper)
        T.nearest_obstacles(g, 33, 5.0, fields)
    with pytest.raises(mrs.MrsError, match="error 1:"):
        T.nearest_obstacles(g, k, 5.0, 8)
    monkeypatch.setattr(T, "_stream", lambda dev: 1234)

    with pytest.raises(AssertionError, match="nearest_obstacles_device"):
        T.nearest_obstacles(g, k, 5.0, fields, **outputs())

    calls = []

    class Taking(_Swarm):
        def nearest_obstacles_device(self, *a):
            calls.append(a)

    o = outputs(60, 40, 9, torch.float64)
    rows, index, counts = T.nearest_obstacles(Taking(), k, 2.5, fields, first=7, count=60, **o)
    assert calls[-1] == (7, 60, k, 2.5, fields, o["out"].data_ptr(), T.DTYPE_F64, 40, o["index"].data_ptr(), 9, o["counts"].data_ptr(), 1234)
    assert rows.shape == (60, 16) and index.shape == (60, k) and counts.shape == (60,)
    o = outputs()
    rows, index, counts = T.nearest_obstacles(Taking(), k, 2.5, 0, index=o["index"], counts=o["counts"])  # no fields: no rows, the default range
    assert rows is None and calls[-1][:5] == (0, 100, k, 2.5, 0) and calls[-1][5:8] == (0, T.DTYPE_F32, 0) and calls[-1][9] == k
    o = outputs(100, 32, 8)
    rows, _, _ = T.nearest_obstacles(Taking(), 8, 2.5, **o)  # the default fields
    assert rows.shape == (100, 32) and rows.dtype == f32 and calls[-1][4] == fields and calls[-1][7] == 32 and calls[-1][6] == T.DTYPE_F32


def test_set_obstacles_checks_and_packs(monkeypatch):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = _Swarm()
    kinds, c, h = [0, 1, 2], np.zeros((3, 3)), np.ones((3, 3))
    bad = [
        (([0, 1, 3], c, h), {}, "kinds must be"),
        ((kinds, np.zeros((3, 2)), h), {}, r"centres must have shape \[3, 3\]"),
        ((kinds, c, np.ones((2, 3))), {}, r"sizes must have shape \[3, 3\]"),
        ((kinds, np.full((3, 3), np.nan), h), {}, "centres must be finite"),
        ((kinds, c, -h), {}, "sizes must be finite and >= 0"),
        ((kinds, c, np.full((3, 3), np.inf)), {}, "sizes must be finite and >= 0"),
        ((kinds, c, h), dict(worlds=[1, 2]), r"worlds must have shape \[3\]"),
        ((kinds, c, h), dict(all_worlds=np.zeros((3, 1), bool)), r"all_worlds must have shape \[3\]"),
        ((np.zeros((3, 1)), c, h), {}, r"kinds must have shape \[M\]"),
        ((["a", "b", "c"], c, h), {}, "expected numbers"),
    ]
    for args, kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            T.set_obstacles(g, *args, **kw)
    with pytest.raises(AssertionError, match="set_obstacles"):
        T.set_obstacles(g, kinds, c, h)
    got = []

    class Taking(_Swarm):
        def set_obstacles(self, rec):
            got.append(rec)

    sizes = np.array([[1.0, np.nan, -1.0], [1.0, 2.0, 3.0], [0.5, np.nan, np.inf]])  # unused entries are not checked; a pillar's inf is legal
    T.set_obstacles(Taking(), torch.tensor(kinds), torch.tensor(c + 2.0), torch.tensor(sizes), worlds=[0, 5, -1], all_worlds=[False, False, True])
    rec = got[-1]
    assert rec.dtype == OBSTACLE and list(rec["kind"]) == kinds and list(rec["world"]) == [0, 5, -1] and list(rec["flags"]) == [0, 0, ALL_WORLDS]
    assert (rec["c"] == 2.0).all() and np.array_equal(rec["h"], sizes, equal_nan=True) and (rec["reserved"] == 0).all()
    T.set_obstacles(Taking(), [], np.zeros((0, 3)), np.zeros((0, 3)))
    assert len(got[-1]) == 0


# ---- tests: the C++ programs ----

def test_grid_builder_under_sanitizers():
    out = subprocess.run([build_grid_test()], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    for tag in ("functions", "empty_and_single", "random", "coarsened", "all"):
        assert f"ok {tag}" in out.stdout, out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_cell_walk_under_sanitizers():
    """tests/cpp/obstacle_walk_test.cpp: mrs_obst::walk_cell, the cell walk of the range scans, on the host compiler without
    contraction under the address and undefined-behaviour sanitizers — intact arrays, damaged arrays, m == 0"""
    exe = os.path.join(ROOT, "tests", "cpp", "obstacle_walk_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "obstacle_walk_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok obstacle_walk" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_obstacles_test_compiles(mrs):
    """tests/cpp/obstacles_test.cpp builds against the facade and the HIP runtime (run on the GPU by test_obstacles_gpu.py)"""
    from test_device_io_gpu import build_cpp
    assert os.path.exists(build_cpp("obstacles_test"))
