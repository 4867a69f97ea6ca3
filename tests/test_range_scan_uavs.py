"""CPU-side checks of the range scans that see other UAVs (include/mrs_swarm.h, "range scans that see other UAVs"): the numpy restatement
the GPU tests compare bits against (restate_scan_uavs below, built on the restatement of test_range_scan.py) is checked here on its own
— known answers that are exact in binary, and a geometric check on the fixture scene that owes nothing to the ray formula; the pure
functions of csrc/range_scan_math.h the kernel calls (uav_target, gate, ray, take_uav) give the restatement's bits in
tests/cpp/range_scan_uavs_math_test.cpp under the address and undefined-behaviour sanitizers; the symbol is exported and listed, header
prototype, ctypes argtypes and method signature agree; the tensor wrapper refuses bad arguments before the library is reached.  No
pointer reaches the library."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import abi_header, abi_prototype, fake_cuda, stand_in
from test_obstacles import OBSTACLE, SPHERE, fixture_scene, obstacles, same_bits
from test_range_scan import BODY_FRAME, GROUND, HIT_GROUND, HIT_NONE, INF, ROOT, TYPES, beam_directions, gate, ground_range, mixed_beams, ray, restate_scan

HIT_UAV = -3
SCENE_RADII = (0.25 + 0.15, 0.27 + 0.11, 0.325 + 0.19)  # x500, f550, t650: arm_length + prop_radius (0.40, 0.38, 0.515), one FP64 addition each


# ---- the numpy restatement (used by test_range_scan_uavs_gpu.py) ----

def uav_targets(pos, rad):
    """UAV j as a beam sees it: the sphere record {SPHERE, c = p_j, h[0] = rad_j}"""
    t = np.zeros(len(pos), OBSTACLE)
    t["kind"], t["c"], t["h"][:, 0] = SPHERE, pos, rad
    return t


def candidate_pairs(pos, worlds, rad, max_range, observers=None, chunk=256):
    """(i, j) of every (observer, candidate) pair in ascending (i, j): j != i, world[j] == world[i], the gate on every axis — all pairs
    are tested, a chunk of observers at a time.  A non-finite p_j fails the gate; a non-finite observer has no candidates."""
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    worlds = np.zeros(n, np.int32) if worlds is None else np.asarray(worlds).astype(np.int32)
    targets = uav_targets(pos, rad)
    observers = np.arange(n) if observers is None else np.asarray(observers)
    pi, pj = [], []
    for cut in range(0, len(observers), chunk):
        i = observers[cut:cut + chunk]
        ok = gate(pos[i], targets, max_range) & (worlds[i][:, None] == worlds[None, :]) & (i[:, None] != np.arange(n)[None, :])
        ok &= np.isfinite(pos[i]).all(axis=1)[:, None]
        a, b = np.nonzero(ok)
        pi.append(i[a])
        pj.append(b)
    return np.concatenate(pi), np.concatenate(pj)


@np.errstate(all="ignore")
def restate_scan_uavs(pos, R, worlds, rad, ob, beams, max_range, body_frame=True, ground_z=None, chunk=1 << 21, base=None, observers=None):
    """The contract of mrs_swarm_range_scan_uavs_device for every UAV (or the rows `observers`): (ranges [n, B] FP64, hit [n, B] int32,
    uav [n, B] int32).  rad [n]: arm_length + prop_radius of each UAV's airframe.  base: restate_scan(...) of the same arguments without
    the ground, which is then not computed again.  The obstacles first (restate_scan), then among the candidate UAVs the lexicographic
    minimum of (t_j, j), which takes the beam only if strictly nearer, then the ground."""
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    beams = np.asarray(beams, np.float64).reshape(-1, 3)
    B = len(beams)
    max_range = np.float64(max_range)
    rad = np.broadcast_to(np.asarray(rad, np.float64), (n,))
    if R is None:
        R = np.broadcast_to(np.eye(3), (n, 3, 3))
    if base is None:
        base = restate_scan(pos, R, worlds, ob, beams, max_range, body_frame)
    ranges, hit = base[0].copy(), base[1].copy()
    uav = np.full((n, B), -1, np.int32)
    u = beam_directions(beams, R, body_frame)
    targets = uav_targets(pos, rad)
    pi, pj = candidate_pairs(pos, worlds, rad, max_range, observers)
    per = max(1, chunk // max(B, 1))
    cut = 0
    while cut < len(pi):
        end = min(cut + per, len(pi))
        if end < len(pi):  # whole observers only
            end = int(np.searchsorted(pi, pi[end], side="left"))
            if end == cut:
                end = int(np.searchsorted(pi, pi[cut], side="right"))
        i, j = pi[cut:end], pj[cut:end]
        t = ray(pos[i], u[i], targets[j])
        t = np.where(np.isnan(t), INF, t)  # (a NaN is never taken)
        who, starts, inv = np.unique(i, return_index=True, return_inverse=True)
        tmin = np.minimum.reduceat(t, starts, axis=0)
        jmin = np.minimum.reduceat(np.where(t == tmin[inv], j[:, None], np.int64(1) << 40), starts, axis=0)
        won = tmin < ranges[who]  # strictly: an obstacle at the same range keeps the beam
        ranges[who] = np.where(won, tmin, ranges[who])
        hit[who] = np.where(won, HIT_UAV, hit[who])
        uav[who] = np.where(won, jmin, -1)
        cut = end
    if ground_z is not None:
        tg = ground_range(pos[:, 2, None], u[..., 2], np.asarray(ground_z, np.float64).reshape(n, 1))
        won = (tg < ranges) & np.isfinite(pos).all(axis=1)[:, None]
        ranges = np.where(won, tg, ranges)
        hit = np.where(won, HIT_GROUND, hit).astype(np.int32)
        uav = np.where(won, -1, uav).astype(np.int32)
    if observers is not None:
        observers = np.asarray(observers)
        return ranges[observers], hit[observers], uav[observers]
    return ranges, hit, uav


def scene_radii():
    n = len(fixture_scene()[0])
    third = n // 3
    return np.repeat(SCENE_RADII, [third, third, n - 2 * third])


# ---- tests: the restatement ----

NO_OBSTACLES = np.zeros(0, OBSTACLE)
X, NEG_X, Y, DOWN = (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0)


def scan(pos, beams, max_range=100.0, rad=0.5, ob=NO_OBSTACLES, worlds=None, **kw):
    return restate_scan_uavs(np.asarray(pos, np.float64), None, worlds, rad, ob, np.atleast_2d(np.asarray(beams, np.float64)), max_range, **kw)


def test_restatement_known_answers():
    from mrs_multirotor_simulator_amd.airframes import AIRFRAMES
    assert SCENE_RADII == tuple(AIRFRAMES[a]["arm_length"] + AIRFRAMES[a]["prop_radius"] for a in ("x500", "f550", "t650"))
    assert np.allclose(SCENE_RADII, (0.40, 0.38, 0.515), rtol=0, atol=1e-15)
    # arm_length = prop_radius = 0.25: the observer at the origin sees the target at (5, 0, 0) at 4.5 along +x and not along -x
    r, h, w = scan([(0, 0, 0), (5.0, 0, 0)], [X, NEG_X, Y])
    assert list(r[0]) == [4.5, 100.0, 100.0] and list(h[0]) == [HIT_UAV, HIT_NONE, HIT_NONE] and list(w[0]) == [1, -1, -1]
    assert list(r[1]) == [100.0, 4.5, 100.0] and list(w[1]) == [-1, 0, -1]  # and the target sees the observer, never itself
    # a target exactly max_range away is not hit; one ulp more range hits
    r, h, w = scan([(0, 0, 0), (5.0, 0, 0)], [X], max_range=4.5)
    assert r[0, 0] == 4.5 and h[0, 0] == HIT_NONE and w[0, 0] == -1
    r, h, w = scan([(0, 0, 0), (5.0, 0, 0)], [X], max_range=np.nextafter(4.5, 5.0))
    assert r[0, 0] == 4.5 and h[0, 0] == HIT_UAV and w[0, 0] == 1
    # an obstacle and a UAV at equal range: the obstacle keeps the beam; a nearer UAV takes it; a nearer obstacle occludes the UAV
    wall = obstacles([(SPHERE, (5.0, 0.0, 0.0), (0.5, 0, 0))])
    r, h, w = scan([(0, 0, 0), (5.0, 0, 0)], [X], ob=wall)
    assert r[0, 0] == 4.5 and h[0, 0] == 0 and w[0, 0] == -1
    r, h, w = scan([(0, 0, 0), (4.0, 0, 0)], [X], ob=wall)
    assert r[0, 0] == 3.5 and h[0, 0] == HIT_UAV and w[0, 0] == 1
    r, h, w = scan([(0, 0, 0), (7.0, 0, 0)], [X], ob=wall)
    assert r[0, 0] == 4.5 and h[0, 0] == 0 and w[0, 0] == -1
    # two UAVs at equal range: the lower index wins, wherever it stands in the array
    r, h, w = scan([(0, 0, 0), (5.0, 0, 0), (5.0, 0, 0)], [X])
    assert r[0, 0] == 4.5 and w[0, 0] == 1
    r, h, w = scan([(5.0, 0, 0), (5.0, 0, 0), (0, 0, 0), (9.0, 0, 0)], [X])
    assert r[2, 0] == 4.5 and w[2, 0] == 0
    # an observer inside two other UAVs' spheres: 0.0 on every beam and the lower index
    r, h, w = scan([(0.25, 0, 0), (0, 0, 0), (0.5, 0.25, 0)], [X, NEG_X, Y, DOWN])
    assert same_bits(r[0], np.zeros(4)) and (h[0] == HIT_UAV).all() and (w[0] == 1).all()
    r, h, w = scan([(0.5, 0, 0), (0, 0, 0)], [X])  # on the surface, pointing away: 0.0
    assert same_bits(r[0], [0.0]) and w[0, 0] == 1
    # a target under another label is invisible; a NaN or infinite target is invisible; a non-finite observer sees nothing
    r, h, w = scan([(0, 0, 0), (5.0, 0, 0), (7.0, 0, 0)], [X], worlds=[3, 4, 3])
    assert r[0, 0] == 6.5 and w[0, 0] == 2 and r[1, 0] == 100.0 and h[1, 0] == HIT_NONE
    r, h, w = scan([(0, 0, 0), (np.nan, 0, 0), (5.0, np.inf, 0), (7.0, 0, 0)], [X], ground_z=np.full(4, -50.0))
    assert r[0, 0] == 6.5 and w[0, 0] == 3 and (r[1:3] == 100.0).all() and (h[1:3] == HIT_NONE).all() and (w[1:3] == -1).all()
    # the ground is taken last: strictly nearer only, and it resets uav
    r, h, w = scan([(0, 0, 5.0), (0, 0, 2.0)], [DOWN], ground_z=[2.5, 0.0])
    assert r[0, 0] == 2.5 and h[0, 0] == HIT_UAV and w[0, 0] == 1  # the sphere's top at z = 2.5, the plane at 2.5: the UAV keeps the beam
    r, h, w = scan([(0, 0, 5.0), (0, 0, 2.0)], [DOWN], ground_z=[3.0, 0.0])
    assert r[0, 0] == 2.0 and h[0, 0] == HIT_GROUND and w[0, 0] == -1
    # per-UAV radii: the target's radius counts, not the observer's
    r, h, w = scan([(0, 0, 0), (5.0, 0, 0)], [X, NEG_X], rad=[0.25, 1.0])
    assert r[0, 0] == 4.0 and r[1, 1] == 4.75
    # the gate: |d| - rad < max_range on every axis; without UAVs the result is restate_scan's
    assert len(candidate_pairs(np.array([(0, 0, 0), (5.0, 0, 0)]), None, 0.5, 4.5)[0]) == 0
    assert len(candidate_pairs(np.array([(0, 0, 0), (5.0, 0, 0)]), None, 0.5, np.nextafter(4.5, 5.0))[0]) == 2
    pos, worlds, ob = fixture_scene()
    far = pos[:1]
    base = restate_scan(far, None, worlds[:1], ob, mixed_beams(7), 6.0)
    r, h, w = restate_scan_uavs(far, None, worlds[:1], 0.4, ob, mixed_beams(7), 6.0)
    assert same_bits(r, base[0]) and np.array_equal(h, base[1]) and (w == -1).all()


_scene = {}


def scene_reference(nb=16, body=False, max_range=6.0):
    """the restatement of the fixture scene with the radii of its three airframes, computed once per key and never written to"""
    from test_range_scan import scene_rotations
    key = (nb, body, max_range)
    if key not in _scene:
        pos, worlds, ob = fixture_scene()
        base = restate_scan(pos, scene_rotations(), worlds, ob, mixed_beams(nb), max_range, body)
        _scene[key] = base + restate_scan_uavs(pos, scene_rotations(), worlds, scene_radii(), ob, mixed_beams(nb), max_range, body, base=base)
        for a in _scene[key]:
            a.setflags(write=False)
    return _scene[key]


def test_every_outcome_occurs_on_the_fixture_scene():
    """16 world-frame beams of mixed_beams at 6 m: the counts the scene was chosen for (half of each is asserted)"""
    pos, worlds, ob = fixture_scene()
    r0, h0, r, h, w = scene_reference()
    on_uav = h == HIT_UAV
    assert on_uav.sum() >= 950 and (on_uav & (r == 0.0)).sum() >= 80, (on_uav.sum(), (on_uav & (r == 0.0)).sum())
    assert (on_uav & (h0 >= 0)).sum() >= 117, (on_uav & (h0 >= 0)).sum()  # a UAV beats an obstacle
    # an obstacle keeps the beam from a UAV: the same scan without obstacles hits a UAV there
    _, hu, _ = restate_scan_uavs(pos, None, worlds, scene_radii(), ob[:0], mixed_beams(16), 6.0, False)
    assert ((hu == HIT_UAV) & (h >= 0)).sum() >= 499, ((hu == HIT_UAV) & (h >= 0)).sum()
    pi, pj = candidate_pairs(pos, worlds, scene_radii(), 6.0)
    assert np.bincount(pi, minlength=len(pos)).max() >= 38
    assert ((w >= 0) == on_uav).all() and (w[on_uav] != np.nonzero(on_uav)[0]).all() and (worlds[w[on_uav]] == worlds[np.nonzero(on_uav)[0]]).all()
    assert (h[200:202] == HIT_NONE).all() and (w[200:202] == -1).all() and not np.isin(w, (200, 201)).any()
    # wherever no UAV took the beam the result is the old scan's
    assert same_bits(r[~on_uav], r0[~on_uav]) and np.array_equal(h[~on_uav], h0[~on_uav]) and (r[on_uav] < r0[on_uav]).all()


def test_geometric_check_independent_of_the_ray_formula():
    """On the fixture scene (16 world-frame beams, 6 m): at every reported UAV hit the point p + t u lies on the reported UAV's sphere —
    its distance to the centre equals the radius to 1e-9 relative — or t == 0 and p lies in or on it; and no same-world UAV sphere holds
    one of 64 evenly spaced points of the beam before its range (distance to every other centre >= radius (1 - 1e-9)).  Only
    Euclidean distances are formed.  1e-9: coordinates <= 40 m and t <= 6 m round the point at about 1e-14; a grazing hit can move t by
    about 1e-7, along the tangent, which changes the distance in second order only."""
    pos, worlds, ob = fixture_scene()
    rad = scene_radii()
    r0, h0, r, h, w = scene_reference()
    u = beam_directions(mixed_beams(16), np.broadcast_to(np.eye(3), (len(pos), 3, 3)), False)
    i, b = np.nonzero(h == HIT_UAV)
    j, t = w[i, b], r[i, b]
    x = pos[i] + t[:, None] * u[i, b]
    d = np.sqrt(((x - pos[j]) ** 2).sum(axis=1))
    assert (np.abs(d[t > 0] - rad[j][t > 0]) <= 1e-9 * rad[j][t > 0]).all(), np.abs(d[t > 0] / rad[j][t > 0] - 1).max()
    assert (d[t == 0] <= rad[j][t == 0] * (1 + 1e-9)).all() and (t > 0).sum() > 500 and (t == 0).sum() > 50
    # along every beam of every finite observer, against every same-world UAV but the observer
    frac = np.arange(64) / 64.0
    checked = 0
    for k in np.flatnonzero(np.isfinite(pos).all(axis=1)):
        others = np.flatnonzero((worlds == worlds[k]) & (np.arange(len(pos)) != k) & (np.abs(pos - pos[k]).max(axis=1) < 6.0 + 0.6))
        live = r[k] > 0
        if not len(others) or not live.any():
            continue
        pts = pos[k] + (r[k][live, None] * frac[None, :])[..., None] * u[k][live][:, None, :]  # [b, 64, 3], all before the range
        dist = np.sqrt(((pts[:, :, None, :] - pos[others][None, None]) ** 2).sum(axis=-1))
        assert (dist >= rad[others] * (1 - 1e-9)).all(), k
        checked += dist.size
    assert checked > 1000000


# ---- tests: the pure functions of csrc/range_scan_math.h, stand-alone under the sanitizers ----

CASE = np.dtype([("q", "f8", 3), ("rad", "f8"), ("p", "f8", 3), ("u", "f8", 3), ("max_range", "f8"), ("t", "f8"), ("best_t", "f8"), ("j", "i4"),
                 ("best_j", "i4"), ("pad", "f8", 2)])
_math_exe = []


def build_math_test():
    """tests/cpp/range_scan_uavs_math_test.cpp: the host compiler, no contraction, address and undefined-behaviour sanitizers (the
    command of test_range_scan.build_math_test)"""
    if not _math_exe:
        exe = os.path.join(ROOT, "tests", "cpp", "range_scan_uavs_math_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "range_scan_uavs_math_test.cpp"), "-o", exe])
        _math_exe.append(exe)
    return _math_exe[0]


def test_pure_functions_equal_the_restatement_bit_for_bit():
    assert CASE.itemsize == 128
    pos, worlds, ob = fixture_scene()
    rad = scene_radii()
    rng = np.random.default_rng(8)
    beams = mixed_beams(16)
    observers = np.r_[0:64, 198:204, 1000:1100, 3000:3072]
    pi, pj = candidate_pairs(pos, worlds, rad, 6.0, observers)
    far = rng.integers(0, len(pos), (len(pi), 2))  # as many arbitrary pairs: most fail the gate, some hold a non-finite UAV
    pi, pj = np.concatenate([pi, far[:, 0], [200, 0, 201]]), np.concatenate([pj, far[:, 1], [0, 200, 5]])
    c = np.zeros(len(pi), CASE)
    c["q"], c["rad"], c["p"], c["max_range"] = pos[pj], rad[pj], pos[pi], 6.0
    c["q"][::11] = c["p"][::11] + rng.uniform(-0.25, 0.25, (len(c["q"][::11]), 3))  # targets around the observer: many of these hold it
    u = beams[rng.integers(0, 16, len(pi))]
    with np.errstate(invalid="ignore"):
        aim = np.nan_to_num(pos[pj] - pos[pi]) + rng.normal(0.0, 0.3, (len(pi), 3))  # towards the target, roughly: many of these hit
    aim /= np.sqrt((aim * aim).sum(axis=1, keepdims=True))
    c["u"] = np.where((np.arange(len(pi)) % 2 == 0)[:, None], u, aim)
    # take_uav: t and best_t from a small set of values so that equal t, NaN t and inf occur often; j above, below and equal to best_j
    vals = np.array([0.0, 1.5, 1.5, 2.0, np.inf, np.nan, 4.5])
    c["t"], c["best_t"] = vals[rng.integers(0, len(vals), len(pi))], vals[rng.integers(0, len(vals) - 2, len(pi))]
    c["best_t"][::7] = np.inf
    c["j"], c["best_j"] = rng.integers(0, 6, len(pi)), rng.integers(0, 6, len(pi))
    c["best_j"][::7] = 0x7FFFFFFF
    exact = [((5.0, 0, 0), 0.5, (0, 0, 0), X, 4.5), ((5.0, 0, 0), 0.5, (0, 0, 0), X, np.nextafter(4.5, 5.0)), ((5.0, 0, 0), 0.5, (0, 0, 0), NEG_X, 9.0),
             ((0, 0, 0), 0.5, (0.25, 0, 0), Y, 9.0), ((0, 0, 0), 0.5, (0.5, 0, 0), X, 9.0), ((0, 0, 2.0), 0.5, (0, 0, 5.0), DOWN, 9.0)]
    ex = np.zeros(len(exact), CASE)
    for k, (q, rd, p, uu, mr) in enumerate(exact):
        ex[k]["q"], ex[k]["rad"], ex[k]["p"], ex[k]["u"], ex[k]["max_range"], ex[k]["t"], ex[k]["best_t"] = q, rd, p, uu, mr, np.nan, np.inf
    cases = np.concatenate([c, ex])
    assert len(cases) > 10000
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cases.bin")
        cases.tofile(path)
        out = subprocess.run([build_math_test(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and f"ok {len(cases)} cases" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines()[:len(cases)]]
    assert all(row[0] == "1" for row in rows)  # uav_target returned the stated record
    targets = uav_targets(cases["q"], cases["rad"])
    want_g = np.array([gate(cases["p"][k:k + 1], targets[k:k + 1], cases["max_range"][k])[0, 0] for k in range(len(cases))])
    assert np.array_equal(np.array([int(row[1]) for row in rows]), want_g.astype(int)) and 0.2 < want_g.mean() < 0.8
    got_t = np.array([int(row[2], 16) for row in rows], np.uint64).view(np.float64)
    want_t = ray(cases["p"], cases["u"][:, None, :], targets)[:, 0]
    bad = np.flatnonzero(got_t.view(np.int64) != want_t.view(np.int64))
    assert not len(bad), (len(bad), bad[:5], got_t[bad[:5]], want_t[bad[:5]])
    assert (want_t == 0).sum() > 50 and np.isinf(want_t).sum() > 1000 and ((want_t > 0) & np.isfinite(want_t)).sum() > 1000
    assert list(want_t[-6:]) == [4.5, 4.5, np.inf, 0.0, 0.0, 2.5] and list(want_g[-6:]) == [False, True, True, True, True, True]
    # take_uav: the lexicographic update; a NaN t is never taken, an equal t goes to the lower index
    t, bt, j, bj = cases["t"], cases["best_t"], cases["j"], cases["best_j"]
    with np.errstate(invalid="ignore"):
        take = (t < bt) | ((t == bt) & (j < bj))
    got_bt = np.array([int(row[3], 16) for row in rows], np.uint64).view(np.float64)
    got_bj = np.array([int(row[4]) for row in rows])
    assert same_bits(got_bt, np.where(take, t, bt)) and np.array_equal(got_bj, np.where(take, j, bj))
    assert not take[np.isnan(t)].any() and (take & (t == bt)).sum() > 100 and (~take & (t == bt)).sum() > 100


# ---- tests: the ABI ----

NAME = "mrs_swarm_range_scan_uavs_device"


def test_symbol_is_declared_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import build, swarm, tensors
    L = C.CDLL(swarm.LIB_PATH)
    assert re.search(r"\bint\s+" + NAME + r"\(", abi_header())
    assert hasattr(L, NAME) and NAME in swarm.ABI_SYMBOLS
    assert callable(getattr(swarm.Swarm, "range_scan_uavs_device", None)) and callable(getattr(tensors, "range_scan_uavs", None))
    assert ("range_scan_uavs.hip", "off") in build.UNITS and {"range_scan_math.h", "range_scan_common.h", "nn_hash.h"} <= set(build.DEPS)
    facade = open(os.path.join(ROOT, "include", "mrs_multirotor_simulator", "uav_system", "uav_system.hpp")).read()
    assert re.search(r"\brangeScanUavsDevice\(", facade)


def test_header_prototype_argtypes_and_method_agree(mrs):
    from mrs_multirotor_simulator_amd import swarm, tensors
    L = swarm.load_library()
    names = ["s", "first", "count", "max_range", "flags", "dev_ranges", "dtype", "stride", "dev_hit", "hit_stride", "dev_uav", "uav_stride", "ext_stream"]
    got_names, types = abi_prototype(NAME)
    assert got_names == names
    got = [C.c_void_p if issubclass(a, C._Pointer) else a for a in getattr(L, NAME).argtypes]
    assert [TYPES[t] for t in types] == got, types
    assert list(inspect.signature(swarm.Swarm.range_scan_uavs_device).parameters) == ["self"] + names[1:]
    vals = {k: int(v) for k, v in re.findall(r"\b(MRS_UAVSCAN_[A-Z0-9_]+)\s*=\s*(-?[0-9]+)", abi_header())}
    assert vals == {"MRS_UAVSCAN_HIT_UAV": HIT_UAV}
    assert swarm.UAVSCAN_HIT_UAV == tensors.UAVSCAN_HIT_UAV == HIT_UAV
    assert HIT_UAV not in (HIT_NONE, HIT_GROUND) and BODY_FRAME == swarm.SCAN_BODY_FRAME and GROUND == swarm.SCAN_GROUND


# ---- tests: the tensor layer without a GPU ----

class _Swarm(stand_in("range_scan_uavs_device", "range_scan_device")):
    beams = 16

    def scan_beam_count(self):
        return self.beams


def test_range_scan_uavs_refuses_before_the_library(monkeypatch):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, i32 = _Swarm(), torch.int32
    cases = [
        (dict(out=torch.zeros(100, 16)), "is on cpu"),
        (dict(out=on(torch.zeros(100, 16), 1)), "the swarm lives on cuda:0"),
        (dict(out=on(torch.zeros(100, 15))), r"expected a \[100, >= 16\] matrix"),
        (dict(out=on(torch.zeros(100, 16, dtype=torch.float16))), "dtype must be torch.float32 or torch.float64"),
        (dict(out=on(torch.zeros(100, 32)[:, ::2])), "rows are not contiguous"),
        (dict(hits=on(torch.zeros(100, 15, dtype=i32))), r"expected a \[100, >= 16\] matrix"),
        (dict(hits=on(torch.zeros(100, 16, dtype=torch.int64))), "expected torch.int32"),
        (dict(hits=3), "expected a torch.Tensor"),
        (dict(uavs=on(torch.zeros(100, 15, dtype=i32))), r"expected a \[100, >= 16\] matrix"),
        (dict(uavs=on(torch.zeros(99, 16, dtype=i32))), r"expected a \[100, >= 16\] matrix"),
        (dict(uavs=on(torch.zeros(100, 16, dtype=torch.int64))), "expected torch.int32"),
        (dict(uavs=torch.zeros(100, 16, dtype=i32)), "is on cpu"),
        (dict(uavs=on(torch.zeros(100, 16, dtype=i32), 1)), "the swarm lives on cuda:0"),
        (dict(uavs="all"), "expected a torch.Tensor"),
        (dict(first=10, count=50, uavs=on(torch.zeros(90, 16, dtype=i32))), r"expected a \[50, >= 16\] matrix"),
    ]
    for kw, msg in cases:
        args = dict(out=on(torch.zeros(100, 16)))
        args.update(kw)
        if "count" in kw:
            args["out"] = on(torch.zeros(50, 16))
        with pytest.raises(ValueError, match=msg):
            T.range_scan_uavs(g, 10.0, **args)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "far"):
        with pytest.raises(ValueError, match="max_range must be a finite number > 0"):
            T.range_scan_uavs(g, bad, out=on(torch.zeros(100, 16)))
    none = _Swarm()
    none.beams = 0
    with pytest.raises(ValueError, match="no beam pattern set"):
        T.range_scan_uavs(none, 10.0, out=on(torch.zeros(100, 16)))
    monkeypatch.setattr(T, "_stream", lambda dev: 1234)
    with pytest.raises(AssertionError, match="range_scan_uavs_device"):
        T.range_scan_uavs(g, np.float32(10.0), out=on(torch.zeros(100, 16)))
    calls = []

    class Taking(_Swarm):
        def range_scan_uavs_device(self, *a):
            calls.append(a)

    out, hits, uavs = on(torch.zeros(60, 40, dtype=torch.float64)), on(torch.zeros(60, 19, dtype=i32)), on(torch.zeros(60, 23, dtype=i32))
    r, h, w = T.range_scan_uavs(Taking(), 12.5, body_frame=False, ground=True, first=7, count=60, out=out, hits=hits, uavs=uavs)
    assert calls[-1] == (7, 60, 12.5, T.SCAN_GROUND, out.data_ptr(), T.DTYPE_F64, 40, hits.data_ptr(), 19, uavs.data_ptr(), 23, 1234)
    assert r.shape == (60, 16) and h.shape == (60, 16) and w.shape == (60, 16)
    out = on(torch.zeros(100, 16))
    r, h, w = T.range_scan_uavs(Taking(), 3.0, out=out)  # the defaults: body frame, no ground, no hits, no uavs
    assert h is None and w is None and calls[-1] == (0, 100, 3.0, T.SCAN_BODY_FRAME, out.data_ptr(), T.DTYPE_F32, 16, 0, 0, 0, 0, 1234)
    r, h, w = T.range_scan_uavs(Taking(), 3.0, out=out, uavs=on(torch.zeros(100, 16, dtype=i32)))  # uavs without hits
    assert h is None and w is not None and calls[-1][7:9] == (0, 0) and calls[-1][10] == 16


def test_range_scan_uavs_test_compiles(mrs):
    """tests/cpp/range_scan_uavs_test.cpp builds against the facade and the HIP runtime (run on the GPU by test_range_scan_uavs_gpu.py)"""
    from test_device_io_gpu import build_cpp
    assert os.path.exists(build_cpp("range_scan_uavs_test"))
