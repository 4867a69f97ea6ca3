"""CPU-side checks of the range scans (include/mrs_swarm.h, "range scans"): the numpy restatement the GPU tests compare bits against
(restate_scan below) follows the header line by line and is checked here on its own — known answers that are exact in binary, and a
geometric check on the fixture scene that owes nothing to the ray formulas (signed distances at the reported hit points and along the
beams); the pure functions of csrc/range_scan_math.h, which the kernel calls, give the restatement's bits in
tests/cpp/range_scan_math_test.cpp under the address and undefined-behaviour sanitizers; the symbols are exported and listed, header
prototypes, ctypes argtypes and method signatures agree; the tensor wrappers refuse bad arguments before the library is reached; the
pattern helpers return unit vectors.  No pointer reaches the library."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import CTYPE, abi_header, abi_prototype, fake_cuda, stand_in
from test_obstacles import ALL_WORLDS, BOX, CYLINDER, OBSTACLE, SPHERE, _mn, _mx, fixture_scene, obstacles, same_bits, signed_distances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BODY_FRAME, GROUND = 1, 2
HIT_NONE, HIT_GROUND = -1, -2
MAX_BEAMS = 4096
TYPES = dict(CTYPE, **{"double*": C.c_void_p, "const double*": C.c_void_p, "int32_t*": C.c_void_p, "const mrs_swarm_t*": C.c_void_p})
INF = np.float64(np.inf)


# ---- the numpy restatement (used by test_range_scan_gpu.py) ----

def beam_directions(beams, R, body_frame):
    """u [n, B, 3]: the beams as they are, or under body_frame u_c = (R[c][0]*bx + R[c][1]*by) + R[c][2]*bz"""
    beams = np.asarray(beams, np.float64).reshape(-1, 3)
    n = len(R)
    if not body_frame:
        return np.broadcast_to(beams[None], (n, len(beams), 3))
    R = np.asarray(R, np.float64).reshape(n, 3, 3)
    bx, by, bz = (beams[None, :, a] for a in range(3))
    return np.stack([(R[:, c, 0, None] * bx + R[:, c, 1, None] * by) + R[:, c, 2, None] * bz for c in range(3)], axis=-1)


def bounding_half_extents(ob):
    """hb [M, 3]: sphere (r, r, r), box h, cylinder (r, r, hz)"""
    h, kind = ob["h"], ob["kind"]
    return np.stack([h[:, 0], np.where(kind == BOX, h[:, 1], h[:, 0]), np.where(kind == SPHERE, h[:, 0], h[:, 2])], axis=1)


def gate(p, ob, max_range):
    """[n, M]: is obstacle m a candidate of a UAV at p — |d_a| - hb_a < max_range on every axis"""
    with np.errstate(all="ignore"):
        return ((np.abs(p[:, None, :] - ob["c"][None]) - bounding_half_extents(ob)[None]) < np.float64(max_range)).all(axis=-1)


def _slab(d, u, h, enter, exit, miss):
    par = u == 0.0
    t1, t2 = (-h - d) / u, (h - d) / u
    miss = miss | (par & (np.abs(d) > h))
    return np.where(par, enter, _mx(enter, _mn(t1, t2))), np.where(par, exit, _mn(exit, _mx(t1, t2))), miss


@np.errstate(all="ignore")
def ray(p, u, o):
    """t [P, B] of P (position, obstacle) pairs with B directions each: p [P, 3], u [P, B, 3], o [P] records; +inf: a miss.  The stated
    arithmetic, every operation a separately rounded numpy FP64 one, the kinds and the branches selected by where."""
    d = p - o["c"]
    dx, dy, dz = (d[:, a, None] for a in range(3))
    ux, uy, uz = (u[..., a] for a in range(3))
    h0, h1, h2 = (o["h"][:, a, None] for a in range(3))
    kind = o["kind"][:, None]
    zero = np.zeros(ux.shape)
    no = np.zeros(ux.shape, bool)
    # sphere
    cc = (((dx * dx) + dy * dy) + dz * dz) - h0 * h0
    b = ((dx * ux) + dy * uy) + dz * uz
    disc = b * b - cc
    t_s = np.where(cc <= 0.0, 0.0, np.where((b < 0.0) & (disc >= 0.0), cc / (-b + np.sqrt(disc)), INF))
    # box
    enter, exit, miss = _slab(dx, ux, h0, zero, zero + INF, no)
    enter, exit, miss = _slab(dy, uy, h1, enter, exit, miss)
    enter, exit, miss = _slab(dz, uz, h2, enter, exit, miss)
    t_b = np.where(~miss & (enter <= exit), enter, INF)
    # cylinder
    enter, exit, miss = _slab(dz, uz, h2, zero, zero + INF, no)
    a = (ux * ux) + uy * uy
    cc = ((dx * dx) + dy * dy) - h0 * h0
    vertical, within = a == 0.0, cc <= 0.0
    b = (dx * ux) + dy * uy
    disc = b * b - a * cc
    q = -b + np.sqrt(disc)
    miss = miss | np.where(vertical, ~within, ~(disc >= 0.0) | (~within & ~(b < 0.0)))
    enter = np.where(~vertical & ~within, _mx(enter, cc / q), enter)
    exit = np.where(~vertical, _mn(exit, q / a), exit)
    t_c = np.where(~miss & (enter <= exit), enter, INF)
    return np.where(kind == SPHERE, t_s, np.where(kind == BOX, t_b, t_c))


@np.errstate(all="ignore")
def ground_range(pz, uz, gz):
    """pz [n, 1], uz [n, B], gz [n, 1]"""
    return np.where(pz <= gz, 0.0, np.where(uz < 0.0, (pz - gz) / (-uz), INF))


@np.errstate(all="ignore")
def restate_scan(pos, R, worlds, ob, beams, max_range, body_frame=True, ground_z=None, chunk=1 << 21, base=None):
    """The contract of mrs_swarm_range_scan_device for every UAV: (ranges [n, B] FP64, hit [n, B] int32).  pos [n, 3]; R [n, 3, 3] or
    None (identity); worlds [n] or None (all 0); ground_z [n] (the plane of each UAV's airframe) or None: without MRS_SCAN_GROUND.
    The candidates of a UAV are formed from the gate alone (no grid), every candidate is tested, and the smallest range below max_range
    wins, ties to the lowest index.  base: the result of the same call without ground_z, which is then not computed again."""
    pos = np.asarray(pos, np.float64)
    n, M = len(pos), (len(ob) if base is None else 0)
    beams = np.asarray(beams, np.float64).reshape(-1, 3)
    B = len(beams)
    max_range = np.float64(max_range)
    worlds = np.zeros(n, np.int32) if worlds is None else np.asarray(worlds).astype(np.int32)
    if R is None:
        R = np.broadcast_to(np.eye(3), (n, 3, 3))
    u = beam_directions(beams, R, body_frame)
    finite = np.isfinite(pos).all(axis=1)
    ranges = np.full((n, B), max_range)
    hit = np.full((n, B), HIT_NONE, np.int32)
    if base is not None:
        ranges, hit = base[0].copy(), base[1].copy()
    if M:
        applies = ((ob["flags"] & ALL_WORLDS) != 0)[None, :] | (ob["world"][None, :] == worlds[:, None])
        pi, pm = np.nonzero(applies & gate(pos, ob, max_range) & finite[:, None])  # ascending (UAV, obstacle index)
        per = max(1, chunk // max(B, 1))
        cut = 0
        while cut < len(pi):
            end = min(cut + per, len(pi))
            if end < len(pi):  # whole UAVs only
                end = int(np.searchsorted(pi, pi[end], side="left"))
                if end == cut:
                    end = int(np.searchsorted(pi, pi[cut], side="right"))
            i, m = pi[cut:end], pm[cut:end]
            t = ray(pos[i], u[i], ob[m])
            t = np.where(np.isnan(t), INF, t)  # (a NaN misses)
            uav, starts, inv = np.unique(i, return_index=True, return_inverse=True)
            tmin = np.minimum.reduceat(t, starts, axis=0)
            imin = np.minimum.reduceat(np.where(t == tmin[inv], m[:, None], np.int64(1) << 40), starts, axis=0)
            won = tmin < max_range
            ranges[uav] = np.where(won, tmin, max_range)
            hit[uav] = np.where(won, imin, HIT_NONE)
            cut = end
    if ground_z is not None:
        tg = ground_range(pos[:, 2, None], u[..., 2], np.asarray(ground_z, np.float64).reshape(n, 1))
        won = (tg < ranges) & finite[:, None]
        ranges = np.where(won, tg, ranges)
        hit = np.where(won, HIT_GROUND, hit).astype(np.int32)
    return ranges, hit


def mixed_beams(nb, seed=11):
    """nb unit vectors: the axes (beams with zero components take the parallel branches in the world frame), two exact diagonals, then
    random directions"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(max(nb, 8), 3))
    v /= np.sqrt((v * v).sum(axis=1, keepdims=True))
    head = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [0.6, 0.8, 0.0], [0.0, -0.6, -0.8], [-1.0, 0.0, 0.0]])
    v[:len(head)] = head
    return np.ascontiguousarray(v[:nb])


# ---- tests: the restatement ----

def one(p, ob, b, max_range=100.0, **kw):
    r, h = restate_scan(np.atleast_2d(np.asarray(p, np.float64)), kw.pop("R", None), kw.pop("worlds", None), ob, np.atleast_2d(np.asarray(b, np.float64)),
                        max_range, **kw)
    return r[0], h[0]


def test_restatement_known_answers_per_kind():
    inf = np.inf
    X, Y, Z, DOWN = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)
    sph = obstacles([(SPHERE, (5.0, 0.0, 0.0), (1.0, 0, 0))])
    box = obstacles([(BOX, (5.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    cyl = obstacles([(CYLINDER, (0.0, 0.0, 0.0), (1.0, 0, 2.0))])
    pil = obstacles([(CYLINDER, (5.0, 0.0, 0.0), (1.0, 0, inf))])
    for ob in (sph, box, pil):
        r, h = one((0, 0, 0), ob, [X, (-1.0, 0.0, 0.0), Y])
        assert list(r) == [4.0, 100.0, 100.0] and list(h) == [0, HIT_NONE, HIT_NONE]
    for z in (-1e30, 0.0, 7.0, 1e30):  # a pillar seen horizontally, at any height
        assert one((0, 0, z), pil, [X])[0][0] == 4.0
    r, h = one((0, 0, 10.0), cyl, [DOWN, Z, X])  # a cylinder's cap from above
    assert list(r) == [8.0, 100.0, 100.0] and list(h) == [0, -1, -1]
    assert one((3.0, 0, 1.5), cyl, [(-1.0, 0.0, 0.0)])[0][0] == 2.0  # its wall from the side
    # an origin inside each kind, and on a surface pointing away: 0.0
    for ob, inside, surface in ((sph, (5.25, 0.5, 0), (6.0, 0, 0)), (box, (5.5, -0.5, 0.25), (6.0, 0.5, 0)), (cyl, (0.5, 0, -1.0), (1.0, 0, 0)),
                                (pil, (5.5, 0, 1e6), (6.0, 0, -3.0))):
        r, h = one(inside, ob, [X, Y, Z, DOWN, (-0.6, 0.0, 0.8)])
        assert same_bits(r, np.zeros(5)) and (h == 0).all()
        r, h = one(surface, ob, [X])
        assert same_bits(r, [0.0]) and h[0] == 0
    assert one((0.5, 0, 2.0), cyl, [Z])[0][0] == 0.0 and one((0.5, 0, np.nextafter(2.0, 3.0)), cyl, [Z])[1][0] == HIT_NONE  # on / above the cap
    # a beam parallel to a box face: inside the slab, outside it, exactly on the face (closed: hits)
    r, h = one((0, 0.5, 0), box, [X])
    assert r[0] == 4.0 and h[0] == 0
    assert one((0, 1.5, 0), box, [X])[1][0] == HIT_NONE
    r, h = one((0, 1.0, -1.0), box, [X])
    assert r[0] == 4.0 and h[0] == 0
    assert one((0, np.nextafter(1.0, 2.0), 0), box, [X])[1][0] == HIT_NONE
    # a vertical beam inside and outside a cylinder's radius, and on it
    assert one((0.5, 0.5, 10.0), cyl, [DOWN])[0][0] == 8.0 and one((0.0, 1.0, 10.0), cyl, [DOWN])[0][0] == 8.0
    assert one((0.8, 0.8, 10.0), cyl, [DOWN])[1][0] == HIT_NONE and one((0.0, np.nextafter(1.0, 2.0), 10.0), cyl, [DOWN])[1][0] == HIT_NONE
    assert one((5.5, 0.5, 1e9), pil, [DOWN, Z])[0].tolist() == [0.0, 0.0]  # inside a pillar: vertical beams never leave it
    # from above the axis at a slant: the beam leaves the radius before it is down at the cap, a steeper one enters through the cap
    assert one((0.0, 0.0, 6.0), cyl, [(0.0, -0.6, -0.8)])[1][0] == HIT_NONE
    r, h = one((0.0, 0.0, 3.0), cyl, [(0.0, -0.6, -0.8)])
    assert r[0] == (2.0 - 3.0) / -0.8 and abs(r[0] - 1.25) < 1e-15 and h[0] == 0
    # a sphere seen at an angle: 3-4-5
    assert one((0, 0, 0), obstacles([(SPHERE, (3.0, 4.0, 0.0), (2.5, 0, 0))]), [(0.6, 0.8, 0.0)])[0][0] == 2.5
    # the body frame: a quarter turn about z takes +x to +y
    Rz = np.array([[[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]])
    oy = obstacles([(BOX, (0.0, 5.0, 0.0), (1.0, 1.0, 1.0))])
    assert one((0, 0, 0), oy, [X], R=Rz)[0][0] == 4.0 and one((0, 0, 0), oy, [X], R=Rz, body_frame=False)[1][0] == HIT_NONE


def test_restatement_selection_rules():
    X, DOWN = (1.0, 0.0, 0.0), (0.0, 0.0, -1.0)
    sph = obstacles([(SPHERE, (5.0, 0.0, 0.0), (1.0, 0, 0))])
    # t == max_range exactly is a miss; one ulp more range hits
    r, h = one((0, 0, 0), sph, [X], max_range=4.0)
    assert r[0] == 4.0 and h[0] == HIT_NONE
    r, h = one((0, 0, 0), sph, [X], max_range=np.nextafter(4.0, 5.0))
    assert r[0] == 4.0 and h[0] == 0
    # two obstacles at equal t: the lower index wins, whatever the kinds; a nearer one wins whatever its index
    two = obstacles([(BOX, (9.0, 0.0, 0.0), (1.0, 1.0, 1.0)), (SPHERE, (5.0, 0.0, 0.0), (1.0, 0, 0)), (BOX, (5.0, 0.0, 0.0), (1.0, 2.0, 2.0)),
                     (CYLINDER, (5.0, 0.0, 0.0), (1.0, 0, np.inf))])
    r, h = one((0, 0, 0), two, [X])
    assert r[0] == 4.0 and h[0] == 1
    assert one((0, 0, 0), two[[0, 3, 2, 1]], [X])[1][0] == 1 and one((0, 0, 0), two[[2, 0]], [X])[1][0] == 0
    # ground against an obstacle at equal t: the obstacle wins; nearer ground wins; ground below max_range only
    slab = obstacles([(BOX, (0.0, 0.0, 0.5), (1.0, 1.0, 0.5))])  # top face at z = 1
    r, h = one((0, 0, 3.0), slab, [DOWN], ground_z=[1.0])
    assert r[0] == 2.0 and h[0] == 0
    r, h = one((0, 0, 3.0), slab, [DOWN], ground_z=[1.5])
    assert r[0] == 1.5 and h[0] == HIT_GROUND
    r, h = one((0, 0, 3.0), slab[:0], [DOWN, X, (0.0, 0.6, -0.8)], ground_z=[-1.0], max_range=4.5)
    assert list(r) == [4.0, 4.5, 4.5] and list(h) == [HIT_GROUND, HIT_NONE, HIT_NONE]  # 4 / 0.8 = 5 is past max_range
    r, h = one((0, 0, 3.0), slab[:0], [DOWN], ground_z=[-1.0], max_range=4.0)
    assert r[0] == 4.0 and h[0] == HIT_NONE
    # at or below the plane: 0.0 on every beam, upward ones included
    r, h = one((0, 0, -2.0), slab[:0], [DOWN, X, (0.0, 0.0, 1.0)], ground_z=[-2.0])
    assert same_bits(r, np.zeros(3)) and (h == HIT_GROUND).all()
    # worlds: the label must match unless the obstacle carries ALL_WORLDS
    ob = obstacles([(SPHERE, (5.0, 0, 0), (1.0, 0, 0), 0), (SPHERE, (4.0, 0, 0), (1.0, 0, 0), 5), (SPHERE, (7.0, 0, 0), (1.0, 0, 0), -3, ALL_WORLDS)])
    r, h = restate_scan(np.zeros((3, 3)), None, [0, 5, 9], ob, [X], 50.0, body_frame=False)
    assert list(r[:, 0]) == [4.0, 3.0, 6.0] and list(h[:, 0]) == [0, 1, 2]
    # a non-finite position: max_range and HIT_NONE on every beam, ground or not
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.0, 0.0, 0.0]])
    r, h = restate_scan(bad, None, None, sph, [X, DOWN], 50.0, ground_z=np.full(4, -1.0))
    assert (r[:3] == 50.0).all() and (h[:3] == HIT_NONE).all() and list(r[3]) == [4.0, 1.0] and list(h[3]) == [0, HIT_GROUND]
    # the gate: an obstacle whose bounding box is max_range away on an axis is no candidate, a hit just inside is one
    far = obstacles([(SPHERE, (5.0, 0.0, 0.0), (1.0, 0, 0))])
    assert not gate(np.zeros((1, 3)), far, 4.0)[0, 0] and gate(np.zeros((1, 3)), far, np.nextafter(4.0, 5.0))[0, 0]
    e = restate_scan(np.zeros((2, 3)), None, None, far[:0], [X], 5.0)
    assert (e[0] == 5.0).all() and (e[1] == HIT_NONE).all() and e[0].shape == (2, 1)


_geo = {}


def scene_rotations():
    import helpers
    pos, _, _ = fixture_scene()
    if "R" not in _geo:
        _geo["R"] = helpers.random_rotations(np.random.default_rng(909), len(pos)).reshape(-1, 3, 3)
        _geo["R"].setflags(write=False)
    return _geo["R"]


def test_geometric_check_independent_of_the_ray_formulas():
    """On the fixture scene, random attitudes, scan_ring(16) + scan_grid(4, 4), max_range 12: the reported hit point lies on the reported
    obstacle's surface (|sd| <= 1e-9; sd <= 1e-9 at t == 0), and 64 evenly spaced points of every beam before its range lie in no
    applicable obstacle (min sd >= -1e-9).  Only signed_distances() of test_obstacles.py is used.  1e-9 m, with coordinates <= 64 m, sizes
    >= 0.3 m and t <= 40 m: forming the point and evaluating sd round at about 1e-14; a grazing sphere hit can move t by up to about
    1e-6, which moves the point along the tangent and changes sd in second order only, below 1e-11: two orders of margin.
    Every beam of every UAV is sampled; a UAV's points are evaluated against the obstacles whose bounding box comes within
    0.5 m of the box around those points (no other obstacle can hold one of them)."""
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    R = scene_rotations()
    beams = np.concatenate([T.scan_ring(16), T.scan_grid(4, 4, np.radians(90.0), np.radians(60.0))])
    max_range, tol = 12.0, 1e-9
    ranges, hit = restate_scan(pos, R, worlds, ob, beams, max_range)
    u = beam_directions(beams, R, True)
    assert (hit >= 0).sum() > 5000 and (hit == HIT_NONE).sum() > 5000 and ((hit >= 0) & (ranges == 0.0)).sum() > 500
    assert set(ob["kind"][hit[hit >= 0]]) == {SPHERE, BOX, CYLINDER} and np.isinf(ob["h"][hit[(hit >= 0) & (ranges > 0)], 2]).any()
    assert (ranges[hit == HIT_NONE] == max_range).all() and (ranges[hit >= 0] < max_range).all()
    # the hit points, all UAVs
    i, b = np.nonzero(hit >= 0)
    m, t = hit[i, b], ranges[i, b]
    x = pos[i] + t[:, None] * u[i, b]
    sd = np.empty(len(i))
    for kind in (SPHERE, BOX, CYLINDER):  # (one obstacle per point: signed_distances of a point against its own obstacle, by kind)
        for mm in np.unique(m[ob["kind"][m] == kind]):
            sel = m == mm
            sd[sel] = signed_distances(x[sel], ob[mm:mm + 1])[0][:, 0]
    assert (np.abs(sd[t > 0]) <= tol).all(), np.abs(sd[t > 0]).max()
    assert (sd[t == 0] <= tol).all()
    applies = ((ob["flags"] & ALL_WORLDS) != 0)[None, :] | (ob["world"][None, :] == worlds[:, None])
    assert applies[i, m].all()
    # along the beams
    frac = np.arange(64) / 64.0
    hb = bounding_half_extents(ob)
    worst, checked = np.inf, 0
    for k in range(len(pos)):
        if not np.isfinite(pos[k]).all():
            assert (hit[k] == HIT_NONE).all() and (ranges[k] == max_range).all()
            continue
        s = ranges[k][:, None] * frac[None, :]  # [B, 64] in [0, t)
        pts = pos[k] + s[..., None] * u[k][:, None, :]
        lo, hi = pts.min(axis=(0, 1)), pts.max(axis=(0, 1))
        with np.errstate(invalid="ignore"):  # (a point inside a solid is inside its bounding box, which then meets the points' own box)
            near = np.flatnonzero(applies[k] & ((np.abs((lo + hi) / 2 - ob["c"]) - hb) <= (hi - lo) / 2 + 0.5).all(axis=1))
        if not len(near):
            continue
        live = np.broadcast_to(ranges[k][:, None] > 0, s.shape)  # (a beam with t == 0 has no point before its range)
        if not live.any():
            continue
        sdk = signed_distances(pts.reshape(-1, 3), ob[near])[0].min(axis=1).reshape(s.shape)
        worst = min(worst, sdk[live].min())
        checked += int(live.sum())
    assert worst >= -tol, worst
    assert checked > 5000000


# ---- tests: the pure functions of csrc/range_scan_math.h, stand-alone under the sanitizers ----

CASE = np.dtype([("o", OBSTACLE), ("p", "f8", 3), ("u", "f8", 3), ("max_range", "f8"), ("ground_z", "f8")])
_math_exe = []


def build_math_test():
    """tests/cpp/range_scan_math_test.cpp: the host compiler, no contraction, address and undefined-behaviour sanitizers"""
    if not _math_exe:
        exe = os.path.join(ROOT, "tests", "cpp", "range_scan_math_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "cpp", "range_scan_math_test.cpp"), "-o", exe])
        _math_exe.append(exe)
    return _math_exe[0]


def test_pure_functions_equal_the_restatement_bit_for_bit():
    assert CASE.itemsize == 128
    pos, worlds, ob = fixture_scene()
    R = scene_rotations()
    rng = np.random.default_rng(5)
    beams = mixed_beams(16)
    max_range = 12.0
    uavs = np.r_[0:40, 64:100, 198:204, 1000:1040]
    uavs = uavs[np.isfinite(pos[uavs]).all(axis=1)]
    cand = gate(pos[uavs], ob, max_range)
    pi, pm = np.nonzero(cand)
    # every candidate pair with three of the beams (body and world frame in turn), and as many pairs that are no candidates
    far_i, far_m = np.nonzero(~cand)
    pick = rng.choice(len(far_i), len(pi), replace=False)
    pi, pm = np.concatenate([pi, far_i[pick]]), np.concatenate([pm, far_m[pick]])
    rows = []
    for rep in range(5):
        bsel = rng.integers(0, len(beams), len(pi))
        u = beam_directions(beams, R[uavs], rep % 2 == 0)[pi, bsel]
        if rep >= 3:  # towards the obstacle, roughly: most of these hit
            with np.errstate(invalid="ignore"):
                u = np.nan_to_num(ob["c"][pm] - pos[uavs][pi]) + rng.normal(0.0, 0.4, (len(pi), 3))
            u /= np.sqrt((u * u).sum(axis=1, keepdims=True))
        c = np.zeros(len(pi), CASE)
        c["o"], c["p"], c["u"], c["max_range"], c["ground_z"] = ob[pm], pos[uavs][pi], u, max_range, rng.uniform(-3.0, 8.0, len(pi))
        rows.append(c)
    # the exact cases: parallel beams on, inside and outside faces, vertical beams, origins on surfaces, zero components
    ex = np.zeros(0, CASE)
    box, cyl = obstacles([(BOX, (5.0, 0.0, 0.0), (1.0, 1.0, 1.0))])[0], obstacles([(CYLINDER, (0.0, 0.0, 0.0), (1.0, 0, 2.0))])[0]
    pil, sph = obstacles([(CYLINDER, (5.0, 0.0, 0.0), (1.0, 0, np.inf))])[0], obstacles([(SPHERE, (5.0, 0.0, 0.0), (1.0, 0, 0))])[0]
    exact = [(box, (0, 1.0, -1.0), (1.0, 0, 0)), (box, (0, 1.5, 0), (1.0, 0, 0)), (box, (0, 0.5, 0), (1.0, 0, 0)), (box, (6.0, 0.5, 0), (1.0, 0, 0)),
             (cyl, (0.5, 0.5, 10.0), (0, 0, -1.0)), (cyl, (0.8, 0.8, 10.0), (0, 0, -1.0)), (cyl, (0.0, 1.0, 10.0), (0, 0, -1.0)),
             (cyl, (0.0, 0.0, 6.0), (0.0, -0.6, -0.8)), (cyl, (0.0, 0.0, 3.0), (0.0, -0.6, -0.8)), (cyl, (1.0, 0, 0), (1.0, 0, 0)), (cyl, (0.5, 0, 2.0), (0, 0, 1.0)),
             (pil, (0, 0, 1e30), (1.0, 0, 0)), (pil, (5.5, 0, 1e6), (0, 0, 1.0)), (pil, (0, 0, 0), (0, 0, -1.0)), (pil, (6.0, 0, -3.0), (1.0, 0, 0)),
             (sph, (0, 0, 0), (1.0, 0, 0)), (sph, (6.0, 0, 0), (1.0, 0, 0)), (sph, (5.25, 0.5, 0), (0, 1.0, 0)), (sph, (0, 0, 0), (-1.0, 0, 0)),
             (sph, (0, 1.0, 0), (1.0, 0, 0)), (sph, (0, np.nextafter(1.0, 0.0), 0), (1.0, 0, 0))]
    for o, p, u in exact:
        c = np.zeros(1, CASE)
        c["o"], c["p"], c["u"], c["max_range"], c["ground_z"] = o, p, u, 4.0, 0.0
        ex = np.concatenate([ex, c])
    cases = np.concatenate(rows + [ex])
    assert len(cases) > 20000
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cases.bin")
        cases.tofile(path)
        out = subprocess.run([build_math_test(), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and f"ok {len(cases)} cases" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    lines = out.stdout.splitlines()[:len(cases)]
    got_t = np.array([int(ln.split()[0], 16) for ln in lines], np.uint64).view(np.float64)
    got_g = np.array([int(ln.split()[1]) for ln in lines])
    got_z = np.array([int(ln.split()[2], 16) for ln in lines], np.uint64).view(np.float64)
    want_t = ray(cases["p"], cases["u"][:, None, :], cases["o"])[:, 0]
    bad = np.flatnonzero(got_t.view(np.int64) != want_t.view(np.int64))
    assert not len(bad), (len(bad), bad[:5], got_t[bad[:5]], want_t[bad[:5]])
    with np.errstate(all="ignore"):
        want_g = ((np.abs(cases["p"] - cases["o"]["c"]) - bounding_half_extents(cases["o"])) < cases["max_range"][:, None]).all(axis=1)
    assert np.array_equal(got_g, want_g.astype(int)) and 0.3 < want_g.mean() < 0.7
    want_z = ground_range(cases["p"][:, 2, None], cases["u"][:, 2, None], cases["ground_z"][:, None])[:, 0]
    assert same_bits(got_z, want_z)
    assert np.isinf(want_t).sum() > 1000 and (want_t == 0).sum() > 100 and ((want_t > 0) & np.isfinite(want_t)).sum() > 1000
    assert {int(k) for k in cases["o"]["kind"][np.isfinite(want_t) & (want_t > 0)]} == {SPHERE, BOX, CYLINDER}


# ---- tests: the ABI ----

NEW_SYMBOLS = ["mrs_swarm_set_scan_beams", "mrs_swarm_get_scan_beams", "mrs_swarm_range_scan_device"]


def test_symbols_are_declared_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import build, swarm, tensors
    L = C.CDLL(swarm.LIB_PATH)
    header = abi_header()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\(", header), name
        assert hasattr(L, name) and name in swarm.ABI_SYMBOLS, name
    for method in ("set_scan_beams", "get_scan_beams", "scan_beam_count", "range_scan_device"):
        assert callable(getattr(swarm.Swarm, method, None)), method
    for fn in ("set_scan_beams", "range_scan", "scan_ring", "scan_grid"):
        assert callable(getattr(tensors, fn, None)), fn
    assert ("range_scan.hip", "off") in build.UNITS and {"range_scan_math.h", "range_scan_common.h", "obstacle_set.h"} <= set(build.DEPS)
    facade = open(os.path.join(ROOT, "include", "mrs_multirotor_simulator", "uav_system", "uav_system.hpp")).read()
    for method in ("setScanBeams", "getScanBeams", "rangeScanDevice"):
        assert re.search(r"\b" + method + r"\(", facade), method


def test_header_prototypes_argtypes_and_methods_agree(mrs):
    from mrs_multirotor_simulator_amd import swarm, tensors
    L = swarm.load_library()
    want = {
        "mrs_swarm_set_scan_beams": ["s", "n_beams", "dirs"],
        "mrs_swarm_get_scan_beams": ["s", "capacity", "out", "n_beams"],
        "mrs_swarm_range_scan_device": ["s", "first", "count", "max_range", "flags", "dev_ranges", "dtype", "stride", "dev_hit", "hit_stride",
                                        "ext_stream"],
    }
    for name, names in want.items():
        got_names, types = abi_prototype(name)
        assert got_names == names, name
        got = [C.c_void_p if issubclass(a, C._Pointer) else a for a in getattr(L, name).argtypes]  # (a typed pointer is a pointer)
        assert [TYPES[t] for t in types] == got, (name, types)
    params = list(inspect.signature(swarm.Swarm.range_scan_device).parameters)
    assert params == ["self"] + want["mrs_swarm_range_scan_device"][1:]
    header = abi_header()
    vals = {k: int(eval(v.replace("u", ""))) for k, v in re.findall(r"\b(MRS_SCAN_[A-Z0-9_]+)\s*=\s*(-?[0-9<u ]+)", header)}
    assert vals == {"MRS_SCAN_MAX_BEAMS": MAX_BEAMS, "MRS_SCAN_BODY_FRAME": BODY_FRAME, "MRS_SCAN_GROUND": GROUND, "MRS_SCAN_HIT_NONE": HIT_NONE,
                    "MRS_SCAN_HIT_GROUND": HIT_GROUND}
    for name, v in vals.items():
        assert getattr(swarm, name[4:]) == getattr(tensors, name[4:]) == v, name


# ---- tests: the tensor layer without a GPU ----

class _Swarm(stand_in("range_scan_device", "set_scan_beams")):
    beams = 16

    def scan_beam_count(self):
        return self.beams


def test_range_scan_refuses_before_the_library(monkeypatch):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f32, i32 = _Swarm(), torch.float32, torch.int32
    cases = [
        (dict(out=torch.zeros(100, 16)), "is on cpu"),
        (dict(out=on(torch.zeros(100, 16), 1)), "the swarm lives on cuda:0"),
        (dict(out=on(torch.zeros(100, 15))), r"expected a \[100, >= 16\] matrix"),
        (dict(out=on(torch.zeros(99, 16))), r"expected a \[100, >= 16\] matrix"),
        (dict(out=on(torch.zeros(100, 16, dtype=torch.float16))), "dtype must be torch.float32 or torch.float64"),
        (dict(out=on(torch.zeros(100, 32)[:, ::2])), "rows are not contiguous"),
        (dict(hits=on(torch.zeros(100, 15, dtype=i32))), r"expected a \[100, >= 16\] matrix"),
        (dict(hits=on(torch.zeros(100, 16, dtype=torch.int64))), "expected torch.int32"),
        (dict(hits=torch.zeros(100, 16, dtype=i32)), "is on cpu"),
        (dict(hits=3), "expected a torch.Tensor"),
        (dict(first=10, count=50, out=on(torch.zeros(90, 16))), r"expected a \[50, >= 16\] matrix"),
    ]
    for kw, msg in cases:
        args = dict(out=on(torch.zeros(100, 16)))
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            T.range_scan(g, 10.0, **args)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "far"):
        with pytest.raises(ValueError, match="max_range must be a finite number > 0"):
            T.range_scan(g, bad, out=on(torch.zeros(100, 16)))
    none = _Swarm()
    none.beams = 0
    with pytest.raises(ValueError, match="no beam pattern set"):
        T.range_scan(none, 10.0, out=on(torch.zeros(100, 16)))
    monkeypatch.setattr(T, "_stream", lambda dev: 1234)
    for good in (10.0, 10, np.float32(10.0), np.float64(10.0), torch.tensor(10.0)):  # anything float() takes
        with pytest.raises(AssertionError, match="range_scan_device"):
            T.range_scan(g, good, out=on(torch.zeros(100, 16)))
    calls = []

    class Taking(_Swarm):
        def range_scan_device(self, *a):
            calls.append(a)

    out, hits = on(torch.zeros(60, 40, dtype=torch.float64)), on(torch.zeros(60, 19, dtype=i32))
    r, h = T.range_scan(Taking(), 12.5, body_frame=False, ground=True, first=7, count=60, out=out, hits=hits)
    assert calls[-1] == (7, 60, 12.5, T.SCAN_GROUND, out.data_ptr(), T.DTYPE_F64, 40, hits.data_ptr(), 19, 1234)
    assert r.shape == (60, 16) and h.shape == (60, 16)
    out = on(torch.zeros(100, 16))
    r, h = T.range_scan(Taking(), 3.0, out=out)  # the defaults: body frame, no ground, no hits
    assert h is None and calls[-1] == (0, 100, 3.0, T.SCAN_BODY_FRAME, out.data_ptr(), T.DTYPE_F32, 16, 0, 0, 1234)


def test_set_scan_beams_checks_and_pattern_helpers(monkeypatch):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = _Swarm()
    ok = mixed_beams(9)
    bad = [
        (np.zeros((3, 2)), r"dirs must have shape \[M, 3\]"),
        (np.zeros(3), r"dirs must have shape \[M, 3\]"),
        (np.array([[1.0, 0.0, np.nan]]), "dirs must be finite"),
        (np.array([[1.0, 0.0, np.inf]]), "dirs must be finite"),
        (np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]), "dirs must be unit vectors"),
        (np.array([[1.0 + 1e-8, 0.0, 0.0]]), "dirs must be unit vectors"),
        (np.array([[1e200, 0.0, 0.0]]), "dirs must be unit vectors"),
        (np.tile(ok[:1], (MAX_BEAMS + 1, 1)), "at most 4096"),
        ([["a", "b", "c"]], "expected numbers"),
    ]
    for dirs, msg in bad:
        with pytest.raises(ValueError, match=msg):
            T.set_scan_beams(g, dirs)
    with pytest.raises(AssertionError, match="set_scan_beams"):
        T.set_scan_beams(g, ok)
    got = []

    class Taking(_Swarm):
        def set_scan_beams(self, d):
            got.append(d)

    T.set_scan_beams(Taking(), torch.tensor(ok))
    assert got[-1].dtype == np.float64 and same_bits(got[-1], ok)
    T.set_scan_beams(Taking(), np.array([[1.0 + 4e-10, 0.0, 0.0]]))  # inside the 1e-9 of the squared norm
    T.set_scan_beams(Taking(), np.zeros((0, 3)))
    assert got[-1].shape == (0, 3)
    # the helpers: unit vectors the setter takes, in the documented order
    for pat in (T.scan_ring(1), T.scan_ring(16), T.scan_ring(360, 0.3), T.scan_ring(7, -1.2), T.scan_grid(4, 4, 1.5, 1.0), T.scan_grid(1, 1, 0.0, 0.0),
                T.scan_grid(64, 48, np.radians(87.0), np.radians(58.0)), T.scan_grid(1, 5, 0.0, 3.0)):
        assert pat.dtype == np.float64 and pat.ndim == 2 and pat.shape[1] == 3 and pat.flags["C_CONTIGUOUS"]
        assert (np.abs(((pat[:, 0] * pat[:, 0] + pat[:, 1] * pat[:, 1]) + pat[:, 2] * pat[:, 2]) - 1.0) <= 1e-12).all()
        T.set_scan_beams(Taking(), pat)
    ring = T.scan_ring(4)
    assert np.allclose(ring, [[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], atol=1e-15) and T.scan_ring(16).shape == (16, 3)
    assert np.allclose(T.scan_ring(8, 0.5)[:, 2], np.sin(0.5)) and np.allclose(T.scan_ring(3, 0.5)[0], [np.cos(0.5), 0, np.sin(0.5)])
    grid = T.scan_grid(3, 2, np.pi / 2, np.pi / 3)
    assert grid.shape == (6, 3) and np.allclose(grid[1], [np.cos(np.pi / 6), 0, 0.5]) and np.allclose(grid[4], [np.cos(np.pi / 6), 0, -0.5])
    assert grid[0, 1] > 0 > grid[2, 1] and grid[0, 2] > 0 > grid[3, 2]  # left to right, top row first
    assert np.allclose(T.scan_grid(1, 1, 1.0, 1.0), [[1.0, 0.0, 0.0]])
    for args in ((0,), (-3,)):
        with pytest.raises(ValueError, match="scan_ring needs"):
            T.scan_ring(*args)
    with pytest.raises(ValueError, match="scan_grid needs"):
        T.scan_grid(0, 4, 1.0, 1.0)


def test_range_scan_test_compiles(mrs):
    """tests/cpp/range_scan_test.cpp builds against the facade and the HIP runtime (run on the GPU by test_range_scan_gpu.py)"""
    from test_device_io_gpu import build_cpp
    assert os.path.exists(build_cpp("range_scan_test"))
