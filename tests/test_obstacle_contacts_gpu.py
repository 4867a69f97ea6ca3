"""The obstacle contacts on the GPU (mrs_swarm_obstacle_contacts_device and tensors.obstacle_contacts): every result is compared on bits
with the numpy restatement of test_obstacle_contacts.py — the fixture scene (3 072 UAVs on three airframes, 384 obstacles, two world
labels) at three margins, every combination of requested outputs, ranges that are no multiple of the block, sentinel padding and NaN
payloads in the cost vector; exact thresholds, ties and special points on hand-placed UAVs; the per-airframe radius and a stale airframe
table; independence of the grid and the three-entry grid cache; the read-only form inside a tick-rollout horizon; the marking form against
the host loop (download, restatement, Swarm.crash) on twin swarms; refusals that change nothing; the caller's stream fence; and the C++
facade (tests/cpp/obstacle_contact_test.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import helpers
from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_obstacle_contacts import MARGINS, body_radius, cost_after, fixture_contacts, fixture_radii, restate_contacts
from test_obstacles import ALL_WORLDS, BOX, CYLINDER, OBSTACLE, SPHERE, fixture_scene, obstacles, same_bits
from test_obstacles_gpu import plain_swarm, scene_swarm
from test_rollout_gpu import DT, REBOUNCE
from test_rollout_tick_cost_gpu import make_targets
from test_rollout_tick_gpu import N_PAIR, assert_same_swarm, pair_state, pair_swarm

pytestmark = pytest.mark.gpu
SENTINEL = -123.456
OUTPUTS = ("hit", "index", "sd", "counts", "cost")
FILL = dict(hit=77, index=-7, sd=SENTINEL, counts=-9)
PAYLOAD = np.array([0x7FF8000000001234], np.uint64).view(np.float64)[0]  # a NaN that is not the default one


def cost_start(count):
    """what the cost vector holds before a call: numbers, signed zeros, and a NaN payload in every third element"""
    c = np.linspace(-3.0, 5.0, count)
    c[::7] = -0.0
    c[::3] = PAYLOAD
    return c


def run_contacts(T, g, margin, crash=False, first=0, count=None, want=OUTPUTS, hit_cost=2.5, pad=3):
    """one tensors.obstacle_contacts call into the middle of sentinel-padded buffers: a dict of the requested outputs as numpy (cost: the
    vector after the call; cost0: before); the elements around the range must come back untouched"""
    import torch
    count = g.n - first if count is None else count
    dev = torch_dev(g)
    dt = dict(hit=torch.uint8, index=torch.int32, sd=torch.float64, counts=torch.int32)
    buf = {k: torch.full((count + 2 * pad,), FILL[k], dtype=dt[k], device=dev) for k in dt if k in want}
    cost0 = cost_start(count)
    if "cost" in want:  # (one host-to-device copy: the NaN payloads arrive as they are)
        buf["cost"] = torch.tensor(np.concatenate([np.full(pad, SENTINEL), cost0, np.full(pad, SENTINEL)]), dtype=torch.float64, device=dev)
    kw = {k: v[pad:pad + count] for k, v in buf.items()}
    got = T.obstacle_contacts(g, margin, crash, first, count, hit_cost=hit_cost, **kw)
    for k, t in zip(("hit", "index", "sd", "counts"), got):
        assert (t is None) == (k not in want), k
        assert t is None or t.data_ptr() == buf[k][pad:].data_ptr(), k
    out = {}
    for k, v in buf.items():
        h = v.cpu().numpy()
        fill = SENTINEL if k == "cost" else FILL[k]
        assert (h[:pad] == fill).all() and (h[pad + count:] == fill).all(), f"{k}: elements outside [0, count) were touched"
        out[k] = h[pad:pad + count]
    out["cost0"] = cost0
    return out


def check_contacts(T, g, res, margin, first=0, count=None, want=OUTPUTS, crash=False, label=""):
    count = g.n - first if count is None else count
    sl = slice(first, first + count)
    got = run_contacts(T, g, margin, crash, first, count, want)
    part = {k: v[sl] for k, v in res.items()}
    if "hit" in want:
        assert np.array_equal(got["hit"], part["hit"]), (label, "hit", first + np.flatnonzero(got["hit"] != part["hit"])[:5])
    if "counts" in want:
        assert np.array_equal(got["counts"], part["count"]), (label, "counts", first + np.flatnonzero(got["counts"] != part["count"])[:5])
    if "index" in want:
        assert np.array_equal(got["index"], part["index"]), (label, "index", first + np.flatnonzero(got["index"] != part["index"])[:5])
    if "sd" in want:
        assert same_bits(got["sd"], part["sd"]), (label, "sd", first + np.flatnonzero(got["sd"] != part["sd"])[:5])
    if "cost" in want:
        assert same_bits(got["cost"], cost_after(got["cost0"], part, 2.5)), (label, "cost")
        assert same_bits(got["cost"][part["hit"] == 0], got["cost0"][part["hit"] == 0]), (label, "cost elements of UAVs that touch nothing")
    return got


RANGES = ((0, None), (67, 1301), (255, 3), (1500, 1), (2000, 257))


@pytest.mark.parametrize("labels", [True, False], ids=["labels", "no_labels"])
def test_exact_against_numpy(mrs, labels):
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene_swarm(mrs, labels=labels)
    before = g.get_states()
    for margin in MARGINS:
        res = fixture_contacts(margin, labels)
        assert res["hit"].sum() > 500 and (res["count"] > 1).sum() > 100 and (res["hit"] == 0).sum() > 1000
        for first, count in RANGES:
            check_contacts(T, g, res, margin, first, count, label=(margin, first, count))
    # every combination of requested outputs (each changes which stores the kernel makes)
    res = fixture_contacts(0.25, labels)
    for mask in range(1, 32):
        want = tuple(k for b, k in enumerate(OUTPUTS) if mask >> b & 1)
        check_contacts(T, g, res, 0.25, 67, 1301, want=want, label=want)
    # True allocates; the defaults: margin 0, the whole swarm
    hit, index, sd, counts = T.obstacle_contacts(g, hit=True, index=True, sd=True, counts=True)
    r0 = fixture_contacts(0.0, labels)
    import torch
    assert hit.dtype == torch.uint8 and sd.dtype == torch.float64 and hit.shape == index.shape == sd.shape == counts.shape == (g.n,)
    assert np.array_equal(hit.cpu().numpy(), r0["hit"]) and np.array_equal(index.cpu().numpy(), r0["index"])
    assert same_bits(sd.cpu().numpy(), r0["sd"]) and np.array_equal(counts.cpu().numpy(), r0["count"])
    # the read-only form wrote no state: nobody is crashed, every record is what it was
    after = g.get_states()
    for key in before.dtype.names:
        assert before[key].tobytes() == after[key].tobytes(), key
    assert not np.asarray(g.has_crashed()).any()
    assert g.obstacle_stats()["grid_builds"] == len(MARGINS) + 2 and g.obstacle_stats()["cells"] == 0  # one grid per margin change; none for the queries


def test_thresholds_ties_and_special_points(mrs):
    from mrs_multirotor_simulator_amd import tensors as T
    inf = np.inf
    rad = body_radius("x500")
    margin = float(np.float64(0.75) - rad)  # thr = 0.75 exactly: a UAV at x = 1.75 is exactly thr from a surface at x = 1
    thr = rad + np.float64(margin)
    at = 1.0 + thr
    closer = np.nextafter(at, 0.0)
    assert thr == 0.75 and at - 1.0 == thr and closer - 1.0 < thr
    # (the three at x = 0: dx is the UAV's x itself, so sd = x - 1 exactly, and the y offsets are exact)
    ob = obstacles([(SPHERE, (0.0, 0.0, 0.0), (1.0, 0, 0)), (BOX, (0.0, 50.0, 0.0), (1.0, 1.0, 1.0)), (CYLINDER, (0.0, 100.0, 0.0), (1.0, 0, inf)),
                    (SPHERE, (65.0, 0.0, 0.0), (1.0, 0, 0)), (BOX, (62.0, 0.0, 0.0), (0.5, 0.5, 0.5)), (SPHERE, (65.0, 0.0, 0.0), (1.0, 0, 0)),
                    (BOX, (62.0, 0.0, 0.0), (0.5, 0.5, 0.5)),
                    (SPHERE, (80.0, 0.0, 0.0), (1.0, 0, 0)), (SPHERE, (80.0, 0.0, 0.0), (3.0, 0, 0)), (BOX, (80.0, 0.0, 0.0), (2.0, 2.0, 2.0)),
                    (SPHERE, (100.0, 0.0, 0.0), (1.0, 0, 0)), (BOX, (102.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
                    (BOX, (120.0, 0.0, 0.0), (1.0, 1.0, 1.0)), (SPHERE, (122.0, 0.0, 0.0), (1.0, 0, 0))])
    pos = np.array([[at, 0, 0], [closer, 0, 0], [at, 50.0, 0], [closer, 50.0, 0], [at, 100.0, 1e6], [closer, 100.0, -1e6],  # 0-5: at / inside thr
                    [63.5, 0, 0],                                      # 6: two pairs of identical obstacles, the spheres nearer: index 3
                    [62.0, 0, 0],                                      # 7: inside the two identical boxes: index 4
                    [80.5, 0, 0], [80.0, 0, 0],                        # 8, 9: inside overlapping solids: the deepest (8)
                    [101.0, 0, 0], [121.0, 0, 0],                      # 10, 11: on two surfaces at once: sd 0.0 twice, the lower index (the
                                                                       # stated arithmetic never gives -0.0; the fold's signed-zero
                                                                       # tie is checked in tests/cpp/obstacle_contact_math_test.cpp)
                    [np.nan, 0, 0], [80.0, inf, 0], [80.0, 0, -inf],   # 12-14: non-finite
                    [0.5, 100.0, 1e30], [at, 100.0, -1e30],            # 15, 16: the pillar without ends, inside and exactly at thr
                    [1e9, -1e9, 1e7], [-300.0, 0, 0]])                 # 17, 18: far outside the grid
    g = plain_swarm(mrs, pos)
    g.set_obstacles(ob)
    x = g.get_states()["x"]
    wider = margin + 2.0 ** -50  # (exact, and eight ulps of thr: fl(rad + wider) > thr whatever the rounding)
    assert rad + np.float64(wider) > thr
    for m in (margin, wider, 0.0, 3.0, 100.0):
        res = restate_contacts(x, None, ob, rad, m)
        got = check_contacts(T, g, res, m, label=("hand-placed", m))
    got = check_contacts(T, g, restate_contacts(x, None, ob, rad, margin), margin, label="hand-placed")
    assert list(got["hit"][:6]) == [0, 1, 0, 1, 0, 1] and list(got["index"][:6]) == [-1, 0, -1, 1, -1, 2], "sd == thr misses, one ulp closer hits"
    assert (got["sd"][:6:2] == inf).all() and list(got["counts"][:6]) == [0, 1, 0, 1, 0, 1]
    assert (got["sd"][1:6:2] == closer - 1.0).all()
    assert list(check_contacts(T, g, restate_contacts(x, None, ob, rad, wider), wider)["hit"][:6]) == [1] * 6
    assert got["index"][6] == 3 and got["counts"][6] == 2 and got["sd"][6] == 0.5, "equal sd: the lower index"
    assert got["index"][7] == 4 and got["counts"][7] == 2 and got["sd"][7] == -0.5
    wide = check_contacts(T, g, restate_contacts(x, None, ob, rad, 3.0), 3.0)
    assert wide["index"][6] == 3 and wide["counts"][6] == 4 and wide["sd"][6] == 0.5, "the nearer pair, its lower index, whatever else touches"
    assert got["index"][8] == 8 and got["counts"][8] == 3 and got["sd"][8] == -2.5 and got["index"][9] == 8 and got["counts"][9] == 3
    assert got["index"][10] == 10 and got["counts"][10] == 2 and got["sd"][10] == 0.0, "-0.0 == +0.0: the lower index"
    assert got["index"][11] == 12 and got["counts"][11] == 2 and got["sd"][11] == 0.0
    sd10 = restate_contacts(x[10:12], None, ob, rad, margin)["sd"]
    assert same_bits(got["sd"][10:12], sd10)
    assert (got["hit"][12:15] == 0).all() and (got["index"][12:15] == -1).all() and (got["sd"][12:15] == inf).all() and (got["counts"][12:15] == 0).all()
    assert got["hit"][15] == 1 and got["index"][15] == 2 and got["sd"][15] == -0.5 and got["hit"][16] == 0
    assert (got["hit"][17:] == 0).all()
    # an empty set: nobody touches, and it is no error; nor is a set that was never given
    g.set_obstacles(None)
    none = restate_contacts(x, None, ob[:0], rad, margin)
    check_contacts(T, g, none, margin, label="cleared")
    fresh = plain_swarm(mrs, pos)
    check_contacts(T, fresh, none, margin, label="never set")
    T.obstacle_contacts(fresh, margin, crash=True)
    assert not np.asarray(fresh.has_crashed()).any()


def test_per_airframe_radius_and_a_stale_table(mrs):
    """a UAV between two airframes' radii from an obstacle: its answer follows set_params changing arm_length between two calls with nothing
    else in between"""
    from mrs_multirotor_simulator_amd import tensors as T
    ob = obstacles([(SPHERE, (0.0, 0.0, 5.0), (1.0, 0, 0)), (CYLINDER, (30.0, 0.0, 0.0), (1.0, 0, np.inf))])
    pos = np.array([[1.45, 0.0, 5.0], [31.45, 0.0, 3.0], [1.45, 0.0, 5.0], [50.0, 0.0, 5.0]])  # sd = 0.45: between x500 (0.4) and t650 (0.515)
    assert body_radius("x500") < 0.45 < body_radius("t650")
    g = plain_swarm(mrs, pos)
    g.construct(2, 1, mrs.model_params("t650"), pos[2:3])
    g.set_obstacles(ob)
    x = g.get_states()["x"]
    rad = np.array([body_radius("x500"), body_radius("x500"), body_radius("t650"), body_radius("x500")])
    got = check_contacts(T, g, restate_contacts(x, None, ob, rad, 0.0), 0.0, label="two airframes")
    assert list(got["hit"]) == [0, 0, 1, 0]
    builds = g.obstacle_stats()["grid_builds"]
    p = mrs.model_params("x500")
    p.arm_length = 0.325  # (the arm of a t650 on an x500: a new entry of the airframe table)
    g.set_params(0, 2, p)
    rad2 = rad.copy()
    rad2[:2] = np.float64(0.325) + np.float64(p.prop_radius)
    got = check_contacts(T, g, restate_contacts(x, None, ob, rad2, 0.0), 0.0, label="after set_params")
    assert list(got["hit"]) == [1, 1, 1, 0] and rad2[0] > 0.45
    g.set_params(0, 1, mrs.model_params("x500"))
    rad2[0] = rad[0]
    got = check_contacts(T, g, restate_contacts(x, None, ob, rad2, 0.0), 0.0, label="and back")
    assert list(got["hit"]) == [0, 1, 1, 0]
    assert g.obstacle_stats()["grid_builds"] == builds  # the largest radius of the table did not change: the same grid served all three
    # the mark follows the same radius
    T.obstacle_contacts(g, crash=True)
    assert list(np.asarray(g.has_crashed())) == [0, 1, 1, 0]


def test_grid_independence_and_cache(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    g = scene_swarm(mrs)
    res = fixture_contacts(0.25)
    assert g.obstacle_stats()["grid_builds"] == 0
    check_contacts(T, g, res, 0.25, label="first")
    assert g.obstacle_stats()["grid_builds"] == 1 and g.obstacle_stats()["cells"] == 0  # the stats describe the queries' grid: none yet
    # one far, huge all-worlds obstacle: another set, another grid, the same answers (index 384 is never the nearest: nobody touches it)
    far = obstacles([(BOX, (5e6, -3e6, 1e5), (4e4, 9e4, 2e4), 0, ALL_WORLDS)])
    bigger = np.concatenate([ob, far])
    g.set_obstacles(bigger)
    assert (restate_contacts(pos, worlds, bigger, fixture_radii(len(pos)), 0.25)["index"] == res["index"]).all()
    check_contacts(T, g, res, 0.25, label="with a far, huge obstacle")
    assert g.obstacle_stats()["grid_builds"] == 2
    g.set_obstacles(ob)
    # an unused airframe type with a large arm in the table: a larger R, another grid, the same answers
    p = mrs.model_params("x500")
    p.arm_length = 7.5
    g.set_params(5, 1, p)
    g.set_params(5, 1, mrs.model_params("x500"))
    check_contacts(T, g, res, 0.25, label="with an unused large airframe in the table")
    assert g.obstacle_stats()["grid_builds"] == 3
    # three callers, three entries: alternating them builds each grid once
    T.set_scan_beams(g, T.scan_ring(8))
    g.set_obstacles(ob)  # (drops the contacts' entry: all three are to be built)
    b0 = g.obstacle_stats()["grid_builds"]
    cost = torch.zeros(g.n, dtype=torch.float64, device=torch_dev(g))
    for _ in range(6):
        T.obstacle_cost(g, 5.0, out=cost, accumulate=True)
        T.range_scan(g, 12.0)
        check_contacts(T, g, res, 0.25, want=("hit", "index"), label="alternating")
    st = g.obstacle_stats()
    assert st["grid_builds"] == b0 + 3 and st["grid_radius"] == 5.0  # three grids over six rounds; the stats are the queries'
    g.set_obstacles(ob[:100])  # replacing the set drops all three entries
    part = restate_contacts(pos, worlds, ob[:100], fixture_radii(len(pos)), 0.25)
    for _ in range(3):
        T.obstacle_cost(g, 5.0, out=cost, accumulate=True)
        T.range_scan(g, 12.0)
        check_contacts(T, g, part, 0.25, label="replaced set")
    assert g.obstacle_stats()["grid_builds"] == b0 + 6
    # a clone has the set and builds its own grid
    c = g.clone()
    assert c.obstacle_stats()["grid_builds"] == 0 and c.obstacle_stats()["count"] == 100
    check_contacts(T, c, part, 0.25, label="clone")
    assert c.obstacle_stats()["grid_builds"] == 1 and g.obstacle_stats()["grid_builds"] == b0 + 6
    c.close()


@pytest.mark.parametrize("crash", [False, True], ids=["elastic", "crash"])
@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
def test_read_only_form_inside_a_horizon(mrs, arith, crash):
    """rollout_tick_cost over 24 + 24 ticks with accumulate, obstacle_contacts without the mark between the halves and after (a collision
    tick is pending at both points); a twin runs the same horizon without the contact calls and adds hit_cost on the host where the
    restatement says so: final state and crash flags are the twin's bit for bit, and so is the cost vector after every piece and every call"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ar = getattr(mrs, "ARITH_" + arith)
    a, b = pair_swarm(mrs, ar), pair_swarm(mrs, ar)
    pos, _ = pair_state()
    rng = np.random.default_rng(31)
    m = 96
    ob = np.zeros(m, OBSTACLE)
    ob["kind"] = np.arange(m) % 3
    ob["c"] = pos[rng.integers(0, 64, m)] + rng.uniform(-2, 2, (m, 3))  # around the colliding pairs and their neighbours
    ob["h"] = rng.uniform(0.2, 1.5, (m, 3))
    ob["h"][5::6, 2] = np.inf
    a.set_obstacles(ob)
    dev = torch_dev(a)
    rad = body_radius("x500")
    ticks, hold = 24, 4
    groups = T.OBS_POS | T.OBS_VEL
    blocks = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (2 * ticks // hold, N_PAIR, 4))
    cmd = torch.tensor(blocks, device=dev)
    tg, wt = make_targets(rng, 2 * ticks // hold, N_PAIR, T.gather_width(groups), torch.float64, dev, False, False)
    costs = {id(a): torch.zeros(N_PAIR, dtype=torch.float64, device=dev), id(b): torch.zeros(N_PAIR, dtype=torch.float64, device=dev)}
    half = ticks // hold
    touching = 0
    for piece in range(2):
        sl = slice(piece * half, (piece + 1) * half)
        for g in (a, b):
            T.rollout_tick_cost(g, O.POSITION_CMD, cmd[sl], DT, crash, REBOUNCE, groups, tg[sl], wt[sl], 1000.0, hold=hold, out=costs[id(g)],
                                accumulate=True)
        xa = T.gather(a, T.OBS_POS, dtype=torch.float64).cpu().numpy()  # (the same calls and host waits in both runs)
        T.gather(b, T.OBS_POS, dtype=torch.float64).cpu()
        assert same_bits(costs[id(a)].cpu().numpy(), costs[id(b)].cpu().numpy()), piece
        for margin, hit_cost in ((0.25, 500.0), (1.0, 0.125)):
            before = costs[id(a)].cpu().numpy()
            res = restate_contacts(xa, None, ob, rad, margin)
            hit, index, sd, counts = T.obstacle_contacts(a, margin, hit=True, index=True, sd=True, counts=True, cost=costs[id(a)], hit_cost=hit_cost)
            assert np.array_equal(hit.cpu().numpy(), res["hit"]) and np.array_equal(index.cpu().numpy(), res["index"]), (piece, margin)
            assert same_bits(sd.cpu().numpy(), res["sd"]) and np.array_equal(counts.cpu().numpy(), res["count"]), (piece, margin)
            assert same_bits(costs[id(a)].cpu().numpy(), cost_after(before, res, hit_cost)), (piece, margin)
            touching += int(res["hit"].sum())
            costs[id(b)].copy_(torch.tensor(cost_after(costs[id(b)].cpu().numpy(), res, hit_cost), device=dev))
    assert touching > 40
    assert same_bits(costs[id(a)].cpu().numpy(), costs[id(b)].cpu().numpy())
    if crash:
        assert np.asarray(a.has_crashed()).any()
    assert_same_swarm(a, b, f"{arith} crash={crash}: with and without the contact calls")
    for g in (a, b):
        g.tick_n(DT, 1, True, crash, REBOUNCE)  # evaluates the collision tick the horizon left pending
    assert_same_swarm(a, b, f"{arith} crash={crash}: one more tick on both")


# ---- the marking form against the host loop ----

N_MARK, CHUNKS, CHUNK_TICKS, MARK_MARGIN = 208, 6, 50, 0.1


def marking_scene():
    """(pos, v, command rows, obstacles) of 208 x500s 10 m apart on a line at z = 5 m: 16 pairs flying at each other (UAV-UAV contacts during
    the horizon); UAVs 40..139 fly in +y at 5 m/s under a position command 20 m ahead, each towards a solid whose surface is between
    0.05 m and 0.95 m beyond its reach — pillars without ends (40..79), spheres (80..99) and ONE wall across the lanes of 100..139, which
    start staggered; UAVs 140..207 hover far from everything"""
    n = N_MARK
    thr = body_radius("x500") + np.float64(MARK_MARGIN)
    pos = np.stack([10.0 * np.arange(n), np.zeros(n), np.full(n, 5.0)], axis=1)
    v = np.zeros((n, 3))
    for k in range(16):
        pos[2 * k + 1, 0] = pos[2 * k, 0] + 1.5
        v[2 * k, 0], v[2 * k + 1, 0] = 15.0, -15.0
    movers = np.arange(40, 140)
    gap = 0.05 + 0.9 * (movers - 40) / 99.0 * ((movers * 7) % 10 + 1) / 10.0  # how far each flies before it touches
    rows = []
    for i, d in zip(movers, gap):
        if i < 80:
            rows.append((CYLINDER, (pos[i, 0], thr + d + 0.5, 0.0), (0.5, 0, np.inf)))
        elif i < 100:
            rows.append((SPHERE, (pos[i, 0], thr + d + 0.75, 5.0), (0.75, 0, 0)))
        else:
            pos[i, 1] = -d  # the wall is where it is: the UAV starts further back
    rows.append((BOX, (1195.0, thr + 0.05, 5.0), (215.0, 0.05, 3.0)))
    v[movers, 1] = 5.0
    cmd = np.concatenate([pos, np.zeros((n, 1))], axis=1)
    cmd[movers, 1] += 20.0
    return pos, v, cmd, obstacles(rows)


def marking_swarm(mrs, arith):
    pos, v, cmd, ob = marking_scene()
    n = len(pos)
    g = mrs.Swarm(n, arith=arith)
    g.construct(0, n, mrs.model_params("x500"), pos)
    st = g.get_states()
    g.set_state(0, n, pos, v, st["R"].reshape(n, 9), st["omega"], st["motor_rpm"])
    g.set_input(0, n, mrs.POSITION_CMD, cmd)
    g.set_obstacles(ob)
    return g


def oracle_marking_horizon(crash):
    """the horizon on the CPU oracle with the restatement as the producer of the mark: per chunk the UAVs newly marked by it"""
    pos, v, cmd, ob = marking_scene()
    n = len(pos)
    o = O.OracleSwarm(n)
    o.construct(0, n, helpers.oracle_params("x500"), pos)
    st = o.get_state()
    o.set_state(0, n, pos, v, st["R"].reshape(n, 9), st["omega"], st["motor_rpm"])
    o.set_input(0, n, O.POSITION_CMD, cmd)
    rad = body_radius("x500")
    newly, touched = [], np.zeros(n, bool)
    for _ in range(CHUNKS):
        for _ in range(CHUNK_TICKS):
            o.step(DT)
            o.handle_collisions(True, crash, REBOUNCE)
        res = restate_contacts(o.get_state()["x"], None, ob, rad, MARK_MARGIN)
        was = np.asarray(o.has_crashed()) != 0
        hit = res["hit"] != 0
        newly.append(np.flatnonzero(hit & ~was))
        touched |= hit
        for i in np.flatnonzero(hit):
            o.crash(int(i), 1)
    return newly, touched


def assert_marking_floors(newly, touched, what):
    marked = sum(len(c) for c in newly)
    assert marked >= 20, f"{what}: {marked} UAVs newly marked during the horizon"
    assert sum(len(c) > 0 for c in newly) >= 3, f"{what}: newly marked UAVs in chunks {[len(c) for c in newly]}"
    assert (~touched).sum() >= 20, f"{what}: {(~touched).sum()} UAVs never touch"


@pytest.mark.parametrize("crash", [False, True], ids=["elastic", "crash"])
@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
def test_marking_form_equals_the_host_loop(mrs, arith, crash):
    """swarm A: tick_n chunks, then obstacle_contacts(crash=True, hit=...) behind the pending collision tick; swarm B: the same chunks, then
    the positions downloaded, the numpy restatement, and Swarm.crash for each hit.  After every chunk everything is bit-identical."""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    assert_marking_floors(*oracle_marking_horizon(crash), "the scene on the CPU oracle")
    ar = getattr(mrs, "ARITH_" + arith)
    a, b = marking_swarm(mrs, ar), marking_swarm(mrs, ar)
    _, _, _, ob = marking_scene()
    n, rad = a.n, body_radius("x500")
    dev = torch_dev(a)
    hit = torch.full((n,), 77, dtype=torch.uint8, device=dev)
    newly, touched = [], np.zeros(n, bool)
    fresh, z_then = np.zeros(0, int), None
    for chunk in range(CHUNKS):
        for g in (a, b):
            g.tick_n(DT, CHUNK_TICKS, True, crash, REBOUNCE)  # (leaves a collision tick pending)
        T.obstacle_contacts(a, MARK_MARGIN, crash=True, hit=hit)
        x = b.get_states()["x"]
        was = np.asarray(b.has_crashed()) != 0
        res = restate_contacts(x, None, ob, rad, MARK_MARGIN)
        for i in np.flatnonzero(res["hit"]):
            b.crash(int(i), 1)
        assert np.array_equal(hit.cpu().numpy(), res["hit"]), (chunk, np.flatnonzero(hit.cpu().numpy() != res["hit"])[:5])
        if len(fresh):  # those marked after the previous chunk fell during this one
            assert (x[fresh, 2] < z_then).all(), (chunk, fresh[x[fresh, 2] >= z_then][:5])
        fresh = np.flatnonzero((res["hit"] != 0) & ~was)
        z_then = x[fresh, 2]
        crashed = T.crashed(a).cpu().numpy()
        assert crashed[fresh].all() and np.array_equal(crashed, np.asarray(b.has_crashed()) != 0), chunk
        assert_same_swarm(a, b, f"{arith} crash={crash}: after chunk {chunk}")
        newly.append(fresh)
        touched |= res["hit"] != 0
    assert_marking_floors(newly, touched, "the scene on the GPU")
    for g in (a, b):
        g.tick_n(DT, CHUNK_TICKS, True, crash, REBOUNCE)
    assert_same_swarm(a, b, f"{arith} crash={crash}: one more chunk on both")
    x = b.get_states()["x"]
    assert len(fresh) == 0 or (x[fresh, 2] < z_then).all()
    # with their motors stopped, the marked UAVs are below every UAV that hovers far from the obstacles
    assert x[touched, 2].max() < x[140:, 2].min() - 0.05, (x[touched, 2].max(), x[140:, 2].min())


def test_refused_calls_change_nothing(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    g = plain_swarm(mrs, pos[:300])
    g.set_obstacles(ob)
    before = g.get_states()
    dev = torch_dev(g)
    st = torch.cuda.current_stream(dev).cuda_stream
    hit = torch.full((300,), 77, dtype=torch.uint8, device=dev)
    index = torch.full((300,), -7, dtype=torch.int32, device=dev)
    sd = torch.full((300,), SENTINEL, dtype=torch.float64, device=dev)
    counts = torch.full((300,), -9, dtype=torch.int32, device=dev)
    cost = torch.full((300,), SENTINEL, dtype=torch.float64, device=dev)
    h, i, d, n, c = hit.data_ptr(), index.data_ptr(), sd.data_ptr(), counts.data_ptr(), cost.data_ptr()
    host = np.zeros(300 * 8)
    hip = C.CDLL("libamdhip64.so")
    small_p, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(small_p), C.c_size_t(4096)) == 0
    assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), small_p) == 0 and size.value < 4100
    small = small_p.value
    nan, inf = float("nan"), float("inf")
    K = T.CONTACT_CRASH
    bad = [
        ((200, 101, 0.25, K, h, i, d, n, c, 1.0), "error 3:"),
        ((-1, 10, 0.25, K, h, i, d, n, c, 1.0), "error 3:"),
        ((0, 300, 0.25, 2, h, i, d, n, c, 1.0), "error 1:.*unknown contact flag bits"),
        ((0, 300, 0.25, K | 4, h, i, d, n, c, 1.0), "error 1:.*unknown contact flag bits"),
        ((0, 300, -0.25, K, h, i, d, n, c, 1.0), "error 1:.*margin"),
        ((0, 300, nan, K, h, i, d, n, c, 1.0), "error 1:.*margin"),
        ((0, 300, inf, K, h, i, d, n, c, 1.0), "error 1:.*margin"),
        ((0, 300, 0.25, K, h, i, d, n, c, nan), "error 1:.*hit_cost"),
        ((0, 300, 0.25, 0, h, i, d, n, c, inf), "error 1:.*hit_cost"),
        ((0, 300, 0.25, 0, 0, 0, 0, 0, 0, 1.0), "error 1:.*nothing to do"),
        ((0, 0, 0.25, 0, 0, 0, 0, 0, 0, 1.0), "error 1:.*nothing to do"),
        ((0, 300, 0.25, K, host.ctypes.data, i, d, n, c, 1.0), "error 1:.*dev_hit"),
        ((0, 300, 0.25, K, h, host.ctypes.data, d, n, c, 1.0), "error 1:.*dev_index"),
        ((0, 300, 0.25, K, h, i, host.ctypes.data, n, c, 1.0), "error 1:.*dev_sd"),
        ((0, 300, 0.25, K, h, i, d, host.ctypes.data, c, 1.0), "error 1:.*dev_count"),
        ((0, 300, 0.25, K, h, i, d, n, host.ctypes.data, 1.0), "error 1:.*dev_cost"),
        ((0, 300, 0.25, K, small + 4096 - 299, i, d, n, c, 1.0), "error 1:.*dev_hit: the rows extend past"),
        ((0, 300, 0.25, K, h, small + 4096 - 1196, d, n, c, 1.0), "error 1:.*dev_index: the rows extend past"),
        ((0, 300, 0.25, K, h, i, small + 4096 - 2392, n, c, 1.0), "error 1:.*dev_sd: the rows extend past"),
        ((0, 300, 0.25, K, h, i, d, small + 4096 - 1196, c, 1.0), "error 1:.*dev_count: the rows extend past"),
        ((0, 300, 0.25, 0, h, i, d, n, small + 4096 - 2392, 1.0), "error 1:.*dev_cost: the rows extend past"),
    ]
    torch.cuda.synchronize(dev)
    for args, msg in bad:
        with pytest.raises(mrs.MrsError, match=msg):
            g.obstacle_contacts_device(*args, st)
    # fl(rmax + margin) that is not > 0.  A swarm's airframe table holds the default airframe from its creation on and every margin is
    # finite and >= 0, so the sum is finite and > 0 for every swarm that has a UAV; what is left is a swarm without UAVs (an empty
    # table, rmax = 0) at margin 0
    nobody = mrs.Swarm(0)
    nobody.set_obstacles(ob)
    for flags in (0, K):
        with pytest.raises(mrs.MrsError, match="error 1:.*largest body radius"):
            nobody.obstacle_contacts_device(0, 0, 0.0, flags, h, i, d, n, c, 1.0, st)
    nobody.obstacle_contacts_device(0, 0, 0.25, K, h, i, d, n, c, 1.0, st)  # (count == 0 after the checks)
    assert nobody.obstacle_stats()["grid_builds"] == 0
    nobody.close()
    torch.cuda.synchronize(dev)
    assert hip.hipFree(C.c_void_p(small)) == 0

    def untouched():
        return ((hit.cpu().numpy() == 77).all() and (index.cpu().numpy() == -7).all() and (sd.cpu().numpy() == SENTINEL).all()
                and (counts.cpu().numpy() == -9).all() and (cost.cpu().numpy() == SENTINEL).all())

    assert untouched() and g.obstacle_stats()["grid_builds"] == 0  # nothing was launched, no grid was built
    # count == 0 is MRS_OK and writes nothing
    g.obstacle_contacts_device(0, 0, 0.25, K, h, i, d, n, c, 1.0, st)
    g.obstacle_contacts_device(300, 0, 0.25, K, 0, 0, 0, 0, 0, 0.0, st)
    g.obstacle_contacts_device(300, 0, 0.25, 0, h, 0, 0, 0, 0, 0.0, st)
    assert untouched() and g.obstacle_stats()["grid_builds"] == 0
    after = g.get_states()
    for key in before.dtype.names:
        assert before[key].tobytes() == after[key].tobytes(), key
    assert not np.asarray(g.has_crashed()).any()
    # a sharded swarm
    group = mrs.LoopbackGroup(2)
    shards = []
    for rk in range(2):
        s = mrs.Swarm(100)
        s.construct(0, 100, mrs.model_params("x500"), np.stack([np.arange(100) * 3.0 + 400 * rk, np.zeros(100), np.full(100, 5.0)], axis=1))
        s.comm_init_loopback(group, rk, 200)
        s.set_obstacles(ob[:10])  # (the set itself is legal there)
        shards.append(s)
    for s in shards:
        for crash in (False, True):
            with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
                T.obstacle_contacts(s, 0.25, crash, hit=hit[:100], cost=cost[:100])
    assert untouched()
    for s in shards:
        s.close()
    group.close()


def test_caller_stream_is_fenced(mrs):
    """the outputs are filled on a side stream kept busy by a long sleep, then the call is made with that stream current: the cost vector must
    hold fill + hit_cost where touching (the kernel ran after the fill), the other outputs the result (not the fill); copies queued behind
    the call on the side stream read them, and so does another stream that waits for the side stream"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene_swarm(mrs)
    dev = torch_dev(g)
    res = fixture_contacts(0.25)
    hit = torch.zeros(g.n, dtype=torch.uint8, device=dev)
    index = torch.zeros(g.n, dtype=torch.int32, device=dev)
    sd = torch.zeros(g.n, dtype=torch.float64, device=dev)
    counts = torch.zeros(g.n, dtype=torch.int32, device=dev)
    cost = torch.zeros(g.n, dtype=torch.float64, device=dev)
    T.obstacle_contacts(g, 0.25, hit=True)  # (the grid is built: the fenced call launches and nothing else)
    torch.cuda.synchronize(dev)
    side, other = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        hit.fill_(77)
        index.fill_(-7)
        sd.fill_(SENTINEL)
        counts.fill_(-9)
        cost.fill_(2.5)
        T.obstacle_contacts(g, 0.25, hit=hit, index=index, sd=sd, counts=counts, cost=cost, hit_cost=40.0)
        copies = [t.clone() for t in (hit, index, sd, counts, cost)]
    other.wait_stream(side)
    with torch.cuda.stream(other):
        second = [t.clone() for t in (hit, index, sd, counts, cost)]
    side.synchronize()
    other.synchronize()
    for got in (copies, second):
        h, i, s, n, c = (t.cpu().numpy() for t in got)
        assert np.array_equal(h, res["hit"]) and np.array_equal(i, res["index"]) and same_bits(s, res["sd"]) and np.array_equal(n, res["count"])
        assert same_bits(c, cost_after(np.full(g.n, 2.5), res, 40.0))


def test_cpp_facade_equals_python(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, m = 2000, 60
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "contacts.bin")
        out = subprocess.run([build_cpp("obstacle_contact_test"), path], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok contacts_equal_brute_force", "ok written"):
            assert tag in out.stdout, out.stdout
        raw = open(path, "rb").read()
    o = 0
    chit = np.frombuffer(raw, np.uint8, n, o)
    o += n
    cidx = np.frombuffer(raw, np.int32, n, o)
    o += 4 * n
    csd = np.frombuffer(raw, np.float64, n, o)
    o += 8 * n
    ccnt = np.frombuffer(raw, np.int32, n, o)
    o += 4 * n
    ccost = np.frombuffer(raw, np.float64, n, o)
    o += 8 * n
    ccrashed = np.frombuffer(raw, np.uint8, n, o)
    i = np.arange(n)
    pos = np.stack([3.1 * (i % 20) + 0.01 * (i % 7), 2.9 * ((i // 20) % 20) - 0.02 * (i % 5), 3.3 * (i // 400) + 0.005 * (i % 11)], axis=1)
    j = np.arange(m)
    ob = np.zeros(m, OBSTACLE)
    ob["kind"] = j % 3
    ob["c"] = np.stack([6.2 * (j % 8) + 0.5, 7.1 * ((j // 8) % 8) - 0.25, 3.0 + 1.5 * (j % 4)], axis=1)
    ob["h"] = np.stack([1.4 + 0.3 * (j % 5), 1.3 + 0.4 * (j % 3), np.where(j % 6 == 2, np.inf, 2.0 + 0.5 * (j % 4))], axis=1)
    g = mrs.Swarm(n)
    g.construct(0, n, mrs.model_params("x500"), pos)
    g.set_obstacles(ob)
    cost0 = 0.5 * i
    bits = cost0.view(np.uint64)
    bits[::3] = np.uint64(0x7FF8000000000000) | (i[::3] + 1).astype(np.uint64)
    cost = torch.tensor(cost0, dtype=torch.float64, device=torch_dev(g))
    assert same_bits(cost.cpu().numpy(), cost0)
    hit, index, sd, counts = T.obstacle_contacts(g, 1.0, hit=True, index=True, sd=True, counts=True, cost=cost, hit_cost=1000.0)
    assert np.array_equal(hit.cpu().numpy(), chit) and np.array_equal(index.cpu().numpy(), cidx) and same_bits(sd.cpu().numpy(), csd)
    assert np.array_equal(counts.cpu().numpy(), ccnt) and same_bits(cost.cpu().numpy(), ccost)
    T.obstacle_contacts(g, 1.0, crash=True)
    assert np.array_equal(T.crashed(g).cpu().numpy().astype(np.uint8), ccrashed) and np.array_equal(ccrashed, chit)
    assert 50 < chit.sum() < n - 50 and (ccnt > 1).any() and (csd < 0).any()
