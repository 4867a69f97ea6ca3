"""The static obstacles on the GPU (mrs_swarm_set_obstacles, mrs_swarm_nearest_obstacles_device, mrs_swarm_obstacle_cost_device and their
tensor wrappers): every result is compared on bits with the numpy restatement of test_obstacles.py — the fixture scene (3 072 UAVs on
three airframes, 384 obstacles of all kinds, two world labels and all-worlds obstacles, a grid of several cells per axis) in FP64 and
FP32, every field subset, k in {1, 8, 32}, padded strides; both cost kinds with and without accumulate; exact thresholds, ties, overlapping
obstacles and non-finite UAVs; labels set after the obstacles; the grid cache and radii that force different grids; calls between the
pieces of a cost tick rollout; clones and replaced sets; refusals that change nothing; the caller's stream fence; and the C++ facade
(tests/cpp/obstacles_test.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import helpers
from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_obstacles import (ALL_WORLDS, BOX, COUNT, CYLINDER, FIXTURE_RADIUS, HINGE2, INVERSE, OBSTACLE, ON_DIST, ON_REL, ON_REL_BODY, SPHERE,
                            add_bits, fixture_scene, obstacles, restate_cost, restate_obstacles, restate_rows, same_bits)
from test_rollout_gpu import DT, REBOUNCE
from test_rollout_tick_cost_gpu import make_targets
from test_rollout_tick_gpu import N_PAIR, assert_same_swarm, pair_state, pair_swarm

pytestmark = pytest.mark.gpu
SENTINEL = -123.456
AIRFRAMES = ("x500", "f550", "t650")
_ref = {}


def fixture_ref(k):
    """the restatement of the fixture scene for list length k, computed once and shared (never written to)"""
    if 32 not in _ref:
        pos, worlds, ob = fixture_scene()
        _ref[32] = restate_obstacles(pos, scene_rotations(), worlds, ob, 32, FIXTURE_RADIUS)
    if k not in _ref:  # the first k slots of the longest list
        _ref[k] = {key: (v[:, :k].copy() if v.ndim > 1 else np.minimum(v, k) if key == "count" else v) for key, v in _ref[32].items()}
    for a in _ref[k].values():
        a.setflags(write=False)
    return _ref[k]


def scene_state():
    pos, _, _ = fixture_scene()
    if "state" not in _ref:
        _ref["state"] = helpers.random_state(np.random.default_rng(808), len(pos), 8, tilted=True)
    return _ref["state"]


def scene_rotations():
    return scene_state()["R"].reshape(-1, 3, 3)


def plain_swarm(mrs, pos, R=None):
    """x500s at `pos` (non-finite coordinates included), attitudes R or level"""
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    g = mrs.Swarm(n)
    g.construct(0, n, mrs.model_params("x500"), np.nan_to_num(pos, posinf=0.0, neginf=0.0))
    g.set_state(0, n, pos, None, R, None, None)
    x = g.get_states()["x"]
    assert same_bits(np.nan_to_num(x, nan=7.0), np.nan_to_num(pos, nan=7.0))
    return g


def scene_swarm(mrs, labels=True, obstacles_too=True):
    """the fixture scene on three airframes with random flight states; returns (swarm, positions as the swarm holds them)"""
    pos, worlds, ob = fixture_scene()
    n = len(pos)
    g = mrs.Swarm(n, arith=mrs.ARITH_FAST)
    third = n // 3
    st = {k: v.copy() for k, v in scene_state().items()}
    for a, name in enumerate(AIRFRAMES):
        first, count = a * third, (n - 2 * third if a == 2 else third)
        g.construct(first, count, mrs.model_params(name), np.nan_to_num(pos[first:first + count], posinf=0.0, neginf=0.0))
        st["motor_rpm"][first:first + count, mrs.AIRFRAMES[name]["n_motors"]:] = 0.0
    g.set_state(0, n, pos, st["v"], st["R"], st["omega"], st["motor_rpm"])
    s = g.get_states()
    assert same_bits(np.nan_to_num(s["x"], nan=7.0), np.nan_to_num(pos, nan=7.0)) and same_bits(s["R"].reshape(n, 9), st["R"].reshape(n, 9))
    if obstacles_too:
        g.set_obstacles(ob)
    if labels:
        g.set_worlds(worlds)
    return g


def run_rows(T, g, k, radius, fields, dtype, first=0, count=None, pad=3, ipad=2):
    """one tensors.nearest_obstacles call into padded, sentinel-filled tensors: (rows [count, k * w], index [count, k], counts [count]) as
    numpy; the slack columns and the rows around the range must come back untouched"""
    import torch
    count = g.n - first if count is None else count
    dev = torch_dev(g)
    width = T.obstacle_width(fields, k)
    out = torch.full((count + 2, width + pad), SENTINEL, dtype=dtype, device=dev)
    index = torch.full((count + 2, k + ipad), -7, dtype=torch.int32, device=dev)
    counts = torch.full((count + 2,), -9, dtype=torch.int32, device=dev)
    rows, idx, cnt = T.nearest_obstacles(g, k, radius, fields, first, count, out=out[1:count + 1] if fields else None, index=index[1:count + 1],
                                         counts=counts[1:count + 1])
    ho, hi, hc = out.cpu().numpy(), index.cpu().numpy(), counts.cpu().numpy()
    assert (ho[0] == SENTINEL).all() and (ho[count + 1] == SENTINEL).all() and (ho[:, width:] == SENTINEL).all(), "row slack was touched"
    assert (hi[0] == -7).all() and (hi[count + 1] == -7).all() and (hi[:, k:] == -7).all(), "index slack was touched"
    assert hc[0] == -9 and hc[count + 1] == -9
    if fields:
        assert rows.shape == (count, width) and rows.data_ptr() == out[1:].data_ptr()
    else:
        assert rows is None and (ho == SENTINEL).all()
    assert idx.shape == (count, k)
    return ho[1:count + 1, :width], hi[1:count + 1, :k], hc[1:count + 1]


def check_rows(T, g, res, k, radius, fields, dtype, first=0, count=None, label=""):
    import torch
    count = g.n - first if count is None else count
    sl = slice(first, first + count)
    rows, idx, cnt = run_rows(T, g, k, radius, fields, dtype, first, count)
    assert np.array_equal(cnt, res["count"][sl]), (label, "counts", np.flatnonzero(cnt != res["count"][sl])[:5])
    assert np.array_equal(idx, res["index"][sl]), (label, "index", np.flatnonzero((idx != res["index"][sl]).any(axis=1))[:5])
    want = restate_rows({key: v[sl] for key, v in res.items()}, fields, np.float64 if dtype == torch.float64 else np.float32)
    assert same_bits(rows, want), (label, "rows", np.flatnonzero((rows != want).any(axis=1))[:5])


def run_cost(T, g, radius, k, kind, weight, first=0, count=None, start=None, pad=3):
    """one tensors.obstacle_cost call into the middle of sentinel-padded buffers: (cost [count], found [count]) as numpy; start: the bits the
    cost vector holds before an accumulating call (None: accumulate=False over NaN bits)"""
    import torch
    count = g.n - first if count is None else count
    dev = torch_dev(g)
    cbuf = torch.full((count + 2 * pad,), SENTINEL, dtype=torch.float64, device=dev)
    fbuf = torch.full((count + 2 * pad,), -9, dtype=torch.int32, device=dev)
    cbuf[pad:pad + count] = float("nan") if start is None else torch.tensor(start, dtype=torch.float64, device=dev)
    out, found = T.obstacle_cost(g, radius, k, kind, weight, first, count, out=cbuf[pad:pad + count], accumulate=start is not None,
                                 found=fbuf[pad:pad + count])
    assert out.data_ptr() == cbuf[pad:].data_ptr() and found.data_ptr() == fbuf[pad:].data_ptr()
    hc, hf = cbuf.cpu().numpy(), fbuf.cpu().numpy()
    assert (hc[:pad] == SENTINEL).all() and (hc[pad + count:] == SENTINEL).all(), "cost elements outside [0, count) were touched"
    assert (hf[:pad] == -9).all() and (hf[pad + count:] == -9).all(), "found elements outside [0, count) were touched"
    return hc[pad:pad + count], hf[pad:pad + count]


def check_cost(T, g, res, k, radius, kind, weight, first=0, count=None, label=""):
    count = g.n - first if count is None else count
    sl = slice(first, first + count)
    term = restate_cost(res, k, radius, kind, weight)[sl]
    got, gf = run_cost(T, g, radius, k, kind, weight, first, count)
    assert np.array_equal(gf, res["found"][sl]), (label, "found")
    assert same_bits(got, add_bits(None, term)), (label, "accumulate=0", np.flatnonzero(got != add_bits(None, term))[:5])
    start = np.linspace(-3.0, 5.0, count)
    start[::7] = -0.0
    got, gf = run_cost(T, g, radius, k, kind, weight, first, count, start=start)
    assert np.array_equal(gf, res["found"][sl]) and same_bits(got, add_bits(start, term)), (label, "accumulate=1")
    return term


@pytest.fixture(scope="module")
def scene(mrs):
    return scene_swarm(mrs)


@pytest.mark.parametrize("k", [1, 8, 32])
def test_rows_exact_against_numpy(mrs, scene, k):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    res = fixture_ref(k)
    assert (res["found"] > k).any() and (res["found"] == 0).any()
    for dtype in (torch.float64, torch.float32):
        for fields in range(8):
            check_rows(T, g, res, k, FIXTURE_RADIUS, fields, dtype, label=(k, dtype, fields))


def test_rows_ranges_and_defaults(mrs, scene):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    res = fixture_ref(8)
    for first, count in ((0, 1), (1000, 517), (g.n - 37, 37)):  # ranges that are no multiple of the block
        check_rows(T, g, res, 8, FIXTURE_RADIUS, T.ON_ALL, torch.float64, first, count, label=(first, count))
    st = g.obstacle_stats()
    assert st["count"] == 384 and all(d > 1 for d in st["dims"]) and st["grid_radius"] == FIXTURE_RADIUS
    # defaults: new tensors, REL | DIST in FP32
    rows, idx, cnt = T.nearest_obstacles(g, 4, FIXTURE_RADIUS)
    assert rows.dtype == torch.float32 and rows.shape == (g.n, 16) and idx.shape == (g.n, 4) and cnt.shape == (g.n,)
    r4 = fixture_ref(4)
    assert same_bits(rows.cpu().numpy(), restate_rows(r4, ON_REL | ON_DIST, np.float32)) and np.array_equal(idx.cpu().numpy(), r4["index"])


def test_cost_exact_against_numpy(mrs, scene):
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    for k in (1, 8, 32):
        res = fixture_ref(k)
        for kind, weight in ((HINGE2, 1.0), (HINGE2, -0.375), (COUNT, 0.3)):
            term = check_cost(T, g, res, k, FIXTURE_RADIUS, kind, weight, label=(k, kind))
            assert (res["found"] > k).sum() >= 20 and (term != 0).any()
        check_cost(T, g, res, k, FIXTURE_RADIUS, HINGE2, 2.0, first=999, count=301, label=(k, "range"))
    # the order of the sum matters: nearest first is not the same bits as ascending index
    res = fixture_ref(32)
    by_index = np.argsort(np.where(res["index"] >= 0, res["index"], 2 ** 40), axis=1, kind="stable")
    swapped = dict(res, sd=np.take_along_axis(res["sd"], by_index, axis=1))
    a, b = restate_cost(res, 32, FIXTURE_RADIUS, HINGE2, 1.0), restate_cost(swapped, 32, FIXTURE_RADIUS, HINGE2, 1.0)
    assert (a.view(np.int64) != b.view(np.int64)).sum() > 50 and np.allclose(a, b, rtol=1e-12)
    # defaults, and without found
    out, nofound = T.obstacle_cost(g, FIXTURE_RADIUS)
    assert nofound is None and same_bits(out.cpu().numpy(), add_bits(None, restate_cost(fixture_ref(8), 8, FIXTURE_RADIUS, HINGE2, 1.0)))
    _, fnd = T.obstacle_cost(g, FIXTURE_RADIUS, found=True)
    assert np.array_equal(fnd.cpu().numpy(), fixture_ref(8)["found"]) and fnd.cpu().numpy().max() > 32  # not capped


def test_thresholds_ties_overlaps_and_non_finite(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    inf = np.inf
    ob = obstacles([(SPHERE, (0.0, 0.0, 0.0), (1.0, 0, 0)), (BOX, (20.0, 0.0, 0.0), (1.0, 1.0, 1.0)), (CYLINDER, (40.0, 0.0, 0.0), (1.0, 0, inf)),
                    (SPHERE, (65.0, 0.0, 0.0), (1.0, 0, 0)), (BOX, (62.0, 0.0, 0.0), (0.5, 0.5, 0.5)), (SPHERE, (65.0, 0.0, 0.0), (1.0, 0, 0)),
                    (BOX, (62.0, 0.0, 0.0), (0.5, 0.5, 0.5)),
                    (SPHERE, (80.0, 0.0, 0.0), (1.0, 0, 0)), (SPHERE, (80.0, 0.0, 0.0), (3.0, 0, 0)), (BOX, (80.0, 0.0, 0.0), (2.0, 2.0, 2.0)),
                    (CYLINDER, (80.0, 0.0, 0.0), (2.5, 0, 4.0))])
    closer = np.nextafter(3.5, 0.0)
    pos = np.array([[3.5, 0, 0], [closer, 0, 0], [23.5, 0, 0], [np.nextafter(23.5, 0.0), 0, 0], [43.5, 0, 1e6], [np.nextafter(43.5, 0.0), 0, -1e6],  # at / inside the radius
                    [60.0, 0, 0],                                    # two pairs of identical obstacles
                    [80.5, 0, 0], [80.0, 0, 0],                      # inside four overlapping obstacles
                    [np.nan, 0, 0], [80.0, inf, 0], [80.0, 0, -inf],  # non-finite
                    [1.0, 0, 0], [0.0, 21.0, 0.0], [40.0, 1.0, 5.0],  # on the surfaces
                    [1e9, -1e9, 1e7], [-300.0, 0, 0]])                # far outside the grid
    g = plain_swarm(mrs, pos)
    g.set_obstacles(ob)
    x = g.get_states()["x"]
    for radius in (2.5, np.nextafter(2.5, 3.0), 0.25, 10.0, 100.0):
        for k in (1, 4, 32):
            res = restate_obstacles(x, None, None, ob, k, radius)
            check_rows(T, g, res, k, radius, T.ON_ALL, torch.float64, label=("rows", radius, k))
            check_rows(T, g, res, k, radius, T.ON_ALL, torch.float32, label=("rows32", radius, k))
            for kind in (HINGE2, COUNT):
                check_cost(T, g, res, k, radius, kind, 1.5, label=("cost", radius, k, kind))
    _, idx, cnt = run_rows(T, g, 4, 2.5, 0, torch.float32)
    assert list(cnt[:6]) == [0, 1, 0, 1, 0, 1] and list(idx[1::2, 0][:3]) == [0, 1, 2], "sd == radius is outside, one ulp closer inside"
    _, idx2, cnt2 = run_rows(T, g, 4, np.nextafter(2.5, 3.0), 0, torch.float32)
    assert list(cnt2[:6]) == [1, 1, 1, 1, 1, 1]
    _, idx, cnt = run_rows(T, g, 4, 10.0, 0, torch.float32)
    assert list(idx[6]) == [4, 6, 3, 5], "identical obstacles list in index order, the nearer pair first"
    assert list(idx[7]) == [8, 10, 9, 7] and list(idx[8]) == [8, 10, 9, 7], "the deepest obstacle first"
    assert (cnt[9:12] == 0).all() and (idx[9:12] == -1).all(), "a non-finite UAV has no obstacles"
    got, found = run_cost(T, g, 10.0, 4, HINGE2, 1.0, start=np.full(len(pos), -0.0))
    assert same_bits(got[9:12], np.zeros(3)) and (found[9:12] == 0).all() and (found[15:] == 0).all()  # -0.0 + (+0.0) = +0.0
    assert found[7] == 4 and got[7] > got[6] > 0  # deeper costs more


def test_worlds_and_labels_set_after_the_obstacles(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    g = scene_swarm(mrs, labels=False)
    R = scene_rotations()
    unlabelled = restate_obstacles(pos, R, None, ob, 8, FIXTURE_RADIUS)
    check_rows(T, g, unlabelled, 8, FIXTURE_RADIUS, T.ON_ALL, torch.float64, label="before labels")
    check_cost(T, g, unlabelled, 8, FIXTURE_RADIUS, HINGE2, 1.0, label="before labels")
    T.set_worlds(g, torch.tensor(worlds, device=torch_dev(g)))  # after the obstacles, and after the grid was built
    res = fixture_ref(8)
    assert (res["found"] != unlabelled["found"]).sum() > 100
    check_rows(T, g, res, 8, FIXTURE_RADIUS, T.ON_ALL, torch.float64, label="labels")
    check_cost(T, g, res, 8, FIXTURE_RADIUS, COUNT, 1.0, label="labels")
    assert g.obstacle_stats()["grid_builds"] == 1  # labels are compared by the kernel: the grid does not depend on them
    # a label no obstacle carries sees the all-worlds obstacles only
    other = np.where(np.arange(len(pos)) % 2 == 0, -17, worlds).astype(np.int32)
    g.set_worlds(other)
    res2 = restate_obstacles(pos, R, other, ob, 8, FIXTURE_RADIUS)
    check_rows(T, g, res2, 8, FIXTURE_RADIUS, T.ON_DIST, torch.float64, label="other labels")
    listed = res2["index"][::2][res2["index"][::2] >= 0]
    assert len(listed) > 100 and (ob["flags"][listed] == ALL_WORLDS).all()


def test_grid_cache_and_radii_that_force_other_grids(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    g = scene_swarm(mrs)
    R = scene_rotations()
    assert g.obstacle_stats()["grid_builds"] == 0 and g.obstacle_stats()["count"] == len(ob) and g.obstacle_stats()["cells"] == 0
    res = fixture_ref(32)
    check_rows(T, g, res, 32, FIXTURE_RADIUS, T.ON_ALL, torch.float64, label="first")
    check_cost(T, g, res, 32, FIXTURE_RADIUS, HINGE2, 1.0, label="second")
    first = g.obstacle_stats()
    assert first["grid_builds"] == 1 and first["grid_radius"] == FIXTURE_RADIUS and first["cell_edge"] == 2 * FIXTURE_RADIUS
    assert first["cells"] == int(np.prod(first["dims"])) and first["list_items"] >= len(ob) and 0 < first["longest_list"] < len(ob)
    seen = {first["dims"]}
    # other radii, other grids (a finer one, a coarser one, one cell): each against the restatement, and each agreeing with the others
    # on what lies within the smallest radius — the traversal order is free
    small = 0.75
    base = restate_obstacles(pos, R, worlds, ob, 32, small)
    assert ((base["found"] > 0) & (base["found"] <= 32)).sum() > 300
    builds = 1
    for radius in (small, FIXTURE_RADIUS, 12.0, 500.0):
        resr = restate_obstacles(pos, R, worlds, ob, 32, radius) if radius != FIXTURE_RADIUS else res
        check_rows(T, g, resr, 32, radius, T.ON_ALL, torch.float64, label=("radius", radius))
        builds += 1
        st = g.obstacle_stats()
        assert st["grid_builds"] == builds and st["grid_radius"] == radius, st
        seen.add(st["dims"])
        rows, idx, _ = run_rows(T, g, 32, radius, T.ON_DIST, torch.float64)
        assert g.obstacle_stats()["grid_builds"] == builds  # the second call with this radius reuses the grid
        for i in np.flatnonzero(resr["found"] <= 32):
            near = rows[i][idx[i] >= 0] < small
            assert list(idx[i][idx[i] >= 0][near]) == list(base["index"][i][:base["count"][i]]), (radius, i)
    assert len(seen) >= 4 and (1, 1, 1) in seen, seen
    # a new set is another build, and so is going back to a radius that is no longer cached
    g.set_obstacles(ob[:100])
    assert g.obstacle_stats()["grid_builds"] == builds and g.obstacle_stats()["cells"] == 0 and g.obstacle_stats()["count"] == 100
    check_rows(T, g, restate_obstacles(pos, R, worlds, ob[:100], 8, 500.0), 8, 500.0, T.ON_ALL, torch.float32, label="new set")
    assert g.obstacle_stats()["grid_builds"] == builds + 1


@pytest.mark.parametrize("crash", [False, True], ids=["elastic", "crash"])
@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
def test_inside_a_horizon(mrs, arith, crash):
    """rollout_tick_cost over 24 + 24 ticks with accumulate, obstacle_cost(accumulate) between the halves and after; a twin runs the same
    horizon without the obstacle calls and adds the restated terms to its vector on the host, in the order of the calls: final state and
    crash flags are the twin's bit for bit, and so is the cost vector after every piece and every call"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ar = getattr(mrs, "ARITH_" + arith)
    a, b = pair_swarm(mrs, ar), pair_swarm(mrs, ar)
    pos, _ = pair_state()
    rng = np.random.default_rng(31)
    m = 96
    ob = np.zeros(m, OBSTACLE)
    ob["kind"] = np.arange(m) % 3
    ob["c"] = pos[rng.integers(0, 64, m)] + rng.uniform(-3, 3, (m, 3))  # around the colliding pairs and their neighbours
    ob["h"] = rng.uniform(0.2, 1.5, (m, 3))
    ob["h"][5::6, 2] = np.inf
    a.set_obstacles(ob)
    dev = torch_dev(a)
    ticks, hold = 24, 4
    groups = T.OBS_POS | T.OBS_VEL
    blocks = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (2 * ticks // hold, N_PAIR, 4))
    cmd = torch.tensor(blocks, device=dev)
    tg, wt = make_targets(rng, 2 * ticks // hold, N_PAIR, T.gather_width(groups), torch.float64, dev, False, False)
    costs = {id(a): torch.zeros(N_PAIR, dtype=torch.float64, device=dev), id(b): torch.zeros(N_PAIR, dtype=torch.float64, device=dev)}
    half = ticks // hold
    listed, terms = 0, []
    for piece in range(2):
        sl = slice(piece * half, (piece + 1) * half)
        for g in (a, b):
            T.rollout_tick_cost(g, O.POSITION_CMD, cmd[sl], DT, crash, REBOUNCE, groups, tg[sl], wt[sl], 1000.0, hold=hold, out=costs[id(g)],
                                accumulate=True)
        xa = T.gather(a, T.OBS_POS, dtype=torch.float64).cpu().numpy()  # (the same calls and host waits in both runs)
        T.gather(b, T.OBS_POS, dtype=torch.float64).cpu()
        # the twin's vector: its own rollout pieces plus the restated terms, added on the host in the order of the calls
        assert same_bits(costs[id(a)].cpu().numpy(), costs[id(b)].cpu().numpy()), piece
        if piece == 1:
            a.set_obstacles(ob)  # the setter too leaves the pending collision tick pending (and drops the cached grid)
        for kind, radius, k, weight in ((HINGE2, 4.0, 4, 0.5), (COUNT, 1.0, 8, 2.0)):
            before = costs[id(a)].cpu().numpy()
            res = restate_obstacles(xa, None, None, ob, k, radius)
            term = restate_cost(res, k, radius, kind, weight)
            _, gf = T.obstacle_cost(a, radius, k, kind, weight, out=costs[id(a)], accumulate=True, found=True)
            assert np.array_equal(gf.cpu().numpy(), res["found"]), (piece, kind)
            assert same_bits(costs[id(a)].cpu().numpy(), add_bits(before, term)), (piece, kind)
            listed += int(res["count"].sum())
            terms.append(term)
            costs[id(b)].copy_(torch.tensor(add_bits(costs[id(b)].cpu().numpy(), term), device=dev))
    assert listed > 100 and len(terms) == 4 and all((t != 0).any() for t in terms)
    assert same_bits(costs[id(a)].cpu().numpy(), costs[id(b)].cpu().numpy())
    if crash:
        assert np.asarray(a.has_crashed()).any()
    assert_same_swarm(a, b, f"{arith} crash={crash}: with and without the obstacle calls")
    for g in (a, b):
        g.tick_n(DT, 1, True, crash, REBOUNCE)  # evaluates the collision tick the horizon left pending
    assert_same_swarm(a, b, f"{arith} crash={crash}: one more tick on both")


def test_lifetime_clone_replace_and_clear(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    sel = slice(0, 600)
    g = plain_swarm(mrs, pos[sel])
    g.set_worlds(worlds[sel])
    x = g.get_states()["x"]
    # no set was ever given: empty rows, +0.0, found 0
    empty = restate_obstacles(x, None, worlds[sel], ob[:0], 8, FIXTURE_RADIUS)
    assert len(g.get_obstacles()) == 0 and g.obstacle_stats()["count"] == 0
    check_rows(T, g, empty, 8, FIXTURE_RADIUS, T.ON_ALL, torch.float64, label="never set")
    got, found = run_cost(T, g, FIXTURE_RADIUS, 8, HINGE2, 1.0, start=np.full(600, -0.0))
    assert same_bits(got, np.zeros(600)) and (found == 0).all()
    T.set_obstacles(g, ob["kind"], ob["c"], ob["h"], worlds=ob["world"], all_worlds=ob["flags"] == ALL_WORLDS)
    back = g.get_obstacles()
    assert back.dtype == OBSTACLE and back.tobytes() == ob.tobytes()
    res = restate_obstacles(x, None, worlds[sel], ob, 8, FIXTURE_RADIUS)
    check_rows(T, g, res, 8, FIXTURE_RADIUS, T.ON_ALL, torch.float64, label="set")
    # the clone owns a copy: it answers like the original, and goes on doing so after the original's set is replaced
    c = g.clone()
    big = g.clone_resized(700)
    assert c.get_obstacles().tobytes() == ob.tobytes() and big.get_obstacles().tobytes() == ob.tobytes()
    assert c.obstacle_stats()["grid_builds"] == 0
    half = ob[1::2]
    g.set_obstacles(half)
    check_rows(T, g, restate_obstacles(x, None, worlds[sel], half, 8, FIXTURE_RADIUS), 8, FIXTURE_RADIUS, T.ON_ALL, torch.float64, label="replaced")
    check_cost(T, g, restate_obstacles(x, None, worlds[sel], half, 8, FIXTURE_RADIUS), 8, FIXTURE_RADIUS, HINGE2, 1.0, label="replaced")
    check_rows(T, c, res, 8, FIXTURE_RADIUS, T.ON_ALL, torch.float64, label="clone")
    check_cost(T, c, res, 8, FIXTURE_RADIUS, COUNT, 1.0, label="clone")
    xb = big.get_states()["x"]
    wb = np.concatenate([worlds[sel], np.zeros(100, np.int32)])
    check_rows(T, big, restate_obstacles(xb, None, wb, ob, 8, FIXTURE_RADIUS), 8, FIXTURE_RADIUS, T.ON_DIST, torch.float64, label="resized clone")
    g.set_obstacles(None)  # cleared
    assert len(g.get_obstacles()) == 0
    check_rows(T, g, empty, 8, FIXTURE_RADIUS, T.ON_ALL, torch.float32, label="cleared")
    # a refused set changes nothing
    assert half["kind"][0] == BOX
    c.set_obstacles(half)
    for mutate in (lambda o: o["h"].__setitem__((3, 0), -1.0), lambda o: o["kind"].__setitem__(0, 3), lambda o: o["c"].__setitem__((7, 1), np.nan),
                   lambda o: o["flags"].__setitem__(2, 2), lambda o: o["reserved"].__setitem__(2, 1), lambda o: o["h"].__setitem__((0, 2), np.inf)):  # (half[0] is a box)
        bad = half.copy()
        mutate(bad)
        with pytest.raises(mrs.MrsError, match="error 1:"):
            c.set_obstacles(bad)
    assert c.get_obstacles().tobytes() == half.tobytes()
    check_rows(T, c, restate_obstacles(x, None, worlds[sel], half, 8, FIXTURE_RADIUS), 8, FIXTURE_RADIUS, T.ON_DIST, torch.float64, label="after refusals")
    for s in (g, c, big):
        s.close()


def test_refused_calls_change_nothing(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    g = plain_swarm(mrs, pos[:300])
    g.set_obstacles(ob)
    before = g.get_states()
    dev = torch_dev(g)
    st = torch.cuda.current_stream(dev).cuda_stream
    rows = torch.full((300, 8 * 7), SENTINEL, dtype=torch.float64, device=dev)
    index = torch.full((300, 8), -7, dtype=torch.int32, device=dev)
    counts = torch.full((300,), -9, dtype=torch.int32, device=dev)
    cost = torch.full((300,), SENTINEL, dtype=torch.float64, device=dev)
    r, i, n, c = rows.data_ptr(), index.data_ptr(), counts.data_ptr(), cost.data_ptr()
    host = np.zeros(300 * 56)
    hip = C.CDLL("libamdhip64.so")
    small_p, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(small_p), C.c_size_t(4096)) == 0
    assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), small_p) == 0 and size.value < 4100
    small = small_p.value
    nan, inf = float("nan"), float("inf")
    F = T.ON_ALL
    bad_rows = [
        ((200, 101, 8, 3.0, F, r, 0, 56, i, 8, n), "error 3:"),
        ((-1, 10, 8, 3.0, F, r, 0, 56, i, 8, n), "error 3:"),
        ((0, 300, 0, 3.0, F, r, 0, 56, i, 8, n), "error 1:.*k must be"),
        ((0, 300, 33, 3.0, F, r, 0, 56, i, 8, n), "error 1:.*k must be"),
        ((0, 300, 8, 0.0, F, r, 0, 56, i, 8, n), "error 1:.*radius"),
        ((0, 300, 8, -2.0, F, r, 0, 56, i, 8, n), "error 1:.*radius"),
        ((0, 300, 8, nan, F, r, 0, 56, i, 8, n), "error 1:.*radius"),
        ((0, 300, 8, inf, F, r, 0, 56, i, 8, n), "error 1:.*radius"),
        ((0, 300, 8, 3.0, 8, r, 0, 56, i, 8, n), "error 1:.*unknown obstacle field bits"),
        ((0, 300, 8, 3.0, F, r, 7, 56, i, 8, n), "error 1:"),
        ((0, 300, 8, 3.0, F, r, 0, 55, i, 8, n), "error 1:.*stride smaller"),
        ((0, 300, 8, 3.0, F, r, 0, 56, i, 7, n), "error 1:.*index_stride smaller"),
        ((0, 300, 8, 3.0, F, 0, 0, 56, 0, 8, 0), "error 1:.*no output given"),
        ((0, 300, 8, 3.0, 0, r, 0, 56, 0, 8, 0), "error 1:.*no output given"),
        ((0, 300, 8, 3.0, F, host.ctypes.data, 0, 56, i, 8, n), "error 1:.*dev_rows"),
        ((0, 300, 8, 3.0, F, small, 0, 56, i, 8, n), "error 1:.*dev_rows: the rows extend past"),
        ((0, 300, 8, 3.0, F, r, 0, 56, small, 8, n), "error 1:.*dev_index: the rows extend past"),
        ((0, 300, 8, 3.0, F, r, 0, 56, i, 8, small + 4096 - 1196), "error 1:.*dev_count: the rows extend past"),
    ]
    H = HINGE2
    bad_cost = [
        ((200, 101, 8, 3.0, H, 1.0, c, 0, n), "error 3:"),
        ((0, 300, 0, 3.0, H, 1.0, c, 0, n), "error 1:.*k must be"),
        ((0, 300, 33, 3.0, H, 1.0, c, 0, n), "error 1:.*k must be"),
        ((0, 300, 8, 0.0, H, 1.0, c, 0, n), "error 1:.*radius"),
        ((0, 300, 8, nan, H, 1.0, c, 0, n), "error 1:.*radius"),
        ((0, 300, 8, inf, H, 1.0, c, 0, n), "error 1:.*radius"),
        ((0, 300, 8, 3.0, INVERSE, 1.0, c, 0, n), "error 1:.*MRS_PROX_INVERSE"),
        ((0, 300, 8, 3.0, 3, 1.0, c, 0, n), "error 1:.*unknown obstacle cost kind"),
        ((0, 300, 8, 3.0, -1, 1.0, c, 0, n), "error 1:.*unknown obstacle cost kind"),
        ((0, 300, 8, 3.0, H, 1.0, 0, 0, n), "error 1:.*dev_cost: null pointer"),
        ((0, 0, 8, 3.0, H, 1.0, 0, 0, n), "error 1:.*dev_cost: null pointer"),
        ((0, 300, 8, 3.0, H, 1.0, host.ctypes.data, 0, n), "error 1:.*dev_cost"),
        ((0, 300, 8, 3.0, H, 1.0, c, 1, host.ctypes.data), "error 1:.*dev_found"),
        ((0, 300, 8, 3.0, H, 1.0, small + 4096 - 2392, 1, n), "error 1:.*dev_cost: the rows extend past"),
        ((0, 300, 8, 3.0, H, 1.0, c, 1, small + 4096 - 1196), "error 1:.*dev_found: the rows extend past"),
    ]
    torch.cuda.synchronize(dev)
    for args, msg in bad_rows:
        with pytest.raises(mrs.MrsError, match=msg):
            g.nearest_obstacles_device(*args, st)
    for args, msg in bad_cost:
        with pytest.raises(mrs.MrsError, match=msg):
            g.obstacle_cost_device(*args, st)
    torch.cuda.synchronize(dev)
    assert hip.hipFree(C.c_void_p(small)) == 0

    def untouched():
        return ((rows.cpu().numpy() == SENTINEL).all() and (index.cpu().numpy() == -7).all() and (counts.cpu().numpy() == -9).all()
                and (cost.cpu().numpy() == SENTINEL).all())

    assert untouched() and g.obstacle_stats()["grid_builds"] == 0  # nothing was launched, no grid was built
    # count == 0 is MRS_OK and writes nothing
    g.nearest_obstacles_device(0, 0, 8, 3.0, F, r, 0, 56, i, 8, n, st)
    g.nearest_obstacles_device(300, 0, 8, 3.0, F, r, 0, 56, 0, 8, 0, st)
    g.obstacle_cost_device(300, 0, 8, 3.0, H, 1.0, c, 1, 0, st)
    assert untouched()
    after = g.get_states()
    for key in before.dtype.names:
        assert before[key].tobytes() == after[key].tobytes(), key
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
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.obstacle_cost(s, 3.0, out=cost[:100])
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.nearest_obstacles(s, 8, 3.0, F, out=rows[:100], index=index[:100], counts=counts[:100])
    assert untouched()
    for s in shards:
        s.close()
    group.close()


def test_caller_stream_is_fenced(mrs, scene):
    """the outputs are filled on a side stream kept busy by a long sleep, then both calls are made with that stream current: the cost vector
    must hold fill + term (the kernel ran after the fill), the rows the result (not the fill), and copies queued behind the calls on the
    side stream read them"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    dev = torch_dev(g)
    res = fixture_ref(8)
    term = restate_cost(res, 8, FIXTURE_RADIUS, HINGE2, 1.0)
    out = torch.zeros(g.n, dtype=torch.float64, device=dev)
    fnd = torch.zeros(g.n, dtype=torch.int32, device=dev)
    rows = torch.zeros((g.n, 8), dtype=torch.float64, device=dev)
    T.obstacle_cost(g, FIXTURE_RADIUS)  # (the grid is built: the fenced calls launch and nothing else)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        out.fill_(2.5)
        fnd.fill_(-5)
        rows.fill_(SENTINEL)
        T.obstacle_cost(g, FIXTURE_RADIUS, out=out, accumulate=True, found=fnd)
        T.nearest_obstacles(g, 8, FIXTURE_RADIUS, T.ON_DIST, out=rows)
        copy, fcopy, rcopy = out * 1.0, fnd.clone(), rows.clone()
    side.synchronize()
    assert same_bits(copy.cpu().numpy(), add_bits(np.full(g.n, 2.5), term)) and np.array_equal(fcopy.cpu().numpy(), res["found"])
    assert same_bits(rcopy.cpu().numpy(), restate_rows(res, ON_DIST))


def test_cpp_facade_equals_python(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, k, m, w = 2000, 4, 60, 7
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "obstacles.bin")
        out = subprocess.run([build_cpp("obstacles_test"), path], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok obstacles_equal_brute_force", "ok written"):
            assert tag in out.stdout, out.stdout
        raw = open(path, "rb").read()
    o = 0
    crow = np.frombuffer(raw, np.float64, n * k * w, o).reshape(n, k * w)
    o += 8 * n * k * w
    cidx = np.frombuffer(raw, np.int32, n * k, o).reshape(n, k)
    o += 4 * n * k
    ccnt = np.frombuffer(raw, np.int32, n, o)
    o += 4 * n
    ccost = np.frombuffer(raw, np.float64, n, o)
    o += 8 * n
    cfound = np.frombuffer(raw, np.int32, n, o)
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
    rows, idx, cnt = T.nearest_obstacles(g, k, 5.0, T.ON_ALL, dtype=torch.float64)
    assert same_bits(rows.cpu().numpy(), crow) and np.array_equal(idx.cpu().numpy(), cidx) and np.array_equal(cnt.cpu().numpy(), ccnt)
    both, fnd = T.obstacle_cost(g, 5.0, k, T.PROX_HINGE2, 0.75, found=True)
    T.obstacle_cost(g, 5.0, k, T.PROX_COUNT, 0.75, out=both, accumulate=True)
    assert same_bits(both.cpu().numpy(), ccost) and np.array_equal(fnd.cpu().numpy(), cfound)
    assert (cfound > k).any() and (crow[:, 6] < 0).any()
