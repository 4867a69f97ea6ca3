"""The line-of-sight neighbours on the GPU (mrs_swarm_nearest_visible_device and tensors.nearest_visible): every result is compared on
bits with the numpy restatement of test_nearest_visible.py — the fixture scene (3 072 UAVs on three airframes, two world labels, 384
obstacles, two non-finite UAVs) at k = 1, 8, 32 in FP64 and FP32 with all fields and with none; equality with nearest where nothing can
hide; more visible candidates than two LDS lists; a 40-UAV swarm whose probes share buckets, alone and padded; another grid and other
radii; labels set later and obstacles of other worlds; sub-ranges, slack, every output left out in turn; a call between the pieces of a
tick rollout; the four cache entries; refusals that change nothing; the caller's stream fence; the C++ facade
(tests/cpp/nearest_visible_test.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_nearest import nearest_rows
from test_nearest_visible import NO_OBSTACLES, SCENE_RADIUS, restate_visible, scene_visible
from test_obstacles import ALL_WORLDS, BOX, OBSTACLE, SPHERE, fixture_scene, obstacles, same_bits
from test_obstacles_gpu import SENTINEL, plain_swarm, scene_state, scene_swarm
from test_rollout_gpu import DT, REBOUNCE
from test_rollout_tick_cost_gpu import make_targets
from test_rollout_tick_gpu import N_PAIR, assert_same_swarm, pair_state, pair_swarm

pytestmark = pytest.mark.gpu
CAP = 256  # NV_CAP of csrc/nearest_visible.hip: entries of the visible list in LDS
NN_ALL, NN_REL_POS, NN_DIST = 0x1F, 1, 16
WIDTH = {0: 0, NN_ALL: 13, NN_REL_POS | NN_DIST: 4}
OUTPUTS = ("rows", "index", "counts", "visible", "hidden")


def first_k(res, k):
    """the first k slots of a restatement of a longer list"""
    return dict(res, index=res["index"][:, :k], d2=res["d2"][:, :k], counts=np.minimum(res["visible"], k))


def run_visible(T, g, k, radius, fields, dtype, first=0, count=None, want=OUTPUTS, pad=3, ipad=2):
    """one tensors.nearest_visible call into padded, sentinel-filled tensors: a dict of numpy arrays (None: not asked for); the slack
    columns and the rows around the range must come back untouched, and an output that is not asked for is not written at all"""
    import torch
    count = g.n - first if count is None else count
    dev = torch_dev(g)
    w = k * WIDTH[fields]
    fields_asked = fields if "rows" in want else 0
    out = torch.full((count + 2, w + pad), SENTINEL, dtype=dtype, device=dev)
    index = torch.full((count + 2, k + ipad), -7, dtype=torch.int32, device=dev)
    vec = {name: torch.full((count + 2,), -9, dtype=torch.int32, device=dev) for name in ("counts", "visible", "hidden")}
    r, ix, c, v, h = T.nearest_visible(g, k, radius, fields_asked, first, count, out=out[1:count + 1] if fields_asked else None,
                                       index=index[1:count + 1] if "index" in want else False,
                                       **{name: (t[1:count + 1] if name in want else (False if name == "counts" else None)) for name, t in vec.items()})
    ho, hi = out.cpu().numpy(), index.cpu().numpy()
    fill = np.float32(SENTINEL) if dtype == torch.float32 else SENTINEL
    got = dict.fromkeys(OUTPUTS)
    if fields_asked:
        assert (ho[0] == fill).all() and (ho[count + 1] == fill).all() and (ho[:, w:] == fill).all(), "row slack was touched"
        assert r.shape == (count, w)
        got["rows"] = ho[1:count + 1, :w]
    else:
        assert r is None and (ho == fill).all()
    if "index" in want:
        assert (hi[0] == -7).all() and (hi[count + 1] == -7).all() and (hi[:, k:] == -7).all(), "index slack was touched"
        assert ix.shape == (count, k)
        got["index"] = hi[1:count + 1, :k]
    else:
        assert ix is None and (hi == -7).all()
    for name, ret in (("counts", c), ("visible", v), ("hidden", h)):
        host = vec[name].cpu().numpy()
        if name in want:
            assert host[0] == -9 and host[count + 1] == -9 and ret.shape == (count,)
            got[name] = host[1:count + 1]
        else:
            assert ret is None and (host == -9).all(), name
    return got


def check_visible(T, g, x, v, R, res, k, radius, fields, dtype, first=0, count=None, want=OUTPUTS, label=""):
    """res: the restatement of observers [first, first + count) for list length k"""
    import torch
    count = g.n - first if count is None else count
    got = run_visible(T, g, k, radius, fields, dtype, first, count, want)
    for name in ("index", "counts", "visible", "hidden"):
        if name in want:
            assert np.array_equal(got[name], res[name]), (label, name, np.argwhere(got[name] != res[name])[:5])
    if fields and "rows" in want:
        rows = nearest_rows(x, v, R, first, res["index"], res["d2"], fields).astype(np.float64 if dtype == torch.float64 else np.float32)
        assert same_bits(got["rows"], rows), (label, "rows", np.argwhere(got["rows"] != rows)[:5])
    return got


def level(n):
    return np.zeros((n, 3)), np.broadcast_to(np.eye(3), (n, 3, 3))


def check_plain(T, g, x, worlds, ob, k, radius, label, first=0, count=None):
    """FP64 REL_POS | DIST rows and every vector of a swarm at rest with level attitudes against the restatement of what it holds"""
    import torch
    count = len(x) - first if count is None else count
    res = restate_visible(x, worlds, ob, first, count, k, radius)
    v, R = level(len(x))
    check_visible(T, g, x, v, R, res, k, radius, NN_REL_POS | NN_DIST, torch.float64, first, count, label=label)
    return res


@pytest.fixture(scope="module")
def scene(mrs):
    return scene_swarm(mrs)


def scene_args():
    pos, worlds, ob = fixture_scene()
    st = scene_state()
    return pos, st["v"], st["R"].reshape(-1, 3, 3)


# ---- 1. the fixture scene ----

@pytest.mark.parametrize("k", [1, 8, 32])
def test_fixture_scene_exact_against_numpy(mrs, scene, k):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    x, v, R = scene_args()
    res = first_k(scene_visible(32), k)
    for dtype in (torch.float64, torch.float32):
        for fields in (NN_ALL, 0):
            check_visible(T, scene, x, v, R, res, k, SCENE_RADIUS, fields, dtype, label=(k, dtype, fields))
    assert (res["counts"][200:202] == 0).all() and (res["hidden"] > 0).sum() > 1000 and (res["visible"] > 8).sum() >= 1000


# ---- 2. equality with nearest where nothing can hide ----

def test_without_anything_to_hide_equals_nearest(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    g = scene_swarm(mrs, obstacles_too=False)
    far = ob.copy()
    far["c"] = far["c"] + 1000.0
    for label, given in (("no set ever given", None), ("an empty set", ob[:0]), ("every obstacle 1 km away", far)):
        if given is not None:
            g.set_obstacles(given)
        for dtype in (torch.float64, torch.float32):
            rows, index, counts = T.nearest(g, 8, SCENE_RADIUS, NN_ALL, dtype=dtype)
            r, ix, c, v, h = T.nearest_visible(g, 8, SCENE_RADIUS, NN_ALL, dtype=dtype)
            assert same_bits(r.cpu().numpy(), rows.cpu().numpy()), label
            assert torch.equal(ix, index) and torch.equal(c, counts) and not h.any() and (v >= c).all() and (v > 8).any(), label


# ---- 3. more visible candidates than the LDS list holds ----

def test_more_visible_candidates_than_two_lists(mrs):
    """700 UAVs in a ball of 3 m around UAV 0 and a thin wall at x = 1.5 m through the ball, k = 32: the list of observer 0 is reduced to
    its first 32 entries at least twice on the way, and more than a group of records is hidden from it"""
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(3)
    pts = rng.uniform(-3, 3, (4000, 3))
    pts = pts[(pts * pts).sum(axis=1) < 8.9][:700]
    x = np.concatenate([np.zeros((1, 3)), pts])
    wall = obstacles([(BOX, (1.5, 0, 0), (0.02, 5.0, 5.0))])
    g = plain_swarm(mrs, x)
    g.set_obstacles(wall)
    res = check_plain(T, g, x, None, wall, 32, 3.0, "dense")
    assert res["visible"][0] > 2 * CAP and res["hidden"][0] > 64, (res["visible"][0], res["hidden"][0])
    assert (res["visible"] > CAP).sum() > 100
    g.close()


# ---- 4. probes that share buckets ----

def test_forty_uavs_and_the_same_forty_padded(mrs):
    """40 UAVs in a swarm of 40: the hash has 128 buckets for 27 probes per observer, so probes share buckets; no neighbour may be counted
    twice.  The same forty in a swarm padded with 5 000 far UAVs (a table of 16 384 buckets): the same bits"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(40)
    x = rng.uniform(-3, 3, (40, 3))
    ob = obstacles([(BOX, (0.5, 0, 0), (0.1, 1.5, 1.5)), (SPHERE, (-1.0, 1.0, 0), (0.7, 0, 0))])
    g = plain_swarm(mrs, x)
    g.set_obstacles(ob)
    res = check_plain(T, g, x, None, ob, 32, 4.0, "forty")
    assert res["visible"].max() > 20 and res["hidden"].max() > 5 and (res["visible"] + res["hidden"]).max() <= 39
    small = run_visible(T, g, 32, 4.0, NN_REL_POS | NN_DIST, torch.float64)
    pad = np.stack([1000.0 + 20.0 * np.arange(5000), np.zeros(5000), np.full(5000, 5.0)], axis=1)
    big = plain_swarm(mrs, np.concatenate([x, pad]))
    big.set_obstacles(ob)
    padded = run_visible(T, big, 32, 4.0, NN_REL_POS | NN_DIST, torch.float64, 0, 40)
    for name in OUTPUTS:
        assert small[name].tobytes() == padded[name].tobytes(), name
    g.close()
    big.close()


# ---- 5. the grid cannot matter ----

def test_grid_independence(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    x, v, R = scene_args()
    g = scene_swarm(mrs)
    far = obstacles([(BOX, (5e6, -3e6, 1e5), (4e4, 9e4, 2e4), 0, ALL_WORLDS)])
    g.set_obstacles(np.concatenate([ob, far]))  # another extent, another coarsening; index 384 hides nothing
    res = first_k(scene_visible(32), 8)
    check_visible(T, g, x, v, R, res, 8, SCENE_RADIUS, NN_ALL, torch.float64, label="with a far, huge obstacle")
    g.set_obstacles(ob)
    for radius in (2.0, 12.0):  # other hash edges, other grids
        sub = restate_visible(pos, worlds, ob, 100, 256, 8, radius)
        check_visible(T, g, x, v, R, sub, 8, radius, NN_ALL, torch.float64, 100, 256, label=radius)
        assert sub["hidden"].sum() > (0 if radius == 2.0 else 1000), sub["hidden"].sum()
    g.close()


# ---- 6. worlds ----

def test_worlds(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    x, v, R = scene_args()
    g = scene_swarm(mrs, labels=False)
    none = restate_visible(pos, None, ob, 0, 512, 8, SCENE_RADIUS)  # every UAV in world 0: the kernel without the label column
    check_visible(T, g, x, v, R, none, 8, SCENE_RADIUS, NN_ALL, torch.float64, 0, 512, label="before labels")
    g.set_worlds(worlds)
    res = first_k(scene_visible(32), 8)
    sub = {name: a[:512] for name, a in res.items() if name != "pairs"}
    check_visible(T, g, x, v, R, sub, 8, SCENE_RADIUS, NN_ALL, torch.float64, 0, 512, label="labels set after a first call")
    assert (none["index"] != sub["index"]).any()
    g.close()
    # observer 0 (world 0) at the origin, a target of its world behind a box, a UAV of world 5 in the open
    x4 = np.array([(0, 0, 0), (7.0, 0, 0), (0, 3.0, 0), (7.0, 0.5, 0)], np.float64)
    w4 = np.array([0, 0, 5, 5], np.int32)
    s = plain_swarm(mrs, x4)
    s.set_worlds(w4)
    for ob4, want in ((obstacles([(BOX, (5.0, 0, 0), (1.0, 1.0, 1.0), 5)]), ([1, -1], 1, 0)),
                      (obstacles([(BOX, (5.0, 0, 0), (1.0, 1.0, 1.0), 77, ALL_WORLDS)]), ([-1, -1], 0, 1))):
        s.set_obstacles(ob4)
        r4 = check_plain(T, s, x4, w4, ob4, 2, 10.0, "four")
        assert (list(r4["index"][0]), r4["visible"][0], r4["hidden"][0]) == want
        assert list(r4["index"][2]) == [-1, -1] and (r4["visible"][2], r4["hidden"][2]) == (0, 1)  # (the box stands between 2 and 3 too)
    s.close()


# ---- 7. sub-ranges, slack, outputs left out, count == 0 ----

def test_subranges_strides_and_optional_outputs(mrs, scene):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    x, v, R = scene_args()
    res = first_k(scene_visible(32), 8)
    for first, count in ((0, 1), (63, 130), (190, 20), (3071, 1), (1500, 1572)):
        sub = {name: a[first:first + count] for name, a in res.items() if name != "pairs"}
        check_visible(T, scene, x, v, R, sub, 8, SCENE_RADIUS, NN_ALL, torch.float32, first, count, label=(first, count))
    sub = {name: a[40:340] for name, a in res.items() if name != "pairs"}
    for left_out in OUTPUTS:
        want = tuple(name for name in OUTPUTS if name != left_out)
        check_visible(T, scene, x, v, R, sub, 8, SCENE_RADIUS, NN_ALL, torch.float64, 40, 300, want=want, label="without " + left_out)
    for only in OUTPUTS:
        check_visible(T, scene, x, v, R, sub, 8, SCENE_RADIUS, NN_ALL, torch.float64, 40, 300, want=(only,), label="only " + only)
    r, ix, c, vis, hid = T.nearest_visible(scene, 8, SCENE_RADIUS, NN_ALL, first=17, count=0)
    assert r.shape == (0, 104) and ix.shape == (0, 8) and c.shape == (0,) and vis.shape == (0,) and hid.shape == (0,)
    st = torch.cuda.current_stream(torch_dev(scene)).cuda_stream
    scene.nearest_visible_device(3072, 0, 8, SCENE_RADIUS, 0, 0, T.DTYPE_F64, 0, 0, 0, 0, 0, 1, st)  # (count == 0 after the checks: MRS_OK)


# ---- 8. inside a horizon ----

@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
def test_inside_a_horizon(mrs, arith):
    """rollout_tick_cost over 24 + 24 ticks with accumulate and a call between the halves and after (a collision tick is pending at both
    points); a twin runs the same horizon without the calls: final state, crash flags and costs are the twin's bit for bit, and each call
    judges the UAVs where the steps have moved them"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ar = getattr(mrs, "ARITH_" + arith)
    a, b = pair_swarm(mrs, ar), pair_swarm(mrs, ar)
    pos, _ = pair_state()
    rng = np.random.default_rng(31)
    m, walls = 128, 96
    ob = np.zeros(m, OBSTACLE)
    ob["kind"] = np.arange(m) % 3
    ob["c"] = pos[rng.integers(0, 64, m)] + rng.uniform(-4, 4, (m, 3))  # around the colliding pairs and their neighbours
    ob["h"] = rng.uniform(0.2, 1.5, (m, 3))
    # 96 solids of every kind, each within 0.2 m per axis of the midpoint between two UAVs that stand 10 m apart, every size at least
    # 0.4 m: each hides the two from each other whatever a few ticks do to them
    gaps = rng.choice(np.arange(32, N_PAIR - 1), walls, replace=False)
    ob["c"][:walls] = pos[gaps] + [5.0, 0.0, 0.0] + rng.uniform(-0.2, 0.2, (walls, 3))
    ob["h"][:walls] = rng.uniform(0.4, 1.5, (walls, 3))
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
    hidden, seen = 0, []
    for piece in range(2):
        sl = slice(piece * half, (piece + 1) * half)
        for g in (a, b):
            T.rollout_tick_cost(g, O.POSITION_CMD, cmd[sl], DT, True, REBOUNCE, groups, tg[sl], wt[sl], 1000.0, hold=hold, out=costs[id(g)],
                                accumulate=True)
        xa = T.gather(a, T.OBS_POS, dtype=torch.float64).cpu().numpy()  # (the same calls and host waits in both runs)
        T.gather(b, T.OBS_POS, dtype=torch.float64).cpu()
        res = check_plain(T, a, xa, None, ob, 4, 12.0, (arith, piece))
        hidden += int(res["hidden"].sum())
        seen.append(xa)
    assert hidden >= 2 * 2 * walls, hidden  # (both directions of every walled gap, in both calls)
    assert not same_bits(seen[0], seen[1]) and not same_bits(seen[0], pos)
    assert same_bits(costs[id(a)].cpu().numpy(), costs[id(b)].cpu().numpy())
    assert_same_swarm(a, b, f"{arith}: with and without the line-of-sight calls")
    for g in (a, b):
        g.tick_n(DT, 1, True, True, REBOUNCE)  # evaluates the collision tick the horizon left pending
    assert_same_swarm(a, b, f"{arith}: one more tick on both")
    a.close()
    b.close()


# ---- 9. the cache ----

def test_four_cache_entries(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    x, v, R = scene_args()
    g = scene_swarm(mrs)
    T.set_scan_beams(g, T.scan_ring(8))
    res = restate_visible(pos, worlds, ob, 0, 200, 8, 7.0)
    b0 = g.obstacle_stats()["grid_builds"]
    assert b0 == 0
    cost = torch.zeros(g.n, dtype=torch.float64, device=torch_dev(g))
    for _ in range(3):
        T.obstacle_cost(g, 5.0, out=cost, accumulate=True)
        T.range_scan(g, 12.0)
        T.obstacle_contacts(g, 0.25, hit=True)
        check_visible(T, g, x, v, R, res, 8, 7.0, NN_ALL, torch.float64, 0, 200, label="alternating")
    st = g.obstacle_stats()
    assert st["grid_builds"] == b0 + 4 and st["grid_radius"] == 5.0  # four grids over three rounds; the stats are the queries'
    g.set_obstacles(ob[:100])  # replacing the set drops the entry
    part = restate_visible(pos, worlds, ob[:100], 0, 200, 8, 7.0)
    check_visible(T, g, x, v, R, part, 8, 7.0, NN_ALL, torch.float64, 0, 200, label="replaced set")
    check_visible(T, g, x, v, R, part, 8, 7.0, NN_ALL, torch.float64, 0, 200, label="replaced set, again")
    assert g.obstacle_stats()["grid_builds"] == b0 + 5 and (part["hidden"] != res["hidden"]).any()
    c = g.clone()  # a clone has the set and builds its own grid
    assert c.obstacle_stats()["grid_builds"] == 0 and c.obstacle_stats()["count"] == 100
    check_visible(T, c, x, v, R, part, 8, 7.0, NN_ALL, torch.float64, 0, 200, label="clone")
    assert c.obstacle_stats()["grid_builds"] == 1 and g.obstacle_stats()["grid_builds"] == b0 + 5
    c.close()
    g.close()


# ---- 10. refusals ----

def test_refused_calls_change_nothing(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    g = plain_swarm(mrs, pos[:300])
    g.set_obstacles(ob)
    before = g.get_states()
    dev = torch_dev(g)
    st = torch.cuda.current_stream(dev).cuda_stream
    rows = torch.full((300, 104), SENTINEL, dtype=torch.float64, device=dev)
    index = torch.full((300, 8), -7, dtype=torch.int32, device=dev)
    vecs = [torch.full((300,), -9, dtype=torch.int32, device=dev) for _ in range(3)]
    r, i = rows.data_ptr(), index.data_ptr()
    c, v, h = (t.data_ptr() for t in vecs)
    host = np.zeros(300 * 104)
    hp = host.ctypes.data
    hip = C.CDLL("libamdhip64.so")
    small_p, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(small_p), C.c_size_t(4096)) == 0
    assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), small_p) == 0 and size.value < 4100
    small = small_p.value
    nan, inf = float("nan"), float("inf")
    F, A = T.DTYPE_F64, NN_ALL
    bad = [  # (first, count, k, radius, fields, rows, dtype, stride, index, index_stride, count, visible, hidden), in the documented order:
        ((200, 101, 8, 6.0, A, r, F, 104, i, 8, c, v, h), "error 3:"),  # each case is wrong in what it names and, after the first two, in
        ((-1, 10, 8, 6.0, A, r, F, 104, i, 8, c, v, h), "error 3:"),  # something that a later check would refuse too
        ((0, 301, 8, 6.0, 32, r, F, 104, i, 8, c, v, h), "error 3:"),
        ((0, 300, 0, 6.0, 32, r, F, 104, i, 8, c, v, h), "error 1:.*unknown neighbour field bits"),
        ((0, 300, 0, nan, A, r, F, 104, i, 8, c, v, h), "error 1:.*k must be in"),
        ((0, 300, 33, 6.0, A, r, F, 104, i, 8, c, v, h), "error 1:.*k must be in"),
        ((0, 300, 8, nan, A, 0, F, 104, 0, 8, 0, 0, 0), "error 1:.*radius"),
        ((0, 300, 8, 0.0, A, r, F, 104, i, 8, c, v, h), "error 1:.*radius"),
        ((0, 300, 8, inf, A, r, F, 104, i, 8, c, v, h), "error 1:.*radius"),
        ((0, 300, 8, -6.0, A, r, F, 104, i, 8, c, v, h), "error 1:.*radius"),
        ((0, 300, 8, 6.0, A, 0, 7, 104, 0, 8, 0, 0, 0), "error 1:.*no output given"),
        ((0, 300, 8, 6.0, 0, r, F, 104, 0, 8, 0, 0, 0), "error 1:.*no output given"),
        ((0, 0, 8, 6.0, 0, 0, F, 0, 0, 0, 0, 0, 0), "error 1:.*no output given"),
        ((0, 300, 8, 6.0, A, r, 7, 103, i, 7, c, v, h), "error 1:.*dtype"),
        ((0, 300, 8, 6.0, A, r, F, 103, i, 7, c, v, h), "error 1:.*stride smaller than k"),
        ((0, 300, 8, 6.0, A, r, F, 104, i, 7, hp, v, h), "error 1:.*index_stride smaller than k"),
        ((0, 300, 8, 6.0, A, hp, F, 104, hp, 8, c, v, h), "error 1:.*dev_rows"),
        ((0, 300, 8, 6.0, A, r, F, 104, hp, 8, hp, v, h), "error 1:.*dev_index"),
        ((0, 300, 8, 6.0, A, r, F, 104, i, 8, hp, hp, h), "error 1:.*dev_count"),
        ((0, 300, 8, 6.0, A, r, F, 104, i, 8, c, hp, hp), "error 1:.*dev_visible"),
        ((0, 300, 8, 6.0, A, r, F, 104, i, 8, c, v, hp), "error 1:.*dev_hidden"),
        ((0, 300, 8, 6.0, A, small, F, 104, i, 8, c, v, h), "error 1:.*dev_rows: the rows extend past"),
        ((0, 300, 8, 6.0, A, r, F, 104, small, 8, c, v, h), "error 1:.*dev_index: the rows extend past"),
        ((0, 300, 8, 6.0, A, r, F, 104, i, 8, small + 4096 - 1196, v, h), "error 1:.*dev_count: the rows extend past"),
        ((0, 300, 8, 6.0, A, r, F, 104, i, 8, c, small + 4096 - 1196, h), "error 1:.*dev_visible: the rows extend past"),
        ((0, 300, 8, 6.0, A, r, F, 104, i, 8, c, v, small + 4096 - 1196), "error 1:.*dev_hidden: the rows extend past"),
    ]
    torch.cuda.synchronize(dev)
    for args, msg in bad:
        with pytest.raises(mrs.MrsError, match=msg):
            g.nearest_visible_device(*args, st)
    torch.cuda.synchronize(dev)
    assert hip.hipFree(C.c_void_p(small)) == 0

    def untouched():
        return (rows.cpu().numpy() == SENTINEL).all() and (index.cpu().numpy() == -7).all() and all((t.cpu().numpy() == -9).all() for t in vecs)

    assert untouched() and g.obstacle_stats()["grid_builds"] == 0  # nothing was launched, no grid was built
    g.nearest_visible_device(0, 0, 8, 6.0, A, r, F, 104, i, 8, c, v, h, st)  # count == 0 is MRS_OK and writes nothing
    g.nearest_visible_device(300, 0, 8, 6.0, 0, 0, F, 0, 0, 0, 0, 0, hp, st)  # (the pointers are looked at after it)
    assert untouched() and g.obstacle_stats()["grid_builds"] == 0
    after = g.get_states()
    for key in before.dtype.names:
        assert before[key].tobytes() == after[key].tobytes(), key
    assert not np.asarray(g.has_crashed()).any()
    group = mrs.LoopbackGroup(2)  # a sharded swarm
    shards = []
    for rk in range(2):
        s = mrs.Swarm(100)
        s.construct(0, 100, mrs.model_params("x500"), np.stack([np.arange(100) * 3.0 + 400 * rk, np.zeros(100), np.full(100, 5.0)], axis=1))
        s.comm_init_loopback(group, rk, 200)
        s.set_obstacles(ob[:10])  # (the set itself is legal there)
        shards.append(s)
    for s in shards:
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.nearest_visible(s, 8, 6.0, NN_ALL, out=rows[:100], index=index[:100], counts=vecs[0][:100], visible=vecs[1][:100], hidden=vecs[2][:100])
    assert untouched()
    for s in shards:
        s.close()
    group.close()
    g.close()


# ---- 11. the stream fence and the facade ----

def test_caller_stream_is_fenced(mrs, scene):
    """the outputs are filled on a side stream kept busy by a long sleep, then the call is made with that stream current: they must hold
    the result, not the fill; copies queued behind the call on the side stream read it, and so does another stream that waits for it"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    dev = torch_dev(g)
    x, v, R = scene_args()
    res = first_k(scene_visible(32), 8)
    want_rows = nearest_rows(x, v, R, 0, res["index"], res["d2"], NN_ALL)
    rows = torch.zeros((g.n, 104), dtype=torch.float64, device=dev)
    index = torch.zeros((g.n, 8), dtype=torch.int32, device=dev)
    vecs = [torch.zeros(g.n, dtype=torch.int32, device=dev) for _ in range(3)]
    T.nearest_visible(g, 8, SCENE_RADIUS, 0)  # (the grid is built: the fenced call launches and nothing else)
    torch.cuda.synchronize(dev)
    side, other = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        rows.fill_(SENTINEL)
        index.fill_(-7)
        for t in vecs:
            t.fill_(-9)
        T.nearest_visible(g, 8, SCENE_RADIUS, NN_ALL, out=rows, index=index, counts=vecs[0], visible=vecs[1], hidden=vecs[2])
        copies = [t.clone() for t in [rows, index] + vecs]
    other.wait_stream(side)
    with torch.cuda.stream(other):
        second = [t.clone() for t in [rows, index] + vecs]
    side.synchronize()
    other.synchronize()
    for got in (copies, second):
        r, i, c, vi, h = (t.cpu().numpy() for t in got)
        assert same_bits(r, want_rows) and np.array_equal(i, res["index"]) and np.array_equal(c, res["counts"])
        assert np.array_equal(vi, res["visible"]) and np.array_equal(h, res["hidden"])


def test_cpp_facade_equals_python(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, m, k, stride = 2000, 60, 8, 8 * 4 + 3
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "visible.bin")
        out = subprocess.run([build_cpp("nearest_visible_test"), path], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok visible_equals_brute_force", "ok written"):
            assert tag in out.stdout, out.stdout
        raw = open(path, "rb").read()
    crows = np.frombuffer(raw, np.float64, n * stride, 0).reshape(n, stride)
    o = 8 * n * stride
    cidx = np.frombuffer(raw, np.int32, n * k, o).reshape(n, k)
    o += 4 * n * k
    ccnt, cvis, chid = (np.frombuffer(raw, np.int32, n, o + 4 * n * e) for e in range(3))
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
    rows, index, counts, visible, hidden = T.nearest_visible(g, k, 4.0, NN_REL_POS | NN_DIST, dtype=torch.float64)
    assert same_bits(rows.cpu().numpy(), crows[:, :k * 4]) and (crows[:, k * 4:] == SENTINEL).all()
    assert np.array_equal(index.cpu().numpy(), cidx) and np.array_equal(counts.cpu().numpy(), ccnt)
    assert np.array_equal(visible.cpu().numpy(), cvis) and np.array_equal(hidden.cpu().numpy(), chid)
    assert chid.sum() > 700 and cvis.sum() > 4000  # (the restatement counts 1 512 hidden and 9 288 visible pairs on this scene)
    g.close()
