"""The range scans on the GPU (mrs_swarm_set_scan_beams, mrs_swarm_range_scan_device and their tensor wrappers): every result is compared
on bits with the numpy restatement of test_range_scan.py — the fixture scene of the static obstacles (3 072 UAVs on three airframes with
three ground planes, 384 obstacles of all kinds, two world labels, UAVs inside solids, two non-finite UAVs) with 1, 7, 16, 64 and 100
beams, both frames, with and without the ground, FP64 and FP32, ranges and hit indices, padded strides and partial ranges; scans of
2, 8 and 40 m (three different grids) agree wherever they can; the ground beam agrees with the rangefinder payload; the scans' grid
cache; a scan between the pieces of a cost tick rollout; clones, replaced and cleared patterns; refusals that change nothing; the
caller's stream fence; and the C++ facade (tests/cpp/range_scan_test.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import helpers
from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_obstacles import OBSTACLE, fixture_scene, grid_of, same_bits
from test_obstacles_gpu import AIRFRAMES, SENTINEL, plain_swarm, scene_state
from test_range_scan import GROUND, HIT_GROUND, HIT_NONE, mixed_beams, restate_scan
from test_rollout_gpu import DT, REBOUNCE
from test_rollout_tick_cost_gpu import make_targets
from test_rollout_tick_gpu import N_PAIR, assert_same_swarm, pair_state, pair_swarm

pytestmark = pytest.mark.gpu
MAX_RANGE = 6.0
GROUND_Z = (-1.0, 0.5, 2.0)  # per airframe of the scene; the middle one with ground_enabled off (the scan reads ground_z whatever it says)
_ref = {}


def scene_ground_z():
    n = len(fixture_scene()[0])
    third = n // 3
    return np.repeat(GROUND_Z, [third, third, n - 2 * third])


def scene_swarm(mrs):
    """the fixture scene on three airframes with three ground planes, random tilted flight states, labels and obstacles set"""
    pos, worlds, ob = fixture_scene()
    n = len(pos)
    g = mrs.Swarm(n, arith=mrs.ARITH_FAST)
    third = n // 3
    st = {k: v.copy() for k, v in scene_state().items()}
    for a, name in enumerate(AIRFRAMES):
        first, count = a * third, (n - 2 * third if a == 2 else third)
        g.construct(first, count, mrs.model_params(name, ground_enabled=a != 1, ground_z=GROUND_Z[a]),
                    np.nan_to_num(pos[first:first + count], posinf=0.0, neginf=0.0))
        st["motor_rpm"][first:first + count, mrs.AIRFRAMES[name]["n_motors"]:] = 0.0
    g.set_state(0, n, pos, st["v"], st["R"], st["omega"], st["motor_rpm"])
    s = g.get_states()
    assert same_bits(np.nan_to_num(s["x"], nan=7.0), np.nan_to_num(pos, nan=7.0)) and same_bits(s["R"].reshape(n, 9), st["R"].reshape(n, 9))
    g.set_obstacles(ob)
    g.set_worlds(worlds)
    return g


def fixture_ref(nb, body, ground, max_range=MAX_RANGE):
    """the restatement of the fixture scene for mixed_beams(nb), computed once per (nb, frame) and shared (never written to)"""
    pos, worlds, ob = fixture_scene()
    R = scene_state()["R"].reshape(-1, 3, 3)
    key = (nb, body, max_range)
    if key not in _ref:
        _ref[key] = restate_scan(pos, R, worlds, ob, mixed_beams(nb), max_range, body)
    if ground and key + (1,) not in _ref:
        _ref[key + (1,)] = restate_scan(pos, R, worlds, ob, mixed_beams(nb), max_range, body, ground_z=scene_ground_z(), base=_ref[key])
    res = _ref[key + (1,)] if ground else _ref[key]
    for a in res:
        a.setflags(write=False)
    return res


def run_scan(T, g, max_range, body, ground, dtype, first=0, count=None, pad=3, hpad=2, hits=True):
    """one tensors.range_scan call into padded, sentinel-filled tensors: (ranges [count, B], hit [count, B]) as numpy; the slack columns and
    the rows around the range must come back untouched"""
    import torch
    count = g.n - first if count is None else count
    nb = len(g.get_scan_beams())
    dev = torch_dev(g)
    out = torch.full((count + 2, nb + pad), SENTINEL, dtype=dtype, device=dev)
    hit = torch.full((count + 2, nb + hpad), -7, dtype=torch.int32, device=dev)
    r, h = T.range_scan(g, max_range, body, ground, first, count, out=out[1:count + 1], hits=hit[1:count + 1] if hits else None)
    ho, hh = out.cpu().numpy(), hit.cpu().numpy()
    fill = np.float32(SENTINEL) if dtype == torch.float32 else SENTINEL
    assert (ho[0] == fill).all() and (ho[count + 1] == fill).all() and (ho[:, nb:] == fill).all(), "range slack was touched"
    assert r.shape == (count, nb) and r.data_ptr() == out[1:].data_ptr()
    if hits:
        assert (hh[0] == -7).all() and (hh[count + 1] == -7).all() and (hh[:, nb:] == -7).all(), "hit slack was touched"
        assert h.shape == (count, nb) and h.dtype == torch.int32
    else:
        assert h is None and (hh == -7).all()
    return ho[1:count + 1, :nb], hh[1:count + 1, :nb]


def check_scan(T, g, res, max_range, body, ground, dtype, first=0, count=None, label=""):
    import torch
    count = g.n - first if count is None else count
    sl = slice(first, first + count)
    ranges, hit = run_scan(T, g, max_range, body, ground, dtype, first, count)
    assert np.array_equal(hit, res[1][sl]), (label, "hit", np.argwhere(hit != res[1][sl])[:5])
    want = res[0][sl].astype(np.float64 if dtype == torch.float64 else np.float32)
    assert same_bits(ranges, want), (label, "ranges", np.argwhere(ranges != want)[:5])


@pytest.fixture(scope="module")
def scene(mrs):
    return scene_swarm(mrs)


@pytest.mark.parametrize("nb", [1, 7, 16, 64, 100])
def test_scan_exact_against_numpy(mrs, scene, nb):
    """1 beam; 7: a wave straddles UAVs at a moving offset; 16; 64; 100: one UAV spans waves"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    T.set_scan_beams(g, mixed_beams(nb))
    assert same_bits(g.get_scan_beams(), mixed_beams(nb))
    for body in (True, False):
        for ground in (False, True):
            res = fixture_ref(nb, body, ground)
            for dtype in (torch.float64, torch.float32):
                check_scan(T, g, res, MAX_RANGE, body, ground, dtype, label=(nb, body, ground, dtype))
    ranges, hit = fixture_ref(nb, True, True)
    if nb >= 7:  # every outcome occurs: obstacles of every kind, the ground, nothing, origins inside solids, the non-finite UAVs
        ob = fixture_scene()[2]
        assert set(ob["kind"][hit[hit >= 0]]) == {0, 1, 2} and (hit == HIT_GROUND).sum() > 100 and (hit == HIT_NONE).sum() > 1000
        assert ((hit >= 0) & (ranges == 0.0)).sum() > 100 and (ranges[200:202] == MAX_RANGE).all() and (hit[200:202] == HIT_NONE).all()
        assert (fixture_ref(nb, True, False)[1] != fixture_ref(nb, False, False)[1]).sum() > 100  # the frame matters


def test_partial_ranges_strides_and_defaults(mrs, scene):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    T.set_scan_beams(g, mixed_beams(7))
    for first, count in ((0, 1), (1000, 517), (g.n - 37, 37)):  # count * 7 is no multiple of 256
        assert (count * 7) % 256 != 0
        check_scan(T, g, fixture_ref(7, True, True), MAX_RANGE, True, True, torch.float64, first, count, label=(first, count))
        check_scan(T, g, fixture_ref(7, False, False), MAX_RANGE, False, False, torch.float32, first, count, label=(first, count, "world"))
    T.set_scan_beams(g, mixed_beams(100))
    check_scan(T, g, fixture_ref(100, True, True), MAX_RANGE, True, True, torch.float32, 2001, 333, label="100 beams, a range")
    # without hits; and the defaults: new tensors, body frame, no ground, FP32, no hits
    T.set_scan_beams(g, mixed_beams(16))
    ranges, _ = run_scan(T, g, MAX_RANGE, True, False, torch.float64, hits=False)
    assert same_bits(ranges, fixture_ref(16, True, False)[0])
    r, h = T.range_scan(g, MAX_RANGE)
    assert h is None and r.dtype == torch.float32 and r.shape == (g.n, 16) and same_bits(r.cpu().numpy(), fixture_ref(16, True, False)[0].astype(np.float32))
    r, h = T.range_scan(g, MAX_RANGE, ground=True, hits=True, dtype=torch.float64)
    assert same_bits(r.cpu().numpy(), fixture_ref(16, True, True)[0]) and np.array_equal(h.cpu().numpy(), fixture_ref(16, True, True)[1])


def test_grid_independence(mrs, scene):
    """max_range 2, 8 and 40 force three different grids; wherever the longer scan's range is below the shorter max_range the shorter scan
    returns the same bits and index, elsewhere its max_range and HIT_NONE"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    ob = fixture_scene()[2]
    assert len({grid_of(ob, r)["dims"] for r in (2.0, 8.0, 40.0)}) == 3
    T.set_scan_beams(g, mixed_beams(16))
    for ground in (False, True):
        got = {r: run_scan(T, g, r, True, ground, torch.float64) for r in (40.0, 8.0, 2.0)}
        for long, short in ((40.0, 8.0), (40.0, 2.0), (8.0, 2.0)):
            (rl, hl), (rs, hs) = got[long], got[short]
            near = rl < short
            assert near.sum() > 1000 and (~near).sum() > 1000
            assert same_bits(rs[near], rl[near]) and np.array_equal(hs[near], hl[near]), (long, short, ground)
            assert (rs[~near] == short).all() and (hs[~near] == HIT_NONE).all(), (long, short, ground)
    # and the 8-m scan is the restatement's
    check_scan(T, g, fixture_ref(16, True, True, 8.0), 8.0, True, True, torch.float64, label="8 m")


def test_ground_beam_agrees_with_the_rangefinder(mrs):
    """no obstacles, one body beam (0, 0, -1), the ground, max_range 40, tilted hovering UAVs: the rangefinder payload computes
    (z - ground_z) / cos(acos(R22)) + 0.01, the scan (z - ground_z) / R22 — a few ulps apart"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n = 2000
    rng = np.random.default_rng(77)
    st = helpers.random_state(rng, n, 4, box=50.0, zlo=0.5, zhi=45.0, tilted=True)
    g = mrs.Swarm(n)
    g.construct(0, n // 2, mrs.model_params("x500", ground_z=0.0), st["x"][:n // 2])
    g.construct(n // 2, n - n // 2, mrs.model_params("x500", ground_z=-3.0), st["x"][n // 2:])
    g.set_state(0, n, st["x"], None, st["R"], None, None)
    T.set_scan_beams(g, [[0.0, 0.0, -1.0]])
    r, h = T.range_scan(g, 40.0, ground=True, hits=True, dtype=torch.float64)
    r, h = r.cpu().numpy()[:, 0], h.cpu().numpy()[:, 0]
    finder = g.get_outputs()["range"]
    below = finder < 40.0
    assert below.sum() > 1000 and (~below).sum() > 20
    want = finder[below] - 0.01
    assert (np.abs(r[below] - want) <= 1e-12 * np.abs(want)).all(), np.abs(r[below] / want - 1.0).max()
    assert (h[below] == HIT_GROUND).all() and (h[r == 40.0] == HIT_NONE).all() and ((h == HIT_GROUND) == (r < 40.0)).all()


def test_scan_grid_cache(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    g = plain_swarm(mrs, pos[:500])
    g.set_obstacles(ob)
    T.set_scan_beams(g, T.scan_ring(8))
    assert g.obstacle_stats()["grid_builds"] == 0
    for rep in range(3):  # two grids, not one per call
        T.obstacle_cost(g, 5.0)
        T.range_scan(g, 12.0)
        st = g.obstacle_stats()
        assert st["grid_builds"] == 2 and st["grid_radius"] == 5.0 and st["cell_edge"] == 10.0, (rep, st)  # the stats describe the queries' grid
    first = T.range_scan(g, 12.0, dtype=torch.float64, hits=True)
    T.range_scan(g, 3.0)  # another range: another scan grid, the queries' grid stays
    assert g.obstacle_stats()["grid_builds"] == 3
    T.obstacle_cost(g, 5.0)
    assert g.obstacle_stats()["grid_builds"] == 3
    g.set_obstacles(ob[::2])  # replacing the set drops both
    assert g.obstacle_stats()["grid_builds"] == 3 and g.obstacle_stats()["cells"] == 0
    T.obstacle_cost(g, 5.0)
    r, h = T.range_scan(g, 3.0, dtype=torch.float64, hits=True)
    assert g.obstacle_stats()["grid_builds"] == 5
    x = g.get_states()["x"]
    want = restate_scan(x, None, None, ob[::2], T.scan_ring(8), 3.0)
    assert same_bits(r.cpu().numpy(), want[0]) and np.array_equal(h.cpu().numpy(), want[1])
    g.set_obstacles(ob)
    again = T.range_scan(g, 12.0, dtype=torch.float64, hits=True)
    assert same_bits(again[0].cpu().numpy(), first[0].cpu().numpy()) and torch.equal(again[1], first[1])
    want = restate_scan(x, None, None, ob, T.scan_ring(8), 12.0)
    assert same_bits(again[0].cpu().numpy(), want[0]) and np.array_equal(again[1].cpu().numpy(), want[1])


@pytest.mark.parametrize("crash", [False, True], ids=["elastic", "crash"])
@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
def test_inside_a_horizon(mrs, arith, crash):
    """rollout_tick_cost over 48 ticks: one swarm runs them cut into 24 + 24 with accumulate, sets a pattern and scans at the cut and after
    the end; its twin runs the uncut horizon in one call and nothing else: final state, crash flags and cost vectors are the twin's bit
    for bit (the pending collision tick stays pending), and the scans are the restatement's of the positions and attitudes at that point"""
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
    beams = np.concatenate([T.scan_ring(8), [[0.0, 0.0, -1.0]]])
    hits = 0
    for piece in range(2):
        sl = slice(piece * half, (piece + 1) * half)
        T.rollout_tick_cost(a, O.POSITION_CMD, cmd[sl], DT, crash, REBOUNCE, groups, tg[sl], wt[sl], 1000.0, hold=hold, out=costs[id(a)],
                            accumulate=True)
        obs = T.gather(a, T.OBS_POS | T.OBS_ROT, dtype=torch.float64).cpu().numpy()
        T.set_scan_beams(a, beams)  # the setter too leaves the pending collision tick pending
        r, h = T.range_scan(a, 7.5, ground=True, hits=True, dtype=torch.float64)
        want = restate_scan(obs[:, :3], obs[:, 3:12].reshape(-1, 3, 3), None, ob, beams, 7.5, ground_z=np.zeros(N_PAIR))
        assert same_bits(r.cpu().numpy(), want[0]) and np.array_equal(h.cpu().numpy(), want[1]), piece
        hits += int((want[1] >= 0).sum())
        assert (want[1][:, 8] == HIT_GROUND).sum() > 100
    assert hits > 100
    T.rollout_tick_cost(b, O.POSITION_CMD, cmd, DT, crash, REBOUNCE, groups, tg, wt, 1000.0, hold=hold, out=costs[id(b)],
                        accumulate=True)  # the uncut horizon
    assert same_bits(costs[id(a)].cpu().numpy(), costs[id(b)].cpu().numpy())
    if crash:
        assert np.asarray(a.has_crashed()).any()
    assert_same_swarm(a, b, f"{arith} crash={crash}: with and without the scans")
    for g in (a, b):
        g.tick_n(DT, 1, True, crash, REBOUNCE)  # evaluates the collision tick the horizon left pending
    assert_same_swarm(a, b, f"{arith} crash={crash}: one more tick on both")


def test_lifetime_clone_replace_and_clear(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    sel = slice(0, 600)
    R = scene_state()["R"].reshape(-1, 3, 3)[sel]
    g = plain_swarm(mrs, pos[sel], R)
    g.set_worlds(worlds[sel])
    g.set_obstacles(ob)
    x = g.get_states()["x"]
    assert g.get_scan_beams().shape == (0, 3)
    ring, grid = T.scan_ring(12, 0.2), T.scan_grid(5, 3, 1.2, 0.8)

    def check(s, beams, label, xs=x, Rs=R, ws=worlds[sel]):
        r, h = T.range_scan(s, MAX_RANGE, dtype=torch.float64, hits=True)
        want = restate_scan(xs, Rs, ws, ob, beams, MAX_RANGE)
        assert same_bits(r.cpu().numpy(), want[0]) and np.array_equal(h.cpu().numpy(), want[1]), label

    T.set_scan_beams(g, ring)
    assert same_bits(g.get_scan_beams(), ring) and g.scan_beam_count() == 12
    # a capacity below the pattern is refused, the size still written; out == NULL asks for the size alone
    L, size, small = mrs.load_library(), C.c_int32(-1), np.full((11, 3), 7.0)
    assert L.mrs_swarm_get_scan_beams(g._h, 11, small.ctypes.data_as(C.c_void_p), C.byref(size)) == 1 and size.value == 12 and (small == 7.0).all()
    assert L.mrs_swarm_get_scan_beams(g._h, 12, None, None) == 1
    size = C.c_int32(-1)
    assert L.mrs_swarm_get_scan_beams(g._h, 0, None, C.byref(size)) == 0 and size.value == 12
    check(g, ring, "set")
    # the clone owns a copy: it answers like the original, and goes on doing so after the original's pattern is replaced
    c, big = g.clone(), g.clone_resized(700)
    assert same_bits(c.get_scan_beams(), ring) and same_bits(big.get_scan_beams(), ring)
    T.set_scan_beams(g, grid)
    assert same_bits(g.get_scan_beams(), grid) and same_bits(c.get_scan_beams(), ring)
    check(g, grid, "replaced")
    check(c, ring, "clone")
    sb = big.get_states()
    check(big, ring, "resized clone", sb["x"], sb["R"].reshape(-1, 3, 3), np.concatenate([worlds[sel], np.zeros(100, np.int32)]))
    # a refused pattern changes nothing
    for bad in (np.array([[1.0, 0.0, 1e-4]]), np.array([[np.nan, 0.0, 0.0]]), np.zeros((1, 3)), np.tile(ring[:1], (4097, 1))):
        with pytest.raises(mrs.MrsError, match="error 1:"):
            g.set_scan_beams(bad)
    assert same_bits(g.get_scan_beams(), grid)
    check(g, grid, "after refusals")
    # cleared: the scan is refused, the setter takes a new pattern
    g.set_scan_beams(None)
    assert g.get_scan_beams().shape == (0, 3)
    with pytest.raises(mrs.MrsError, match="error 1:.*no beam pattern"):
        g.range_scan_device(0, 600, MAX_RANGE, 0, 1, 0, 16, 0, 0, 0)
    T.set_scan_beams(g, ring[:5])
    check(g, ring[:5], "set again")
    # an empty obstacle set is legal: the ground or nothing
    g.set_obstacles(None)
    r, h = T.range_scan(g, MAX_RANGE, ground=True, hits=True, dtype=torch.float64)
    want = restate_scan(x, R, None, ob[:0], ring[:5], MAX_RANGE, ground_z=np.zeros(600))
    assert same_bits(r.cpu().numpy(), want[0]) and np.array_equal(h.cpu().numpy(), want[1]) and (want[1] == HIT_GROUND).any()
    for s in (g, c, big):
        s.close()


def test_refused_calls_change_nothing(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    g = plain_swarm(mrs, pos[:300])
    g.set_obstacles(ob)
    dev = torch_dev(g)
    st = torch.cuda.current_stream(dev).cuda_stream
    ranges = torch.full((300, 16), SENTINEL, dtype=torch.float64, device=dev)
    hit = torch.full((300, 16), -7, dtype=torch.int32, device=dev)
    r, h = ranges.data_ptr(), hit.data_ptr()
    with pytest.raises(mrs.MrsError, match="error 1:.*no beam pattern"):
        g.range_scan_device(0, 300, 5.0, 0, r, 0, 16, h, 16, st)
    T.set_scan_beams(g, mixed_beams(16))
    before = g.get_states()
    host = np.zeros(300 * 16)
    hip = C.CDLL("libamdhip64.so")
    small_p, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(small_p), C.c_size_t(4096)) == 0
    assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), small_p) == 0 and size.value < 4100
    small = small_p.value
    nan, inf = float("nan"), float("inf")
    bad = [
        ((200, 101, 5.0, 3, r, 0, 16, h, 16), "error 3:"),
        ((-1, 10, 5.0, 3, r, 0, 16, h, 16), "error 3:"),
        ((0, 300, 0.0, 3, r, 0, 16, h, 16), "error 1:.*max_range"),
        ((0, 300, -2.0, 3, r, 0, 16, h, 16), "error 1:.*max_range"),
        ((0, 300, nan, 3, r, 0, 16, h, 16), "error 1:.*max_range"),
        ((0, 300, inf, 3, r, 0, 16, h, 16), "error 1:.*max_range"),
        ((0, 300, 5.0, 4, r, 0, 16, h, 16), "error 1:.*unknown scan flag bits"),
        ((0, 300, 5.0, 0x80000001, r, 0, 16, h, 16), "error 1:.*unknown scan flag bits"),
        ((0, 300, 5.0, 3, r, 7, 16, h, 16), "error 1:.*dtype"),
        ((0, 300, 5.0, 3, r, 0, 15, h, 16), "error 1:.*stride smaller"),
        ((0, 300, 5.0, 3, r, 0, 16, h, 15), "error 1:.*hit_stride smaller"),
        ((0, 300, 5.0, 3, 0, 0, 16, h, 16), "error 1:.*dev_ranges: null pointer"),
        ((0, 0, 5.0, 3, 0, 0, 16, h, 16), "error 1:.*dev_ranges: null pointer"),
        ((0, 300, 5.0, 3, host.ctypes.data, 0, 16, h, 16), "error 1:.*dev_ranges"),
        ((0, 300, 5.0, 3, r, 0, 16, host.ctypes.data, 16), "error 1:.*dev_hit"),
        ((0, 300, 5.0, 3, small, 0, 16, h, 16), "error 1:.*dev_ranges: the rows extend past"),
        ((0, 300, 5.0, 3, r, 0, 16, small, 16), "error 1:.*dev_hit: the rows extend past"),
    ]
    torch.cuda.synchronize(dev)
    for args, msg in bad:
        with pytest.raises(mrs.MrsError, match=msg):
            g.range_scan_device(*args, st)
    torch.cuda.synchronize(dev)
    assert hip.hipFree(C.c_void_p(small)) == 0

    def untouched():
        return (ranges.cpu().numpy() == SENTINEL).all() and (hit.cpu().numpy() == -7).all()

    assert untouched() and g.obstacle_stats()["grid_builds"] == 0  # nothing was launched, no grid was built
    g.range_scan_device(0, 0, 5.0, 3, r, 0, 16, h, 16, st)  # count == 0 is MRS_OK and writes nothing
    g.range_scan_device(300, 0, 5.0, 3, r, 0, 16, 0, 0, st)
    assert untouched() and g.obstacle_stats()["grid_builds"] == 0
    after = g.get_states()
    for key in before.dtype.names:
        assert before[key].tobytes() == after[key].tobytes(), key
    # a sharded swarm: the pattern is legal there, the scan is not
    group = mrs.LoopbackGroup(2)
    shards = []
    for rk in range(2):
        s = mrs.Swarm(100)
        s.construct(0, 100, mrs.model_params("x500"), np.stack([np.arange(100) * 3.0 + 400 * rk, np.zeros(100), np.full(100, 5.0)], axis=1))
        s.comm_init_loopback(group, rk, 200)
        s.set_scan_beams(mixed_beams(16))
        shards.append(s)
    for s in shards:
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.range_scan(s, 5.0, out=ranges[:100])
    assert untouched()
    for s in shards:
        s.close()
    group.close()


def test_caller_stream_is_fenced(mrs, scene):
    """the outputs are filled on a side stream kept busy by a long sleep, then the scan is made with that stream current: the rows must
    hold the result (the kernel ran after the fill), and copies queued behind the call on the side stream read it"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    dev = torch_dev(g)
    T.set_scan_beams(g, mixed_beams(16))
    res = fixture_ref(16, True, True)
    ranges = torch.zeros((g.n, 16), dtype=torch.float64, device=dev)
    hit = torch.zeros((g.n, 16), dtype=torch.int32, device=dev)
    T.range_scan(g, MAX_RANGE, ground=True)  # (the grid is built: the fenced call launches and nothing else)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        ranges.fill_(SENTINEL)
        hit.fill_(-7)
        T.range_scan(g, MAX_RANGE, ground=True, out=ranges, hits=hit)
        rcopy, hcopy = ranges.clone(), hit.clone()
    side.synchronize()
    assert same_bits(rcopy.cpu().numpy(), res[0]) and np.array_equal(hcopy.cpu().numpy(), res[1])


def test_cpp_facade_equals_python(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, m, nb = 2000, 60, 10
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "scan.bin")
        out = subprocess.run([build_cpp("range_scan_test"), path], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok range_scan_equals_brute_force", "ok written"):
            assert tag in out.stdout, out.stdout
        raw = open(path, "rb").read()
    cr = np.frombuffer(raw, np.float64, n * nb, 0).reshape(n, nb)
    ch = np.frombuffer(raw, np.int32, n * nb, 8 * n * nb).reshape(n, nb)
    i = np.arange(n)
    pos = np.stack([3.1 * (i % 20) + 0.01 * (i % 7), 2.9 * ((i // 20) % 20) - 0.02 * (i % 5), 3.3 * (i // 400) + 0.005 * (i % 11)], axis=1)
    j = np.arange(m)
    ob = np.zeros(m, OBSTACLE)
    ob["kind"] = j % 3
    ob["c"] = np.stack([6.2 * (j % 8) + 0.5, 7.1 * ((j // 8) % 8) - 0.25, 3.0 + 1.5 * (j % 4)], axis=1)
    ob["h"] = np.stack([1.4 + 0.3 * (j % 5), 1.3 + 0.4 * (j % 3), np.where(j % 6 == 2, np.inf, 2.0 + 0.5 * (j % 4))], axis=1)
    beams = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.6, 0.8, 0.0],
                      [0.0, -0.6, -0.8], [-0.8, 0.0, 0.6], [0.28, -0.96, 0.0]])
    g = mrs.Swarm(n)
    g.construct(0, n, mrs.model_params("x500"), pos)
    g.set_obstacles(ob)
    T.set_scan_beams(g, beams)
    r, h = T.range_scan(g, 9.0, ground=True, hits=True, dtype=torch.float64)
    assert same_bits(r.cpu().numpy(), cr) and np.array_equal(h.cpu().numpy(), ch)
    assert (ch >= 0).any() and (ch == HIT_GROUND).any() and (ch == HIT_NONE).any() and GROUND == T.SCAN_GROUND
