"""The range scans that see other UAVs on the GPU (mrs_swarm_range_scan_uavs_device and tensors.range_scan_uavs): every result is compared
on bits with the numpy restatement of test_range_scan_uavs.py — the fixture scene of the range scans (3 072 UAVs on three airframes of
three radii, two world labels, 384 obstacles, the 64-UAV cluster, two non-finite UAVs) with 1, 7, 64 and 100 beams, both frames, with and
without the ground, FP64 and FP32, ranges, hit values and UAV indices; more candidates than two chunks; scans of 2, 6 and 20 m (three
hash edges) agree wherever they can; swarms without labels and with labels set later; a 40-UAV swarm whose probes share buckets;
partial ranges, padded strides, either index output without the other; agreement with the old call where no UAV is near; moved UAVs; a
scan between the pieces of a cost tick rollout; alternation with nearest and proximity_cost; clones; refusals that change nothing; the
caller's stream fence; and the C++ facade (tests/cpp/range_scan_uavs_test.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_obstacles import OBSTACLE, fixture_scene, same_bits
from test_obstacles_gpu import SENTINEL, plain_swarm, scene_state
from test_range_scan import HIT_GROUND, HIT_NONE, mixed_beams, restate_scan
from test_range_scan_gpu import MAX_RANGE, fixture_ref, scene_ground_z, scene_swarm
from test_range_scan_uavs import HIT_UAV, candidate_pairs, restate_scan_uavs, scene_radii
from test_rollout_gpu import DT, REBOUNCE
from test_rollout_tick_cost_gpu import make_targets
from test_rollout_tick_gpu import N_PAIR, assert_same_swarm, pair_state, pair_swarm

pytestmark = pytest.mark.gpu
CHUNK = 256  # RU_CAP of csrc/range_scan_uavs.hip: entries of the candidate chunk in LDS
X500 = 0.25 + 0.15  # arm_length + prop_radius of the x500 (plain_swarm, pair_swarm)
_ref = {}


def uav_ref(nb, body, ground, max_range=MAX_RANGE):
    """the restatement of the fixture scene for mixed_beams(nb), computed once per key and shared (never written to)"""
    key = (nb, body, ground, max_range)
    if key not in _ref:
        pos, worlds, ob = fixture_scene()
        R = scene_state()["R"].reshape(-1, 3, 3)
        base = fixture_ref(nb, body, False, max_range)
        _ref[key] = restate_scan_uavs(pos, R, worlds, scene_radii(), ob, mixed_beams(nb), max_range, body,
                                      ground_z=scene_ground_z() if ground else None, base=base)
        for a in _ref[key]:
            a.setflags(write=False)
    return _ref[key]


def run_scan(T, g, max_range, body, ground, dtype, first=0, count=None, pads=(3, 2, 5), hits=True, uavs=True):
    """one tensors.range_scan_uavs call into padded, sentinel-filled tensors: (ranges, hit, uav) [count, B] as numpy; the slack columns and
    the rows around the range must come back untouched, and an output that is not asked for is not written at all"""
    import torch
    count = g.n - first if count is None else count
    nb = len(g.get_scan_beams())
    dev = torch_dev(g)
    out = torch.full((count + 2, nb + pads[0]), SENTINEL, dtype=dtype, device=dev)
    hit = torch.full((count + 2, nb + pads[1]), -7, dtype=torch.int32, device=dev)
    uav = torch.full((count + 2, nb + pads[2]), -9, dtype=torch.int32, device=dev)
    r, h, w = T.range_scan_uavs(g, max_range, body, ground, first, count, out=out[1:count + 1], hits=hit[1:count + 1] if hits else None,
                                uavs=uav[1:count + 1] if uavs else None)
    ho, hh, hw = out.cpu().numpy(), hit.cpu().numpy(), uav.cpu().numpy()
    fill = np.float32(SENTINEL) if dtype == torch.float32 else SENTINEL
    assert (ho[0] == fill).all() and (ho[count + 1] == fill).all() and (ho[:, nb:] == fill).all(), "range slack was touched"
    assert r.shape == (count, nb) and r.data_ptr() == out[1:].data_ptr()
    for name, asked, got, host, mark in (("hit", hits, h, hh, -7), ("uav", uavs, w, hw, -9)):
        if asked:
            assert (host[0] == mark).all() and (host[count + 1] == mark).all() and (host[:, nb:] == mark).all(), name + " slack was touched"
            assert got.shape == (count, nb) and got.dtype == torch.int32
        else:
            assert got is None and (host == mark).all(), name
    return ho[1:count + 1, :nb], hh[1:count + 1, :nb], hw[1:count + 1, :nb]


def check_scan(T, g, res, max_range, body, ground, dtype, first=0, count=None, label="", **kw):
    import torch
    count = g.n - first if count is None else count
    sl = slice(first, first + count)
    ranges, hit, uav = run_scan(T, g, max_range, body, ground, dtype, first, count, **kw)
    if kw.get("hits", True):
        assert np.array_equal(hit, res[1][sl]), (label, "hit", np.argwhere(hit != res[1][sl])[:5])
    if kw.get("uavs", True):
        assert np.array_equal(uav, res[2][sl]), (label, "uav", np.argwhere(uav != res[2][sl])[:5])
    want = res[0][sl].astype(np.float64 if dtype == torch.float64 else np.float32)
    assert same_bits(ranges, want), (label, "ranges", np.argwhere(ranges != want)[:5])


def check_plain(T, g, x, R, worlds, ob, beams, max_range, label, rad=X500, ground_z=None):
    """a scan of every UAV of g (FP64, both index outputs) against the restatement of what g holds"""
    import torch
    r, h, w = T.range_scan_uavs(g, max_range, ground=ground_z is not None, hits=True, uavs=True, dtype=torch.float64)
    want = restate_scan_uavs(x, R, worlds, rad, ob, beams, max_range, ground_z=ground_z)
    assert same_bits(r.cpu().numpy(), want[0]) and np.array_equal(h.cpu().numpy(), want[1]) and np.array_equal(w.cpu().numpy(), want[2]), label
    return want


@pytest.fixture(scope="module")
def scene(mrs):
    return scene_swarm(mrs)


@pytest.mark.parametrize("nb", [1, 7, 64, 100])
def test_scan_exact_against_numpy(mrs, scene, nb):
    """1 beam; 7; 64: one full beam group; 100: two beam groups, the second partly filled"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    T.set_scan_beams(g, mixed_beams(nb))
    for body in (True, False):
        for ground in (False, True):
            res = uav_ref(nb, body, ground)
            for dtype in (torch.float64, torch.float32):
                check_scan(T, g, res, MAX_RANGE, body, ground, dtype, label=(nb, body, ground, dtype))
    # every outcome occurs (bounds: about half of what the restatement counts per beam on this scene: 119 UAV hits, 10 at range 0,
    # 15 that beat an obstacle, 62 where an obstacle keeps the beam from a UAV)
    pos, worlds, ob = fixture_scene()
    r0, h0 = fixture_ref(nb, False, False)
    r, h, w = uav_ref(nb, False, False)
    on_uav = h == HIT_UAV
    assert on_uav.sum() >= 55 * nb and (on_uav & (r == 0.0)).sum() >= 4 * nb and (on_uav & (h0 >= 0)).sum() >= 6 * nb, \
        (on_uav.sum(), (on_uav & (r == 0.0)).sum(), (on_uav & (h0 >= 0)).sum())
    if nb == 7:
        hu = restate_scan_uavs(pos, None, worlds, scene_radii(), ob[:0], mixed_beams(nb), MAX_RANGE, False)[1]
        assert ((hu == HIT_UAV) & (h >= 0)).sum() >= 28 * nb
        assert np.bincount(candidate_pairs(pos, worlds, scene_radii(), MAX_RANGE)[0]).max() >= 38
    assert (h[200:202] == HIT_NONE).all() and (w[200:202] == -1).all() and (r[200:202] == MAX_RANGE).all()
    rg, hg, wg = uav_ref(nb, True, True)
    assert (hg == HIT_GROUND).sum() > 10 * nb and (wg[hg != HIT_UAV] == -1).all() and (wg[hg == HIT_UAV] >= 0).all()


def test_more_candidates_than_two_chunks(mrs, scene):
    """observers [0, 128) at 20 m: the gather fills the chunk and sweeps it several times per observer"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    pos, worlds, ob = fixture_scene()
    obs = np.arange(128)
    most = np.bincount(candidate_pairs(pos, worlds, scene_radii(), 20.0, obs)[0]).max()
    assert most > 2 * CHUNK, most
    T.set_scan_beams(g, mixed_beams(16))
    R = scene_state()["R"].reshape(-1, 3, 3)
    want = restate_scan_uavs(pos, R, worlds, scene_radii(), ob, mixed_beams(16), 20.0, True, ground_z=scene_ground_z(), observers=obs)
    assert (want[1] == HIT_UAV).sum() >= 15  # (the restatement counts 30: most of these observers stand in the obstacle cluster)
    ranges, hit, uav = run_scan(T, g, 20.0, True, True, torch.float64, 0, 128)
    assert same_bits(ranges, want[0]) and np.array_equal(hit, want[1]) and np.array_equal(uav, want[2])


def test_hash_edge_independence(mrs, scene):
    """max_range 2, 6 and 20 force three hash edges (and three obstacle grids); wherever the longer scan's range is below the shorter
    max_range the shorter scan returns the same bits, hit value and UAV, elsewhere its max_range, HIT_NONE and -1"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    T.set_scan_beams(g, mixed_beams(16))
    for ground in (False, True):
        got = {r: run_scan(T, g, r, True, ground, torch.float64) for r in (20.0, 6.0, 2.0)}
        for long, short in ((20.0, 6.0), (20.0, 2.0), (6.0, 2.0)):
            (rl, hl, wl), (rs, hs, ws) = got[long], got[short]
            near = rl < short
            assert near.sum() > 1000 and (~near).sum() > 1000 and (hl[near] == HIT_UAV).sum() > 50
            assert same_bits(rs[near], rl[near]) and np.array_equal(hs[near], hl[near]) and np.array_equal(ws[near], wl[near]), (long, short, ground)
            assert (rs[~near] == short).all() and (hs[~near] == HIT_NONE).all() and (ws[~near] == -1).all(), (long, short, ground)
        res = uav_ref(16, True, ground)
        assert same_bits(got[6.0][0], res[0]) and np.array_equal(got[6.0][1], res[1]) and np.array_equal(got[6.0][2], res[2])


def test_without_labels_and_labels_set_after_a_first_call(mrs):
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    sel = slice(0, 700)
    R = scene_state()["R"].reshape(-1, 3, 3)[sel]
    g = plain_swarm(mrs, pos[sel], R)
    g.set_obstacles(ob)
    T.set_scan_beams(g, mixed_beams(16))
    a = check_plain(T, g, pos[sel], R, None, ob, mixed_beams(16), MAX_RANGE, "no labels")  # the kernel without the label column
    g.set_worlds(worlds[sel])
    b = check_plain(T, g, pos[sel], R, worlds[sel], ob, mixed_beams(16), MAX_RANGE, "labels set after the first call")
    assert (a[1] == HIT_UAV).sum() > (b[1] == HIT_UAV).sum() >= 29  # (the restatement counts 58 with the labels)
    g.set_worlds(np.zeros(700, np.int32))  # all zero again: the labelled kernel, the answers of the first call
    check_plain(T, g, pos[sel], R, None, ob, mixed_beams(16), MAX_RANGE, "labels back to 0")
    g.close()


def test_forty_uavs_share_buckets(mrs):
    """40 UAVs: 128 buckets for 27 probes, so two probed cells share a bucket all the time and its records are gathered twice"""
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(40)
    pos = rng.uniform(-4.0, 4.0, (40, 3)) + [0.0, 0.0, 10.0]
    worlds = (np.arange(40) % 3 == 0).astype(np.int32) * 9
    g = plain_swarm(mrs, pos)
    g.set_worlds(worlds)
    T.set_scan_beams(g, mixed_beams(64))
    for max_range in (1.5, 3.0, 12.0):
        want = check_plain(T, g, pos, None, worlds, np.zeros(0, OBSTACLE), mixed_beams(64), max_range, max_range)
    assert (want[1] == HIT_UAV).sum() > 100
    g.close()


def test_partial_ranges_strides_and_either_index_output(mrs, scene):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    T.set_scan_beams(g, mixed_beams(7))
    for first, count in ((0, 1), (1000, 517), (g.n - 37, 37)):
        check_scan(T, g, uav_ref(7, True, True), MAX_RANGE, True, True, torch.float64, first, count, label=(first, count))
        check_scan(T, g, uav_ref(7, False, False), MAX_RANGE, False, False, torch.float32, first, count, label=(first, count, "world"))
    T.set_scan_beams(g, mixed_beams(100))
    check_scan(T, g, uav_ref(100, True, True), MAX_RANGE, True, True, torch.float32, 2001, 333, label="100 beams, a range")
    check_scan(T, g, uav_ref(100, True, True), MAX_RANGE, True, True, torch.float64, 5, 200, label="uav without hit", hits=False)
    check_scan(T, g, uav_ref(100, True, True), MAX_RANGE, True, True, torch.float64, 5, 200, label="hit without uav", uavs=False)
    check_scan(T, g, uav_ref(100, True, True), MAX_RANGE, True, True, torch.float64, 5, 200, label="ranges alone", hits=False, uavs=False)
    # the defaults: new tensors, body frame, no ground, FP32, no index outputs
    T.set_scan_beams(g, mixed_beams(7))
    r, h, w = T.range_scan_uavs(g, MAX_RANGE)
    assert h is None and w is None and r.dtype == torch.float32 and r.shape == (g.n, 7)
    assert same_bits(r.cpu().numpy(), uav_ref(7, True, False)[0].astype(np.float32))
    r, h, w = T.range_scan_uavs(g, MAX_RANGE, ground=True, hits=True, uavs=True, dtype=torch.float64)
    res = uav_ref(7, True, True)
    assert same_bits(r.cpu().numpy(), res[0]) and np.array_equal(h.cpu().numpy(), res[1]) and np.array_equal(w.cpu().numpy(), res[2])


def test_agrees_with_the_old_call_where_no_uav_is_near(mrs):
    """every other UAV at least max_range + 1 away on some axis: the range scan's bits and hit values, and uav all -1"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    k = np.arange(343)
    grid = np.stack([k % 7, (k // 7) % 7, k // 49], axis=1) * 8.0 + [-24.0, -24.0, 0.0] + np.random.default_rng(3).uniform(-0.2, 0.2, (343, 3))
    g = plain_swarm(mrs, grid)
    g.set_obstacles(ob)
    T.set_scan_beams(g, mixed_beams(16))
    assert len(candidate_pairs(grid, None, X500, MAX_RANGE + 1.0)[0]) == 0
    for ground in (False, True):
        r, h, w = T.range_scan_uavs(g, MAX_RANGE, ground=ground, hits=True, uavs=True, dtype=torch.float64)
        r0, h0 = T.range_scan(g, MAX_RANGE, ground=ground, hits=True, dtype=torch.float64)
        assert torch.equal(r.view(torch.int64), r0.view(torch.int64)) and torch.equal(h, h0) and (w == -1).all()
        assert (h0 >= 0).sum() > 100
    g.close()


def test_moved_uavs_are_seen_where_they_are(mrs):
    from mrs_multirotor_simulator_amd import tensors as T
    rng = np.random.default_rng(12)
    pos = rng.uniform(-8.0, 8.0, (300, 3)) + [0.0, 0.0, 12.0]
    g = plain_swarm(mrs, pos)
    T.set_scan_beams(g, mixed_beams(16))
    none = np.zeros(0, OBSTACLE)
    a = check_plain(T, g, pos, None, None, none, mixed_beams(16), 5.0, "before")
    moved = pos.copy()
    moved[::2] += rng.uniform(-3.0, 3.0, (150, 3))
    g.set_state(0, 300, moved, None, None, None, None)
    b = check_plain(T, g, moved, None, None, none, mixed_beams(16), 5.0, "after set_state")
    assert (a[2] != b[2]).sum() > 100


@pytest.mark.parametrize("arith,crash", [("LITERAL", False), ("FAST", True)])
def test_inside_a_horizon(mrs, arith, crash):
    """rollout_tick_cost over 48 ticks: one swarm runs them cut into 24 + 24 with accumulate and scans at the cut and after the end; its
    twin runs the uncut horizon in one call and nothing else: final state, crash flags and cost vectors are the twin's bit for bit (the
    pending collision tick stays pending), and the scans are the restatement's of the positions and attitudes at that point"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ar = getattr(mrs, "ARITH_" + arith)
    a, b = pair_swarm(mrs, ar), pair_swarm(mrs, ar)
    pos, _ = pair_state()
    rng = np.random.default_rng(31)
    dev = torch_dev(a)
    ticks, hold = 24, 4
    groups = T.OBS_POS | T.OBS_VEL
    blocks = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (2 * ticks // hold, N_PAIR, 4))
    cmd = torch.tensor(blocks, device=dev)
    tg, wt = make_targets(rng, 2 * ticks // hold, N_PAIR, T.gather_width(groups), torch.float64, dev, False, False)
    costs = {id(a): torch.zeros(N_PAIR, dtype=torch.float64, device=dev), id(b): torch.zeros(N_PAIR, dtype=torch.float64, device=dev)}
    half = ticks // hold
    beams = np.concatenate([T.scan_ring(8), [[0.0, 0.0, -1.0]]])
    T.set_scan_beams(a, beams)
    hits = 0
    for piece in range(2):
        sl = slice(piece * half, (piece + 1) * half)
        T.rollout_tick_cost(a, O.POSITION_CMD, cmd[sl], DT, crash, REBOUNCE, groups, tg[sl], wt[sl], 1000.0, hold=hold, out=costs[id(a)],
                            accumulate=True)
        obs = T.gather(a, T.OBS_POS | T.OBS_ROT, dtype=torch.float64).cpu().numpy()
        want = check_plain(T, a, obs[:, :3], obs[:, 3:12].reshape(-1, 3, 3), None, np.zeros(0, OBSTACLE), beams, 12.0, piece, ground_z=np.zeros(N_PAIR))
        hits += int((want[1] == HIT_UAV).sum())
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


def test_alternating_with_nearest_and_proximity_cost(mrs, scene):
    """the three calls share the swarm's hash scratch, each building it for its own radius: every result is what it was alone"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    T.set_scan_beams(g, mixed_beams(16))
    res = uav_ref(16, True, True)

    def three():
        rows, index, counts = T.nearest(g, 8, 4.0, T.NN_REL_POS | T.NN_DIST, dtype=torch.float64)
        cost, found = T.proximity_cost(g, 2.5, found=True)
        scan = T.range_scan_uavs(g, MAX_RANGE, ground=True, hits=True, uavs=True, dtype=torch.float64)
        return [t.clone() for t in (rows, index, counts, cost, found) + scan]

    first = three()
    assert same_bits(first[5].cpu().numpy(), res[0]) and np.array_equal(first[6].cpu().numpy(), res[1]) and np.array_equal(first[7].cpu().numpy(), res[2])
    for rep in range(2):
        T.range_scan_uavs(g, 2.0 + rep)  # (another edge in between)
        again = three()
        for k, (x, y) in enumerate(zip(first, again)):
            assert x.dtype == y.dtype and torch.equal(torch.nan_to_num(x.double(), nan=7.0), torch.nan_to_num(y.double(), nan=7.0)), (rep, k)


def test_queries_and_scans_interleaved_on_two_cache_entries(mrs):
    """nearest_obstacles, range_scan, range_scan_uavs and obstacle_cost interleaved on one swarm (600 UAVs of the fixture scene, 16 beams):
    every result is its restatement's bit for bit, and the grid builds are those of two independent cache entries — the two scan calls
    share the scans' entry, the two queries the queries'"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    from test_obstacles import HINGE2, ON_DIST, ON_REL, add_bits, restate_cost, restate_obstacles, restate_rows
    pos, worlds, ob = fixture_scene()
    n, k, r1, r2, r3 = 600, 8, 3.0, MAX_RANGE, 2.5
    pos, worlds = pos[:n], worlds[:n]
    R = scene_state()["R"].reshape(-1, 3, 3)[:n]
    beams, gz = mixed_beams(16), np.zeros(n)
    g = plain_swarm(mrs, pos, R)
    g.set_worlds(worlds)
    g.set_obstacles(ob)
    T.set_scan_beams(g, beams)
    near = restate_obstacles(pos, R, worlds, ob, k, r1)
    rows_want = restate_rows(near, ON_REL | ON_DIST)
    cost_want = add_bits(None, restate_cost(near, k, r1, HINGE2, 1.5))
    scan_want = {r: restate_scan(pos, R, worlds, ob, beams, r, ground_z=gz) for r in (r2, r3)}
    uavs_want = {r: restate_scan_uavs(pos, R, worlds, X500, ob, beams, r, ground_z=gz) for r in (r2, r3)}
    assert (near["found"] > 0).sum() > 100 and (scan_want[r3][1] >= 0).sum() > 100 and (uavs_want[r3][1] == HIT_UAV).sum() >= 10

    def nearest():
        rows, index, counts = T.nearest_obstacles(g, k, r1, ON_REL | ON_DIST, dtype=torch.float64)
        assert same_bits(rows.cpu().numpy(), rows_want) and np.array_equal(index.cpu().numpy(), near["index"])
        assert np.array_equal(counts.cpu().numpy(), near["count"])

    def scan(r):
        ranges, hit = T.range_scan(g, r, ground=True, hits=True, dtype=torch.float64)
        assert same_bits(ranges.cpu().numpy(), scan_want[r][0]) and np.array_equal(hit.cpu().numpy(), scan_want[r][1]), r

    def scan_uavs(r):
        ranges, hit, uav = T.range_scan_uavs(g, r, ground=True, hits=True, uavs=True, dtype=torch.float64)
        assert same_bits(ranges.cpu().numpy(), uavs_want[r][0]) and np.array_equal(hit.cpu().numpy(), uavs_want[r][1]), r
        assert np.array_equal(uav.cpu().numpy(), uavs_want[r][2]), r

    def cost():
        c, found = T.obstacle_cost(g, r1, k, HINGE2, 1.5, found=True)
        assert same_bits(c.cpu().numpy(), cost_want) and np.array_equal(found.cpu().numpy(), near["found"])

    def builds():
        return g.obstacle_stats()["grid_builds"]

    assert builds() == 0
    for call, want in ((nearest, 1), (lambda: scan(r2), 2), (lambda: scan_uavs(r2), 2), (cost, 2), (lambda: scan_uavs(r3), 3), (lambda: scan(r3), 3)):
        call()
        assert builds() == want, want
    for call in (nearest, lambda: scan(r3), lambda: scan_uavs(r3), cost, lambda: scan_uavs(r3), lambda: scan(r3)):  # r1 and r3 only: no build
        call()
        assert builds() == 3
    assert g.obstacle_stats()["grid_radius"] == r1  # (the stats describe the queries' entry)
    g.set_obstacles(ob)  # the same set again: both entries are dropped
    assert builds() == 3 and g.obstacle_stats()["cells"] == 0
    cost()
    assert builds() == 4
    scan_uavs(r3)
    assert builds() == 5
    scan(r3)
    nearest()
    assert builds() == 5
    g.close()


def test_clones(mrs):
    from mrs_multirotor_simulator_amd import tensors as T
    pos, worlds, ob = fixture_scene()
    sel = slice(0, 600)
    R = scene_state()["R"].reshape(-1, 3, 3)[sel]
    g = plain_swarm(mrs, pos[sel], R)
    g.set_worlds(worlds[sel])
    g.set_obstacles(ob)
    T.set_scan_beams(g, mixed_beams(16))
    check_plain(T, g, pos[sel], R, worlds[sel], ob, mixed_beams(16), MAX_RANGE, "original")
    c, big = g.clone(), g.clone_resized(700)
    check_plain(T, c, pos[sel], R, worlds[sel], ob, mixed_beams(16), MAX_RANGE, "clone")
    sb = big.get_states()
    check_plain(T, big, sb["x"], sb["R"].reshape(-1, 3, 3), np.concatenate([worlds[sel], np.zeros(100, np.int32)]), ob, mixed_beams(16), MAX_RANGE,
                "resized clone")
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
    uav = torch.full((300, 16), -9, dtype=torch.int32, device=dev)
    r, h, u = ranges.data_ptr(), hit.data_ptr(), uav.data_ptr()
    with pytest.raises(mrs.MrsError, match="error 1:.*no beam pattern"):
        g.range_scan_uavs_device(0, 300, 5.0, 0, r, 0, 16, h, 16, u, 16, st)
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
        ((200, 101, 5.0, 3, r, 0, 16, h, 16, u, 16), "error 3:"),
        ((-1, 10, 5.0, 3, r, 0, 16, h, 16, u, 16), "error 3:"),
        ((0, 300, 0.0, 3, r, 0, 16, h, 16, u, 16), "error 1:.*max_range must be finite and > 0"),
        ((0, 300, -2.0, 3, r, 0, 16, h, 16, u, 16), "error 1:.*max_range"),
        ((0, 300, nan, 3, r, 0, 16, h, 16, u, 16), "error 1:.*max_range"),
        ((0, 300, inf, 3, r, 0, 16, h, 16, u, 16), "error 1:.*max_range"),
        ((0, 300, 5.0, 4, r, 0, 16, h, 16, u, 16), "error 1:.*unknown scan flag bits"),
        ((0, 300, 5.0, 0x80000001, r, 0, 16, h, 16, u, 16), "error 1:.*unknown scan flag bits"),
        ((0, 300, 5.0, 3, r, 7, 16, h, 16, u, 16), "error 1:.*dtype"),
        ((0, 300, 5.0, 3, r, 0, 15, h, 16, u, 16), "error 1:.*stride smaller than n_beams"),
        ((0, 300, 5.0, 3, r, 0, 16, h, 15, u, 16), "error 1:.*hit_stride smaller than n_beams"),
        ((0, 300, 5.0, 3, r, 0, 16, h, 16, u, 15), "error 1:.*uav_stride smaller than n_beams"),
        ((0, 300, 5.0, 3, r, 0, 16, 0, 0, u, 15), "error 1:.*uav_stride smaller than n_beams"),
        ((0, 300, 5.0, 3, 0, 0, 16, h, 16, u, 16), "error 1:.*dev_ranges: null pointer"),
        ((0, 0, 5.0, 3, 0, 0, 16, h, 16, u, 16), "error 1:.*dev_ranges: null pointer"),
        ((0, 300, 5.0, 3, host.ctypes.data, 0, 16, h, 16, u, 16), "error 1:.*dev_ranges"),
        ((0, 300, 5.0, 3, r, 0, 16, host.ctypes.data, 16, u, 16), "error 1:.*dev_hit"),
        ((0, 300, 5.0, 3, r, 0, 16, h, 16, host.ctypes.data, 16), "error 1:.*dev_uav"),
        ((0, 300, 5.0, 3, small, 0, 16, h, 16, u, 16), "error 1:.*dev_ranges: the rows extend past"),
        ((0, 300, 5.0, 3, r, 0, 16, small, 16, u, 16), "error 1:.*dev_hit: the rows extend past"),
        ((0, 300, 5.0, 3, r, 0, 16, h, 16, small, 16), "error 1:.*dev_uav: the rows extend past"),
    ]
    torch.cuda.synchronize(dev)
    for args, msg in bad:
        with pytest.raises(mrs.MrsError, match=msg):
            g.range_scan_uavs_device(*args, st)
    torch.cuda.synchronize(dev)
    assert hip.hipFree(C.c_void_p(small)) == 0

    def untouched():
        return (ranges.cpu().numpy() == SENTINEL).all() and (hit.cpu().numpy() == -7).all() and (uav.cpu().numpy() == -9).all()

    assert untouched() and g.obstacle_stats()["grid_builds"] == 0  # nothing was launched, no grid was built
    g.range_scan_uavs_device(0, 0, 5.0, 3, r, 0, 16, h, 16, u, 16, st)  # count == 0 is MRS_OK and writes nothing
    g.range_scan_uavs_device(300, 0, 5.0, 3, r, 0, 16, 0, 0, 0, 0, st)
    assert untouched() and g.obstacle_stats()["grid_builds"] == 0
    after = g.get_states()
    for key in before.dtype.names:
        assert before[key].tobytes() == after[key].tobytes(), key
    # the old call keeps refusing what it refused
    with pytest.raises(mrs.MrsError, match="error 1:.*unknown scan flag bits"):
        g.range_scan_device(0, 300, 5.0, 4, r, 0, 16, h, 16, st)
    # a sharded swarm
    group = mrs.LoopbackGroup(2)
    shards = []
    for rk in range(2):
        s = mrs.Swarm(100)
        s.construct(0, 100, mrs.model_params("x500"), np.stack([np.arange(100) * 3.0 + 400 * rk, np.zeros(100), np.full(100, 5.0)], axis=1))
        s.comm_init_loopback(group, rk, 200)
        s.set_scan_beams(mixed_beams(16))
        shards.append(s)
    for s in shards:
        with pytest.raises(mrs.MrsError, match="error 1:.*mrs_swarm_range_scan_uavs_device: not on a sharded swarm"):
            T.range_scan_uavs(s, 5.0, out=ranges[:100])
    assert untouched()
    for s in shards:
        s.close()
    group.close()
    g.close()


def test_caller_stream_is_fenced(mrs, scene):
    """the outputs are filled on a side stream kept busy by a long sleep, then the scan is made with that stream current: the rows must
    hold the result (the kernels ran after the fill), and copies queued behind the call on the side stream read it"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = scene
    dev = torch_dev(g)
    T.set_scan_beams(g, mixed_beams(16))
    res = uav_ref(16, True, True)
    ranges = torch.zeros((g.n, 16), dtype=torch.float64, device=dev)
    hit = torch.zeros((g.n, 16), dtype=torch.int32, device=dev)
    uav = torch.zeros((g.n, 16), dtype=torch.int32, device=dev)
    T.range_scan_uavs(g, MAX_RANGE, ground=True)  # (the grid is built and the scratch allocated: the fenced call only launches)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        ranges.fill_(SENTINEL)
        hit.fill_(-7)
        uav.fill_(-9)
        T.range_scan_uavs(g, MAX_RANGE, ground=True, out=ranges, hits=hit, uavs=uav)
        rcopy, hcopy, ucopy = ranges.clone(), hit.clone(), uav.clone()
    side.synchronize()
    assert same_bits(rcopy.cpu().numpy(), res[0]) and np.array_equal(hcopy.cpu().numpy(), res[1]) and np.array_equal(ucopy.cpu().numpy(), res[2])


def test_cpp_facade_equals_python(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, m, nb = 2000, 60, 10
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "scan.bin")
        out = subprocess.run([build_cpp("range_scan_uavs_test"), path], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok range_scan_uavs_equals_brute_force", "ok written"):
            assert tag in out.stdout, out.stdout
        raw = open(path, "rb").read()
    cr = np.frombuffer(raw, np.float64, n * nb, 0).reshape(n, nb)
    ch = np.frombuffer(raw, np.int32, n * nb, 8 * n * nb).reshape(n, nb)
    cu = np.frombuffer(raw, np.int32, n * nb, 12 * n * nb).reshape(n, nb)
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
    r, h, w = T.range_scan_uavs(g, 9.0, ground=True, hits=True, uavs=True, dtype=torch.float64)
    assert same_bits(r.cpu().numpy(), cr) and np.array_equal(h.cpu().numpy(), ch) and np.array_equal(w.cpu().numpy(), cu)
    assert (ch >= 0).any() and (ch == HIT_UAV).any() and (ch == HIT_GROUND).any() and (ch == HIT_NONE).any()
    g.close()
