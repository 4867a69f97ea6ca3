"""Collision worlds on the GPU (include/mrs_swarm.h, "collision worlds"): a swarm whose UAVs carry W distinct labels behaves, world by
world, as W separate swarms that hold the UAVs of one label in ascending index order and receive the same calls.

Scenarios: tests/collision_worlds.py — worlds stacked on the same coordinates (contiguous and interleaved labels), 40 pairs on one
spot, the hit-list clusters twice, a dense box of six worlds.  Checked: one collision pass against the oracle run per world; the
neighbour lists against the per-world restatement under every lanes-per-UAV instantiation; every path (no lists, no fused launches)
against the default's bits; 200 ticks against three separate swarms bit for bit; the fork -> set_worlds -> tick-rollout recipe against
separate swarms loaded from the same records; nearest-neighbour rows per world; and the bookkeeping of the labels."""
import os
import subprocess

import numpy as np
import pytest

import collision_thresholds as ct
import collision_worlds as cw
import helpers
from helpers import RTOL_FAST, RTOL_LITERAL
from collision_threshold_swarms import DT, REBOUNCE, oracle_swarm, product
from test_collision_thresholds_gpu import check_result, differing
from test_device_io_gpu import build_cpp, torch_dev
from test_nearest import nearest_ref, nearest_rows

pytestmark = pytest.mark.gpu
ARITH = pytest.mark.parametrize("fast", [False, True], ids=["literal", "fast"])
CRASH = pytest.mark.parametrize("crash", [False, True], ids=["elastic", "crash"])
SCENES = {"stacked": lambda: cw.stacked(False), "interleaved": lambda: cw.stacked(True), "clusters": lambda: cw.clusters()[:3],
          "many pairs": cw.many_pairs, "wide": cw.wide, "stacked x500": lambda: cw.stacked(False, mixed=False),
          "interleaved x500": lambda: cw.stacked(True, mixed=False)}
_refs = {}


def labelled(M, O, pos, af, world, fast, state=None):
    g = product(M, O, pos, af, fast)
    if state is not None:
        g.set_state(0, len(pos), *state)
    g.set_worlds(world)
    return g


def references(O, name, crash):
    """restatement and oracle of one pass, the oracle run once per world on that world's UAVs alone"""
    if (name, crash) not in _refs:
        pos, world, af = SCENES[name]()
        arm, prop, mass = ct.constants(af)
        want = cw.restatement(pos, world, arm, prop, mass, crash, REBOUNCE)
        want["oracle_crashed"], want["oracle_force"] = np.zeros(len(pos), dtype=np.int32), np.zeros((len(pos), 3))
        for _, idx in cw.split(world):
            o = oracle_swarm(O, pos[idx], af[idx])
            o.handle_collisions(True, crash, REBOUNCE)
            want["oracle_crashed"][idx], want["oracle_force"][idx] = o.has_crashed(), o.get_external_force()
        want["pushed"] = np.abs(want["force"]).sum(axis=1) > 0
        assert np.array_equal(want["oracle_crashed"], want["crashed"])
        helpers.assert_close(want["oracle_force"], want["force"], 1e-14, f"{name}: oracle vs restatement")
        _refs[(name, crash)] = want
    return _refs[(name, crash)]


# ---- 1: one pass ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stacked", "interleaved", "clusters"])
@ARITH
@CRASH
def test_one_pass_search_tick_and_list_tick(mrs, oracle, name, fast, crash):
    """mixed airframes; world 1 coincides with world 0 (clusters: both worlds coincide), and no force is NaN"""
    pos, world, af = SCENES[name]()
    want = references(oracle, name, crash)
    g = labelled(mrs, oracle, pos, af, world, fast)
    g.handle_collisions(True, crash, REBOUNCE)
    force = g.get_external_force()
    assert np.isfinite(force).all(), "coincident UAVs of two worlds met"
    check_result(g.has_crashed(), force, want, crash, fast, f"{name}: search tick")
    assert g.collision_stats() == (1, 1)
    g = labelled(mrs, oracle, pos, af, world, fast)
    g.handle_collisions(True, False, 37.0)
    g.handle_collisions(True, crash, REBOUNCE)
    force = g.get_external_force()
    assert np.isfinite(force).all()
    check_result(g.has_crashed(), force, want, crash, fast, f"{name}: list tick")
    assert g.collision_stats() == (2, 1), "the second call repeated the search"


# ---- 2: lists -------------------------------------------------------------------------------------------------------------------------
def read_lists(g):
    count, nbr, cap, radius = g.debug_neighbour_lists()
    assert cap == cw.LIST_CAP and radius * radius * (1.0 + 1e-9) + 1e-5 == ct.LIST_R2
    return [nbr[:count[i], i].astype(np.int64).tolist() for i in range(g.n)]


@pytest.mark.parametrize("lanes", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["stacked", "interleaved", "many pairs", "wide"])
@ARITH
def test_lists_hold_same_world_partners_only(mrs, oracle, monkeypatch, name, lanes, fast):
    monkeypatch.setenv("MRS_QUERY_LPU", str(lanes))
    pos, world, af = SCENES[name]()
    want = cw.list_sets(pos, world)
    got = read_lists(labelled(mrs, oracle, pos, af, world, fast))
    bad = [(i, got[i], want[i].tolist()) for i in range(len(pos)) if got[i] != want[i].tolist()]
    assert not bad, f"{name}, {lanes} lane(s): {len(bad)} of {len(pos)} lists differ, first: {bad[:4]}"
    if name == "many pairs":
        assert all(got[i] == [i ^ 1] for i in range(len(pos)))


@ARITH
@CRASH
def test_the_filter_is_in_the_list_building(mrs, oracle, fast, crash):
    """40 pairs on one spot: with labels every list is one partner and the second tick is a list tick; with every label 0 on the same
    positions every UAV has 79 neighbours, no list fits, and every tick searches"""
    pos, world, af = cw.many_pairs()
    g = labelled(mrs, oracle, pos, af, world, fast)
    g.handle_collisions(True, crash, REBOUNCE)
    g.handle_collisions(True, crash, REBOUNCE)
    assert g.collision_stats() == (2, 1)
    assert not g.has_crashed().any() and not np.any(g.get_external_force()), "pairs 1 m apart do not touch"
    g = labelled(mrs, oracle, pos, af, np.zeros(len(pos), dtype=np.int32), fast)
    g.handle_collisions(True, crash, REBOUNCE)
    g.handle_collisions(True, crash, REBOUNCE)
    g.handle_collisions(True, crash, REBOUNCE)
    assert g.collision_stats() == (3, 3)


# ---- moving scenes --------------------------------------------------------------------------------------------------------------------
def closing_state(pos, world, speed=3.0):
    """every UAV flies towards the centre of its world's scene (the same velocities for the same positions), level, motors off"""
    n = len(pos)
    v = np.zeros((n, 3))
    for _, idx in cw.split(world):
        d = pos[idx].mean(axis=0) - pos[idx]
        v[idx] = speed * d / np.maximum(np.linalg.norm(d, axis=1), 0.3)[:, None]
    return pos, v, np.tile(np.eye(3).reshape(9), (n, 1)), np.zeros((n, 3)), np.zeros((n, 8))


def snapshot(g):
    st = g.get_state()
    return dict(st, force=g.get_external_force(), crashed=g.has_crashed())


def assert_same_bits(a, b, what, keys=("x", "v", "R", "omega", "motor_rpm", "force", "crashed")):
    for k in keys:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs at UAVs {differing(np.asarray(a[k]).reshape(len(a[k]), -1).tolist(), np.asarray(b[k]).reshape(len(b[k]), -1).tolist())}"


# ---- 3: every path --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stacked", "clusters"])
@ARITH
@CRASH
def test_every_path_gives_the_default_paths_bits(mrs, oracle, monkeypatch, name, fast, crash):
    """30 ticks with UAVs closing in: search every tick (no lists), every tick on its own (no fused launches) and fused launches named
    explicitly all equal the default: bit for bit in LITERAL; in FAST the crash flags exactly and state and force within RTOL_FAST (the
    paths evaluate a tick in different units, collide.hip built without contraction and the FAST step unit with it; on the MI355X one
    UAV's x and v come out 5e-17 relative apart under MRS_NEIGHBOUR_LISTS=0, everything else the same bits)"""
    pos, world, af = SCENES[name]()
    state = closing_state(pos, world)

    def run():
        g = labelled(mrs, oracle, pos, af, world, fast, state)
        g.tick_n(DT, 30, True, crash, REBOUNCE)
        return snapshot(g)

    default = run()
    touched = default["crashed"].any() if crash else np.any(default["force"])
    assert touched and np.isfinite(default["x"]).all()
    for var, val in (("MRS_NEIGHBOUR_LISTS", "0"), ("MRS_FUSED_COLLISIONS", "0"), ("MRS_FUSED_COLLISIONS", "1")):
        with monkeypatch.context() as m:
            m.setenv(var, val)
            got = run()
            print(f"{name} fast={fast} crash={crash} {var}={val}: " + ", ".join(f"{k} {'same bits' if np.array_equal(got[k], default[k]) else 'rel %.3e' % helpers.rel_linf(got[k], default[k])}" for k in ("x", "v", "R", "omega", "motor_rpm", "force")))
            if not fast:
                assert_same_bits(got, default, f"{name}: {var}={val}")
                continue
            assert np.array_equal(got["crashed"], default["crashed"]), f"{name}: {var}={val}: crash flags"
            for k in ("x", "v", "R", "omega", "motor_rpm", "force"):
                helpers.assert_close(got[k], default[k], RTOL_FAST, f"{name}: {var}={val}: {k}")


# ---- 4: W swarms in one ---------------------------------------------------------------------------------------------------------------
TICKS = 200


def oracle_horizon(O, pos, af, state, crash):
    """the oracle through the horizon on one world's UAVs: final state and crash flags, whether a contact and a list rebuild happen
    inside it, and how close any pair distance comes to a threshold (d2 against 3.0 and against crit, per tick)"""
    o = oracle_swarm(O, pos, af)
    o.set_state(0, len(pos), *state)
    arm, prop, _ = ct.constants(af)
    crit = ((arm[:, None] + prop[:, None]) + arm[None, :]) + prop[None, :]
    off = ~np.eye(len(pos), dtype=bool)
    margin, contact, x0, moved = np.inf, False, pos.copy(), 0.0
    for _ in range(TICKS):
        o.step(DT)
        x = o.get_state()["x"]
        d2 = ct.d2_written(x[:, None, :], x[None, :, :])
        margin = min(margin, np.abs(d2 - 3.0)[off].min(), np.abs(d2 - crit)[off].min())
        contact = contact or bool(np.any((d2 < crit) & (d2 < 3.0) & off))
        moved = max(moved, np.linalg.norm(x - x0, axis=1).max())
        o.handle_collisions(True, crash, REBOUNCE)
    return o.get_state(), o.has_crashed(), contact, moved, margin


@pytest.mark.parametrize("name", ["stacked x500", "interleaved x500"])
@ARITH
@CRASH
def test_worlds_equal_separate_swarms_over_200_ticks(mrs, oracle, name, fast, crash):
    pos, world, af = SCENES[name]()
    state = closing_state(pos, world, speed=3.25)  # (at 3.0 and 2.75 m/s a pair passes within 1e-6 of a threshold)
    parts = cw.split(world)
    g = labelled(mrs, oracle, pos, af, world, fast, state)
    g.tick_n(DT, TICKS, True, crash, REBOUNCE)
    got = snapshot(g)
    assert g.collision_stats()[1] >= 2, "no list rebuild inside the horizon"
    keys = ("x", "v", "R", "omega", "motor_rpm", "force", "crashed")
    for w, idx in parts:
        sub = tuple(a[idx] for a in state)
        so, co, contact, moved, margin = oracle_horizon(oracle, pos[idx], af[idx], sub, crash)
        assert contact and moved > 0.25 and margin > 1e-6, f"world {w}: contact {contact}, moved {moved:.3f} m, threshold margin {margin:.3e}"
        s = product(mrs, oracle, pos[idx], af[idx], fast)
        s.set_state(0, len(idx), *sub)
        s.tick_n(DT, TICKS, True, crash, REBOUNCE)
        alone = snapshot(s)
        mine = {k: got[k][idx] for k in keys}
        # FAST too comes out bit for bit on the MI355X (the same kernels on the same lists), so that is what both flavours assert
        assert_same_bits(mine, alone, f"world {w} vs the separate swarm")
        assert np.array_equal(mine["crashed"], co), f"world {w}: crash flags vs the oracle"
        for k in ("x", "v"):  # (level UAVs with their motors off: R stays I and omega 0 up to rounding residues, which have no scale to be relative to)
            helpers.assert_close(mine[k], so[k], RTOL_FAST if fast else RTOL_LITERAL, f"world {w}: {k} vs the oracle")
        assert np.abs(mine["omega"] - so["omega"]).max() < 1e-12 and np.abs(mine["R"] - so["R"]).max() < 1e-12


# ---- 5: fork, then plan ---------------------------------------------------------------------------------------------------------------
@ARITH
@CRASH
def test_fork_set_worlds_tick_rollouts(mrs, oracle, fast, crash):
    """M = 40 agents, S = 8 samples: the 40-UAV scene saved, loaded into 320 UAVs (index i % 40), world i // 40, a command row per
    sample.  The costs, crash rows and closed-loop states of sample s equal those of a separate 40-UAV swarm loaded from the same
    records and given sample s's rows — bit for bit in LITERAL, within RTOL_FAST in FAST (crash rows exactly)."""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    M, S, B, hold = 40, 8, 6, 10
    rng = np.random.default_rng(31)
    pos = rng.uniform(-2.5, 2.5, (M, 3)) + [0.0, 0.0, 20.0]
    af = np.array(["x500"] * M, dtype=object)
    base = product(mrs, oracle, pos, af, fast)
    base.set_state(0, M, *closing_state(pos, np.zeros(M, dtype=np.int32), speed=2.0))
    dev = torch_dev(base)
    rec = T.save(base)
    big = product(mrs, oracle, np.tile(pos, (S, 1)) + [100.0, 0.0, 0.0], np.tile(af, S), fast)
    T.load(big, rec, index=(torch.arange(S * M, dtype=torch.int32, device=dev) % M))
    T.set_worlds(big, (torch.arange(S * M, dtype=torch.int32, device=dev) // M))
    assert np.array_equal(big.get_worlds(), np.arange(S * M) // M) and np.array_equal(big.get_state()["x"], np.tile(pos, (S, 1)))
    goals = np.concatenate([pos[None, None] + rng.uniform(-1.5, 1.5, (B, S, 1, 3)), np.zeros((B, S, M, 1))], axis=3)  # [B, S, M, 4]
    t64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    cmd = t64(goals.reshape(B, S * M, 4))
    tgt = t64(np.broadcast_to(goals[..., :3], (B, S, M, 3)).reshape(B, S * M, 3))
    wts = t64([[1.0, 1.0, 2.0]])
    gain = t64(rng.uniform(0.0, 0.3, (1, 4, 3, S * M)))
    gain[:, 3] = 0.0
    smalls = []
    for s in range(S):
        g = product(mrs, oracle, pos + [-100.0, 0.0, 0.0], af, fast)
        T.load(g, rec)
        smalls.append(g)
    cut = lambda t, s: t[:, s * M:(s + 1) * M].contiguous()

    def same(a, b, what):
        a, b = np.asarray(a), np.asarray(b)
        if fast and a.dtype.kind == "f":
            helpers.assert_close(a, b, RTOL_FAST, what)
        else:
            assert np.array_equal(a, b), f"{what}: differs at {differing(a.reshape(len(a), -1).tolist(), b.reshape(len(b), -1).tolist())}"

    cost = T.rollout_tick_cost(big, oracle.POSITION_CMD, cmd, DT, crash, REBOUNCE, T.OBS_POS, tgt, wts, crash_cost=5.0, hold=hold, cost_every=10).cpu().numpy()
    assert np.isfinite(cost).all() and len({cost[s * M:(s + 1) * M].tobytes() for s in range(S)}) == S, "the samples do not differ"
    for s, g in enumerate(smalls):
        c = T.rollout_tick_cost(g, oracle.POSITION_CMD, cut(cmd, s), DT, crash, REBOUNCE, T.OBS_POS, cut(tgt, s), wts, crash_cost=5.0, hold=hold, cost_every=10)
        same(cost[s * M:(s + 1) * M], c.cpu().numpy(), f"sample {s}: costs")
    rows, crows = T.rollout_ticks(big, oracle.POSITION_CMD, cmd, DT, crash, REBOUNCE, T.OBS_POS, hold=hold)
    rows, crows = rows.cpu().numpy(), crows.cpu().numpy()
    for s, g in enumerate(smalls):
        r, c = T.rollout_ticks(g, oracle.POSITION_CMD, cut(cmd, s), DT, crash, REBOUNCE, T.OBS_POS, hold=hold)
        assert np.array_equal(crows[:, s * M:(s + 1) * M], c.cpu().numpy()), f"sample {s}: crash rows"
        same(rows[:, s * M:(s + 1) * M].reshape(-1, 3), r.cpu().numpy().reshape(-1, 3), f"sample {s}: position rows")
    refs = tgt[:1].contiguous()
    T.rollout_tick_feedback(big, oracle.POSITION_CMD, cmd, DT, crash, REBOUNCE, T.OBS_POS, gain, refs, hold=hold)
    st, cr = big.get_state(), big.has_crashed()
    for s, g in enumerate(smalls):
        T.rollout_tick_feedback(g, oracle.POSITION_CMD, cut(cmd, s), DT, crash, REBOUNCE, T.OBS_POS, gain[..., s * M:(s + 1) * M].contiguous(), cut(refs, s), hold=hold)
        assert np.array_equal(cr[s * M:(s + 1) * M], g.has_crashed()), f"sample {s}: crash flags after the closed loop"
        for k in ("x", "v", "omega"):
            same(st[k][s * M:(s + 1) * M], g.get_state()[k], f"sample {s}: {k} after the closed loop")
    if crash:
        assert cr.any() and not cr.all()
    assert big.fused_stats()[0] > 0


# ---- 6: nearest -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stacked", "interleaved", "wide"])
@pytest.mark.parametrize("k", [4, 32])
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_nearest_rows_per_world(mrs, oracle, name, k, f32):
    """radius 4 m (cells of 4 m: the 6-m and 8-m boxes span several), whole swarm and a sub-range, sorted and index order"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, world, af = SCENES[name]()
    n, radius, fields = len(pos), 4.0, T.NN_REL_POS | T.NN_REL_VEL | T.NN_DIST
    rng = np.random.default_rng(3)
    v = rng.normal(0, 1, (n, 3))
    g = labelled(mrs, oracle, pos, af, world, False, (pos, v, np.tile(np.eye(3).reshape(9), (n, 1)), np.zeros((n, 3)), np.zeros((n, 8))))
    idx, cnt, dd = np.full((n, k), -1, np.int64), np.zeros(n, np.int64), np.zeros((n, k))
    for _, m in cw.split(world):
        i, c, d = nearest_ref(pos[m], 0, len(m), k, radius)
        idx[m], cnt[m], dd[m] = np.where(i >= 0, m[np.maximum(i, 0)], -1), c, d
    assert cnt.max() == min(k, 32) or k == 32
    for first, count in ((0, n), (37, 70)):
        want = nearest_rows(pos, v, np.tile(np.eye(3), (n, 1, 1)), first, idx[first:first + count], dd[first:first + count], fields)
        rows, gi, gc = T.nearest(g, k, radius, fields, first, count, dtype=torch.float32 if f32 else torch.float64)
        gi, gc = gi.cpu().numpy(), gc.cpu().numpy()
        assert np.array_equal(gi, idx[first:first + count]) and np.array_equal(gc, cnt[first:first + count]), f"{name} [{first}, +{count}): index / counts"
        assert np.array_equal(rows.cpu().numpy(), want.astype(np.float32) if f32 else want), f"{name} [{first}, +{count}): rows"
        listed = gi[gi >= 0]
        owner = np.repeat(np.arange(first, first + count), (gi >= 0).sum(axis=1))
        assert np.all(world[listed] == world[owner]) and not np.any(np.all(pos[listed] == pos[owner], axis=1)), "a UAV of another world is listed"


# ---- 7: bookkeeping -------------------------------------------------------------------------------------------------------------------
def test_round_trip_and_bad_arguments(mrs, oracle):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, world, af = cw.stacked(True)
    n = len(pos)
    g = product(mrs, oracle, pos, af, False)
    assert np.array_equal(g.get_worlds(), np.zeros(n, dtype=np.int32)) and g.get_worlds(10, 0).shape == (0,)
    g.set_worlds(world[20:90], first=20)
    want = np.zeros(n, dtype=np.int32)
    want[20:90] = world[20:90]
    assert np.array_equal(g.get_worlds(), want) and np.array_equal(g.get_worlds(19, 3), want[19:22])
    dev = torch_dev(g)
    T.set_worlds(g, torch.tensor(world[100:], dtype=torch.int32, device=dev), first=100)
    want[100:] = world[100:]
    assert np.array_equal(g.get_worlds(), want)
    g.set_worlds(np.zeros(0, dtype=np.int32), first=n)  # count == 0
    # refusals: error codes (1 = MRS_ERR_ARG, 3 = MRS_ERR_RANGE), nothing changed
    big = torch.zeros(5 * 1024 * 1024, dtype=torch.int32, device=dev)  # 20 MiB: an allocation of its own, whose end the runtime knows
    for call, code in ((lambda: g.set_worlds(world[:11], first=140), 3), (lambda: g.get_worlds(-1, 4), 3), (lambda: g.get_worlds(0, n + 1), 3),
                       (lambda: g.set_worlds_device(0, 4, 0, 0), 1), (lambda: g.set_worlds_device(140, 11, 1, 0), 3),
                       (lambda: g.set_worlds_device(0, 8, world.ctypes.data, 0), 1),
                       (lambda: g.set_worlds_device(0, 9, big.data_ptr() + 4 * (big.numel() - 8), 0), 1)):  # a row one label too short
        with pytest.raises(mrs.MrsError, match=f"error {code}:"):
            call()
    if torch.cuda.device_count() > 1:
        other = torch.zeros(8, dtype=torch.int32, device=torch.device("cuda", 1 - g.device()))
        with pytest.raises(mrs.MrsError, match="error 1:"):
            g.set_worlds_device(0, 8, other.data_ptr(), 0)
    assert np.array_equal(g.get_worlds(), want)


@CRASH
def test_a_setter_after_the_lists_are_built(mrs, oracle, crash):
    """lists built under one labelling; new labels; the next tick is a search and obeys them"""
    pos, world, af = cw.stacked(False)
    g = labelled(mrs, oracle, pos, af, world, False)
    g.handle_collisions(True, False, 37.0)
    g.handle_collisions(True, False, 37.0)
    assert g.collision_stats() == (2, 1)
    g.set_worlds(cw.stacked(True)[1])  # the interleaved labels on the contiguous positions: other neighbour sets
    arm, prop, mass = ct.constants(af)
    want = cw.restatement(pos, cw.stacked(True)[1], arm, prop, mass, crash, REBOUNCE)
    old = cw.restatement(pos, world, arm, prop, mass, crash, REBOUNCE)
    assert not np.array_equal(want["crashed"] if crash else want["force"], old["crashed"] if crash else old["force"])
    g.handle_collisions(True, crash, REBOUNCE)
    assert g.collision_stats() == (3, 2)
    if crash:
        assert np.array_equal(g.has_crashed(), want["crashed"])
    else:
        f = g.get_external_force()
        assert np.array_equal(np.abs(f).sum(axis=1) > 0, np.abs(want["force"]).sum(axis=1) > 0)
        helpers.assert_close(f, want["force"], 1e-12, "forces under the new labels")


def test_labels_belong_to_the_slot(mrs, oracle):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, world, af = cw.stacked(True, mixed=False)
    n = len(pos)
    g = labelled(mrs, oracle, pos, af, world, False)
    c, r = g.clone(), g.clone_resized(n + 70)
    assert np.array_equal(c.get_worlds(), world) and np.array_equal(r.get_worlds(), np.concatenate([world, np.zeros(70, dtype=np.int32)]))
    plain = product(mrs, oracle, pos, af, False)
    assert np.array_equal(plain.clone().get_worlds(), np.zeros(n, dtype=np.int32))
    c.set_worlds(np.full(n, 9, dtype=np.int32))
    assert np.array_equal(g.get_worlds(), world), "a clone shares its labels with the original"
    g.copy_uavs(0, c, 50, 40)
    assert np.array_equal(g.get_worlds(), world), "copy_uavs moved labels"
    dev = torch_dev(g)
    rec = T.save(c)
    T.load(g, rec)
    g.reset_device(0, n, torch.ones(n, dtype=torch.uint8, device=dev).data_ptr(), torch.tensor(pos, dtype=torch.float64, device=dev).data_ptr(), 0,
                   T.DTYPE_F64, False, 0)
    g.set_state_pos(0, n, pos)
    g.set_state(0, n, *closing_state(pos, world))
    assert np.array_equal(g.get_worlds(), world)
    # ... and still act: one pass gives the labelled result
    arm, prop, mass = ct.constants(af)
    g.handle_collisions(True, True, REBOUNCE)
    assert np.array_equal(g.has_crashed(), cw.restatement(pos, world, arm, prop, mass, True)["crashed"])


@ARITH
def test_all_labels_zero_is_no_labels(mrs, oracle, fast):
    """50 ticks: explicit zeros (the world-aware kernels) give the bits of a swarm on which no setter was called (the kernels without labels)"""
    pos, world, af = cw.wide()
    state = closing_state(pos, np.zeros(len(pos), dtype=np.int32), speed=2.0)
    out = []
    for zeros in (False, True):
        g = product(mrs, oracle, pos, af, fast)
        g.set_state(0, len(pos), *state)
        if zeros:
            g.set_worlds(world)
            g.set_worlds(np.zeros(len(pos), dtype=np.int32))
        g.tick_n(DT, 50, True, False, REBOUNCE)
        out.append(snapshot(g))
    assert np.any(out[0]["force"])
    assert_same_bits(out[1], out[0], "all labels 0")


def test_sharded_refusals(mrs, oracle):
    """a labelled swarm cannot join a communicator or take gathered records; a sharded swarm takes no labels, and its getter answers zeros"""
    pos = np.stack([np.arange(100) * 3.0, np.zeros(100), np.full(100, 5.0)], axis=1)
    group = mrs.LoopbackGroup(2)
    g = mrs.Swarm(100)
    g.construct(0, 100, mrs.model_params("x500"), pos)
    g.set_worlds(np.arange(100, dtype=np.int32) % 2)
    with pytest.raises(mrs.MrsError, match="error 1:.*world"):
        g.comm_init_loopback(group, 0, 200)
    ptr, nbytes = g.pack_positions()
    with pytest.raises(mrs.MrsError, match="error 1:.*world"):
        g.handle_collisions_gathered(ptr, 100, 0, True, False, 100.0)
    g.set_worlds(np.zeros(100, dtype=np.int32))  # all labels back to 0: an ordinary swarm again
    g.handle_collisions_gathered(ptr, 100, 0, True, False, 100.0)
    shards = [g, mrs.Swarm(100)]
    shards[1].construct(0, 100, mrs.model_params("x500"), pos + [400.0, 0.0, 0.0])
    for r, s in enumerate(shards):
        s.comm_init_loopback(group, r, 200)
    import torch
    dev_labels = torch.ones(100, dtype=torch.int32, device=torch_dev(g))
    for s in shards:
        for call in (lambda: s.set_worlds(np.ones(100, dtype=np.int32)), lambda: s.set_worlds_device(0, 100, dev_labels.data_ptr(), 0)):
            with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
                call()
        assert np.array_equal(s.get_worlds(), np.zeros(100, dtype=np.int32)) and np.array_equal(s.get_worlds(40, 7), np.zeros(7, dtype=np.int32))
    for s in shards:
        s.close()
    group.close()


def test_caller_stream_is_fenced(mrs, oracle):
    """the labels are written on a side stream kept busy by a long sleep, then handed over with that stream current: the pass that
    follows must see them"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, world, af = cw.stacked(False)
    g = product(mrs, oracle, pos, af, False)
    dev = torch_dev(g)
    labels = torch.zeros(len(pos), dtype=torch.int32, device=dev)
    src = torch.tensor(world, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        labels.copy_(src)
        T.set_worlds(g, labels)
        labels.fill_(0)  # queued behind the call: the library has taken its copy
    assert np.array_equal(g.get_worlds(), world)
    side.synchronize()
    arm, prop, mass = ct.constants(af)
    g.handle_collisions(True, True, REBOUNCE)
    assert np.array_equal(g.has_crashed(), cw.restatement(pos, world, arm, prop, mass, True)["crashed"])


def facade_scene():
    """(pos, world) of tests/cpp/worlds_test.cpp: the same expressions"""
    i = np.arange(150)
    w, k = i % 3, i // 3
    s = (w == 2).astype(np.float64)
    pos = np.stack([0.85 * (k % 5) + 0.0013 * k + 0.31 * s, 1.6 * ((k // 5) % 5) - 0.0007 * k, 10.0 + 2.0 * (k // 25) + 0.11 * s], axis=1)
    return pos, np.array(cw.LABELS, dtype=np.int32)[w]


def test_cpp_facade_equals_python(mrs, tmp_path):
    pos, world = facade_scene()
    path = str(tmp_path / "worlds.bin")
    out = subprocess.run([build_cpp("worlds_test"), path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok written" in out.stdout, out.stdout + out.stderr
    raw = open(path, "rb").read()
    labels, force = np.frombuffer(raw[:600], dtype=np.int32), np.frombuffer(raw[600:], dtype=np.float64).reshape(150, 3)
    g = mrs.Swarm(150, arith=mrs.ARITH_FAST)  # (the facade's default flavour)
    g.construct(0, 150, mrs.default_params(), pos, np.zeros(150))
    g.set_worlds(world)
    g.handle_collisions(True, False, 100.0)
    assert np.array_equal(labels, g.get_worlds()) and np.array_equal(labels, world)
    assert np.array_equal(force, g.get_external_force())
    z = np.zeros(150)
    lists = cw.list_sets(pos, world)
    assert max(len(x) for x in lists) <= cw.LIST_CAP
    p = mrs.default_params()
    want = cw.restatement(pos, world, z + p.arm_length, z + p.prop_radius, z + p.mass, False, 100.0)
    helpers.assert_close(force, want["force"], RTOL_FAST, "the facade's forces")
