"""The collision predicates at their exact thresholds, on every path that evaluates them on the GPU.

The cases of tests/collision_thresholds.py (pairs whose squared distance is a threshold exactly, an ulp below it, or on either side of
it depending on whether the sum is contracted) run through the stand-alone pass (search tick and list tick), the search's fallback
path, the list-building sweep, the collision evaluation fused into the step kernels (single-airframe and mixed blocks, listed
partners behind the prefetched ones), the sharded evaluation with foreign partners, and a tick rollout — in LITERAL and FAST, elastic
and crash mode, each against the numpy restatement AND the oracle.  Crash flags, the sets of UAVs with a non-zero force and list
contents must be equal exactly; forces within 1e-12 (LITERAL) or RTOL_FAST (FAST) of the restatement.

A fused launch's force is never written out — the step consumes it — so the fused tests read it from what it does: the UAVs rest on the
ground plane (ACTUATOR_CMD far below hover, R = I, v = omega = 0, z = ground_z, pairs in the plane with dz = 0), where a step without
force leaves a position bit-identical, and a UAV is pushed exactly when its x or y has changed after the step."""
import numpy as np
import pytest

import collision_thresholds as ct
import helpers
from helpers import RTOL_FAST, RTOL_LITERAL
from collision_threshold_swarms import (DT, N_MOTORS, REBOUNCE, arith_of, fused_scenarios, oracle_lockstep, oracle_swarm, params, product,
                                        references)
from collision_threshold_swarms import cluster_preconditions
from test_export_sets_gpu import VirtualShards

pytestmark = pytest.mark.gpu
ARITH = pytest.mark.parametrize("fast", [False, True], ids=["literal", "fast"])
CRASH = pytest.mark.parametrize("crash", [False, True], ids=["elastic", "crash"])

def assert_displacement(x, xo, pos, rtol, what):
    """displacements from `pos` against the oracle's: within rtol of the largest one, plus two ulps of the coordinate itself"""
    err = np.abs((x - pos) - (xo - pos))
    tol = rtol * np.abs(xo - pos).max() + 2 * np.spacing(np.abs(xo))
    assert np.all(err <= tol), f"{what}: displacement off by {(err - tol).max():.3e} beyond its tolerance at UAV {int(np.argmax((err - tol).max(axis=1)))}"


def differing(a, b):
    return np.nonzero(np.asarray(a) != np.asarray(b))[0][:12].tolist()


def check_result(crashed, force, want, crash, fast, what):
    """crash flags and the set of pushed UAVs exactly, forces within the flavour's tolerance — against restatement and oracle"""
    pushed = np.abs(force).sum(axis=1) > 0
    print(f"{what}: {int(np.asarray(crashed).astype(bool).sum())} crashed, {int(pushed.sum())} pushed")
    if crash:
        assert np.array_equal(crashed, want["crashed"]), f"{what}: crash flags differ at UAVs {differing(crashed, want['crashed'])}"
        assert not pushed.any(), what
    else:
        assert not np.asarray(crashed).any(), what
        assert np.array_equal(pushed, want["pushed"]), f"{what}: pushed sets differ at UAVs {differing(pushed, want['pushed'])}"
        for ref in (want["force"], want["oracle_force"]):
            helpers.assert_close(force, ref, RTOL_FAST if fast else 1e-12, f"{what}: forces")


# ---- the stand-alone pass ---------------------------------------------------------------------------------------------------------
@ARITH
@CRASH
def test_stand_alone_pass_search_tick_and_list_tick(mrs, oracle, fast, crash):
    """all cases in space, mixed airframes.  One swarm: the first handle_collisions is a search tick.  Another: a first call (elastic,
    another rebounce) builds the lists, the second call on the untouched swarm is a list tick — and only its result is read."""
    c = ct.cases(False)
    want = references(oracle, "space", c.pos, c.airframe, crash)
    g = product(mrs, oracle, c.pos, c.airframe, fast)
    g.handle_collisions(True, crash, REBOUNCE)
    check_result(g.has_crashed(), g.get_external_force(), want, crash, fast, "search tick")
    assert g.collision_stats() == (1, 1)
    g = product(mrs, oracle, c.pos, c.airframe, fast)
    g.handle_collisions(True, False, 37.0)
    half = g.get_external_force()
    assert g.collision_stats() == (1, 1) and not g.has_crashed().any()
    g.handle_collisions(True, crash, REBOUNCE)
    check_result(g.has_crashed(), g.get_external_force(), want, crash, fast, "list tick")
    assert g.collision_stats() == (2, 1), "the second call repeated the search"
    assert np.array_equal(np.abs(half).sum(axis=1) > 0, references(oracle, "space", c.pos, c.airframe, False)["pushed"])


@ARITH
@CRASH
def test_search_tick_with_a_threshold_partner_behind_a_full_hit_list(mrs, oracle, fast, crash):
    """clusters whose centre has more contacts than the four hits the query keeps, among them partners AT crit and an ulp below it:
    the search's fallback path decides them (ct.overflow_clusters).  Elastic mode reads the decision from the centre's force.  In
    crash mode a UAV's flag is evaluated in its own lane, from the partner's side: the shell clusters are those where the centre's
    flag hangs on one threshold partner — nobody crashes the f450 among six t650 at d2 == 0.85, one t650 an ulp nearer does.  Then
    the same from the lists."""
    pos, af, clusters = ct.overflow_clusters()
    cluster_preconditions(pos, af, clusters)
    want = references(oracle, "clusters", pos, af, crash)
    for c in clusters:  # literally
        if crash and c["kind"] != "fillers":
            assert want["crashed"][c["centre"]] == (c["kind"] == "shell-below") and all(want["crashed"][i] for i in c["at"] + c["below"])
        if not crash:
            assert want["pushed"][c["centre"]] and all(want["pushed"][i] for i in c["below"]) and not any(want["pushed"][i] for i in c["at"])
    g = product(mrs, oracle, pos, af, fast)
    g.handle_collisions(True, crash, REBOUNCE)
    check_result(g.has_crashed(), g.get_external_force(), want, crash, fast, "clusters, search tick")
    assert g.collision_stats() == (1, 1)
    g = product(mrs, oracle, pos, af, fast)
    g.handle_collisions(True, False, 37.0)
    g.handle_collisions(True, crash, REBOUNCE)
    check_result(g.has_crashed(), g.get_external_force(), want, crash, fast, "clusters, list tick")
    assert g.collision_stats() == (2, 1)


# ---- the list radius ----------------------------------------------------------------------------------------------------------------
def read_lists(g, n):
    count, nbr, cap, radius = g.debug_neighbour_lists()
    assert radius * radius * (1.0 + 1e-9) + 1e-5 == ct.LIST_R2, "the generator's LIST_R2 is not the library's"
    return [nbr[:count[i], i].astype(np.int64).tolist() for i in range(n)]


@ARITH
def test_list_radius_with_cells_and_quantisation_against_it(mrs, oracle, fast):
    """pairs at LIST_R2 across all 26 cell offsets, in-cell positions on the lines of a 1/1024 grid, at the far end of a cell and a
    hair below zero: the lists equal brute force — `at` and `fma-out` pairs absent, `below` and `fma-in` pairs present"""
    pos, first, second, cls, direction = ct.list_radius_cases()
    n = len(pos)
    zero = np.zeros(n)
    want = ct.restatement(pos, zero, zero, zero, False, radius2=ct.LIST_R2)["neighbours"]
    assert len({tuple(d) for d in direction}) == 26
    g = product(mrs, oracle, pos, np.array(["x500"] * n, dtype=object), fast)
    got = read_lists(g, n)
    bad = [(i, got[i], want[i].tolist()) for i in range(n) if got[i] != want[i].tolist()]
    assert not bad, f"{len(bad)} of {n} lists differ, first: {bad[:4]}"
    inside = np.isin(cls, [ct.CLASSES.index("below"), ct.CLASSES.index("fma-in")])
    for k in range(len(first)):
        i, j = int(first[k]), int(second[k])
        assert got[i] == ([j] if inside[k] else []) and got[j] == ([i] if inside[k] else []), (k, ct.CLASSES[cls[k]], tuple(direction[k]))
    # and the LIST_R2 pairs among all the cases, the far-out ones included
    c = ct.cases(False)
    want = ct.restatement(c.pos, np.zeros(c.n), np.zeros(c.n), np.zeros(c.n), False, radius2=ct.LIST_R2)["neighbours"]
    got = read_lists(product(mrs, oracle, c.pos, c.airframe, fast), c.n)
    bad = [(i, got[i], want[i].tolist()) for i in range(c.n) if got[i] != want[i].tolist()]
    assert not bad, f"all cases: {len(bad)} of {c.n} lists differ, first: {bad[:4]}"
    for k in c.pairs_of("LIST_R2", "at").tolist() + c.pairs_of("LIST_R2", "fma-out").tolist():
        assert got[c.first[k]] == [] and got[c.second[k]] == []
    for k in c.pairs_of("LIST_R2", "below").tolist() + c.pairs_of("LIST_R2", "fma-in").tolist():
        assert got[c.first[k]] == [c.second[k]] and got[c.second[k]] == [c.first[k]]


# ---- the evaluation fused into the step kernels ---------------------------------------------------------------------------------------
def check_moved(g, pos, want, crash, fast, what, O, af, calls):
    """after the step that consumed the evaluated force: exactly the pushed UAVs have moved (crash mode: nobody), everybody else is
    where it was set bit for bit, crash flags are the expected ones, and the state is the oracle's after the same calls"""
    x = g.get_state()["x"]
    moved = np.any(x != pos, axis=1)
    assert np.all(x[:, 2] == 0.0), what
    expect = np.zeros(len(pos), dtype=bool) if crash else want["pushed"]
    print(f"{what}: {int(moved.sum())} UAVs moved, {int(g.has_crashed().sum())} crashed")
    bad = differing(moved, expect)
    assert not bad, f"{what}: moved and pushed sets differ at UAVs {bad}, displaced by {(x - pos)[bad].tolist()}"
    assert np.array_equal(g.has_crashed(), want["crashed"]), f"{what}: crash flags differ at UAVs {differing(g.has_crashed(), want['crashed'])}"
    so, co = oracle_lockstep(O, pos, af, calls)
    assert np.array_equal(co, want["crashed"]) and np.array_equal(np.any(so["x"] != pos, axis=1), expect), f"{what}: the oracle disagrees with the restatement"
    assert_displacement(x, so["x"], pos, RTOL_FAST if fast else RTOL_LITERAL, what)


@pytest.mark.parametrize("scenario", ["x500 only", "giant only", "mixed", "deep lists"])
@ARITH
@CRASH
def test_fused_evaluation(mrs, oracle, scenario, fast, crash):
    """x500 / giant only: one airframe, the buffer kernel.  mixed: airframe runs that end inside blocks (mrs_uav_step_mixed_coll), the
    asymmetric pairs among them.  deep lists: the threshold partner is entry 5 or 6 of a list of six (the loop behind MRS_NPRE).
    (a) list tick: two ticks without force build the lists; the tick under test is evaluated by the NEXT step launch from the lists,
    and a last tick without a collision pass keeps a stand-alone pass from evaluating anything after it.
    (b) search tick: the first tick of a fresh swarm, evaluated by the search before the second step.
    (c) five ticks in a row: search tick, list ticks and the pass at the end all see the pairs that stay at their thresholds."""
    pos, af = fused_scenarios()[scenario]
    want = references(oracle, scenario, pos, af, crash)
    if scenario == "deep lists":
        lists = ct.restatement(pos, np.zeros(len(pos)), np.zeros(len(pos)), np.zeros(len(pos)), False, radius2=ct.LIST_R2)["neighbours"]
        deep = ct.deep_list_cases()
        assert all(len(lists[i]) == 6 and lists[i].tolist().index(j) in (4, 5) for i, j in zip(deep.second, deep.first))
    # (a)
    g = product(mrs, oracle, pos, af, fast, grounded=True)
    g.tick_n(DT, 2, True, False, 0.0)
    g.tick_n(DT, 1, True, crash, REBOUNCE)
    g.tick_n(DT, 1, False, False, 0.0)
    fused, stalls, _, ahead = g.fused_stats()
    assert fused >= 2 and (stalls, ahead) == (0, 0) and g.collision_stats() == (3, 1), (g.fused_stats(), g.collision_stats())
    calls = [(2, True, False, 0.0), (1, True, crash, REBOUNCE), (1, False, False, 0.0)]
    check_moved(g, pos, want, crash, fast, f"{scenario}: list tick in a step launch", oracle, af, calls)
    # the force the launch evaluated, written out afterwards from the positions it saw
    check_result(g.has_crashed(), g.get_external_force(), want, crash, fast, f"{scenario}: latched force")
    # the precondition, in this flavour: without force nobody moves
    g = product(mrs, oracle, pos, af, fast, grounded=True)
    g.tick_n(DT, 3, True, False, 0.0)
    st = g.get_state()
    assert np.array_equal(st["x"], pos) and np.all(st["v"] == 0), f"{scenario}: resting UAVs move without a force"
    # (b)
    g = product(mrs, oracle, pos, af, fast, grounded=True)
    g.tick_n(DT, 1, True, crash, REBOUNCE)
    g.tick_n(DT, 1, False, False, 0.0)
    assert g.collision_stats() == (1, 1)
    check_moved(g, pos, want, crash, fast, f"{scenario}: search tick", oracle, af, [(1, True, crash, REBOUNCE), (1, False, False, 0.0)])
    # (c)
    g = product(mrs, oracle, pos, af, fast, grounded=True)
    g.tick_n(DT, 5, True, crash, REBOUNCE)
    x, so = g.get_state()["x"], oracle_lockstep(oracle, pos, af, [(5, True, crash, REBOUNCE)])
    still = ~want["pushed"] if not crash else np.ones(len(pos), dtype=bool)
    assert np.array_equal(x[still], pos[still]), f"{scenario}: UAVs that nobody may push moved within five ticks: {differing(np.any(x != pos, axis=1), ~still)}"
    assert np.any(x != pos, axis=1)[~still].all()
    assert np.array_equal(g.has_crashed(), so[1]) and np.array_equal(so[1], want["crashed"])
    assert_displacement(x, so[0]["x"], pos, RTOL_FAST if fast else RTOL_LITERAL, f"{scenario}: after five ticks")
    assert g.fused_stats()[0] >= 3


# ---- sharded: every partner foreign ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", ["export sets", "full gather"])
@ARITH
@CRASH
def test_sharded_pairs_across_the_slab_boundary(mrs, oracle, exchange, fast, crash):
    """two slabs, every pair with one UAV in each: a partner's constants come with its export slot, and the asymmetric pairs are
    evaluated once on each rank.  (a) the pass at the end of a call; (b) the evaluation inside the next step launch."""
    M = mrs
    c = ct.straddle_cases()
    want = references(oracle, "straddle", c.pos, c.airframe, crash)
    order = M.slab_partition(c.pos, 2)
    rank = np.empty(c.n, dtype=np.int64)
    rank[order] = np.arange(c.n) // (c.n // 2)
    assert c.n % 2 == 0 and np.all(rank[c.first] != rank[c.second]), "a pair lies within one slab"
    po = [helpers.to_product_params(M, params(oracle, name)) for name in sorted(set(c.airframe))]
    po = [po[sorted(set(c.airframe)).index(name)] for name in c.airframe]
    st = dict(x=c.pos, v=np.zeros((c.n, 3)), R=np.tile(np.eye(3), (c.n, 1, 1)), omega=np.zeros((c.n, 3)), motor_rpm=np.zeros((c.n, 8)))
    mode = np.full(c.n, oracle.ACTUATOR_CMD)
    rows = [np.full(N_MOTORS[name], 0.1) for name in c.airframe]
    ex = M.EXCHANGE_EXPORT_SETS if exchange == "export sets" else M.EXCHANGE_FULL_GATHER

    def shards():
        return VirtualShards(M, 2, order, po, c.pos, np.zeros(c.n), st, mode, rows, arith_of(M, fast), ex)

    # (a)
    vs = shards()
    vs.tick_n(1, True, False, 0.0)
    vs.tick_n(1, True, crash, REBOUNCE)
    a = vs.gather()
    assert np.array_equal(a["x"], c.pos), "resting UAVs move without a force"
    check_result(a["crashed"], a["f"], want, crash, fast, f"{exchange}: pass at the end of a call")
    vs.close()
    # (b)
    vs = shards()
    vs.tick_n(1, True, False, 0.0)
    vs.tick_n(2, True, crash, REBOUNCE)
    a = vs.gather()
    moved = np.any(a["x"] != c.pos, axis=1)
    expect = np.zeros(c.n, dtype=bool) if crash else want["pushed"]
    assert np.array_equal(moved, expect), f"{exchange}: moved and pushed sets differ at UAVs {differing(moved, expect)}"
    assert np.array_equal(a["crashed"], want["crashed"])
    o = oracle_swarm(oracle, c.pos, c.airframe, grounded=True)
    for enabled, cr, reb in [(True, False, 0.0), (True, crash, REBOUNCE), (True, crash, REBOUNCE)]:
        o.step(DT)
        o.handle_collisions(enabled, cr, reb)
    assert_displacement(a["x"], o.get_state()["x"], c.pos, RTOL_FAST if fast else RTOL_LITERAL, f"{exchange}: after the second tick")
    helpers.assert_close(a["f"], o.get_external_force(), RTOL_FAST if fast else 1e-12, f"{exchange}: forces after the second tick vs oracle")
    assert np.array_equal(a["crashed"], o.has_crashed())
    vs.close()


# ---- tick rollouts ----------------------------------------------------------------------------------------------------------------------
@ARITH
@CRASH
def test_tick_rollout_rows_equal_tick_n(mrs, oracle, fast, crash):
    """four ticks of the mixed resting swarm as one rollout_ticks call and as four tick_n calls with the rows read in between: the crash
    rows (crash mode) and the position rows (elastic mode: who has been pushed, and how far) are the same, and the expected ones"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    pos, af = fused_scenarios()["mixed"]
    n, ticks = len(pos), 4
    want = references(oracle, "mixed", pos, af, crash)
    a = product(mrs, oracle, pos, af, fast, grounded=True)
    b = product(mrs, oracle, pos, af, fast, grounded=True)
    rows_a, crash_a = np.zeros((ticks, n, 3)), np.zeros((ticks, n), dtype=bool)
    for t in range(ticks):
        crash_a[t] = a.has_crashed() != 0  # a row is taken after the tick's step and before its collision pass
        a.tick_n(DT, 1, True, crash, REBOUNCE)
        rows_a[t] = a.get_state()["x"]
    cmd = torch.full((ticks, n, 8), 0.1, dtype=torch.float64, device=torch.device("cuda", b.device()))
    rows_b, crash_b = T.rollout_ticks(b, oracle.ACTUATOR_CMD, cmd, DT, crash, REBOUNCE, T.OBS_POS)
    rows_b, crash_b = rows_b.cpu().numpy(), crash_b.cpu().numpy().astype(bool)
    assert np.array_equal(crash_a, crash_b), "crash rows differ"
    moved_a, moved_b = np.any(rows_a != pos, axis=2), np.any(rows_b != pos, axis=2)
    assert np.array_equal(moved_a, moved_b), f"the rollout pushed other UAVs than the ticks did: {differing(moved_a.any(axis=0), moved_b.any(axis=0))}"
    if fast:
        for t in range(ticks):
            assert_displacement(rows_b[t], rows_a[t], pos, RTOL_FAST, f"position row {t}")
    else:
        assert np.array_equal(rows_a, rows_b), "position rows differ"
    assert np.array_equal(b.has_crashed(), a.has_crashed()) and np.array_equal(b.has_crashed(), want["crashed"])
    # and the expected ones: nothing before the first collision pass; its result in the row after it
    assert not crash_b[0].any() and not moved_b[0].any()
    if crash:
        assert np.array_equal(crash_b[1], want["crashed"] != 0) and np.array_equal(crash_b[3], want["crashed"] != 0) and not moved_b.any()
    else:  # (the step of tick 1 consumed the force of tick 0's pass)
        assert np.array_equal(moved_b[1], want["pushed"]) and np.array_equal(moved_b[3], want["pushed"]) and not crash_b.any()
    assert b.fused_stats()[0] >= 2


# ---- what keeps the planar scenarios off the axes --------------------------------------------------------------------------------------
@ARITH
def test_drift_of_a_resting_uav_at_the_origin(mrs, oracle, fast):
    """The planar scenarios have no x or y of exactly 0.0 (ct.Cases): a FAST step moves a UAV that rests on the ground by a rounding
    residue which every other coordinate absorbs.  This pins its size, so that it is tracked and not just avoided.  LITERAL: the UAV at
    the origin stays at 0.0 exactly.  FAST: per tick below 1e-24 m — equal throttles leave a torque of a few ulps of one motor's
    (0.25 m * kf * rpm^2 ~ 0.04 N m, so ~1e-17 N m), over J ~ 1e-2 kg m^2 and one step an attitude error of ~1e-21 rad before the
    ground clamp zeroes the rates again, which tilts g by 1e-20 m/s^2: 5e-27 m in a step, taken with a margin of 200.  (Some 1.5e-33 m
    per tick are observed.)"""
    pos = np.array([[0.0, 0.0, 0.0], [40.0, 0.0, 0.0], [0.0, -40.0, 0.0]])
    g = product(mrs, oracle, pos, np.array(["x500"] * 3, dtype=object), fast, grounded=True)
    ticks = 8
    g.tick_n(DT, ticks, True, False, 0.0)
    d = np.abs(g.get_state()["x"] - pos)
    print(f"{'FAST' if fast else 'LITERAL'}: largest displacement of a resting UAV after {ticks} ticks: {d.max():.3e} m")
    assert np.all(d[:, 2] == 0.0) and d.max() <= (ticks * 1e-24 if fast else 0.0)
