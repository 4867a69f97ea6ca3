"""The collision predicates at their exact thresholds, on the CPU: the generator of tests/collision_thresholds.py delivers its
classes, its numpy restatement of handleCollisions equals the oracle on every case, the d2 < 3.0 sets are those of the reference's
own kd-tree, and the rule for the two airframe pairs whose crit differs by an ulp between its two orders is asserted literally.
tests/test_collision_thresholds_gpu.py runs the same cases through every kernel that holds a copy of the predicate."""
import os
import re

import numpy as np
import pytest

import collision_thresholds as ct
import helpers
from collision_threshold_swarms import cluster_preconditions, fused_scenarios, oracle_lockstep, oracle_params, references, runs
from mrs_multirotor_simulator_amd import airframes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collision_threshold_sets.npz")
FORCE_RTOL = 1e-14  # forces against the oracle, as tests/test_collisions_ref.py


def test_airframe_constants_are_the_shipped_ones():
    for name, (arm, prop, mass) in ct.AIRFRAME.items():
        if name != "giant":
            a = airframes.AIRFRAMES[name]
            assert (a["arm_length"], a["prop_radius"], a["mass"]) == (arm, prop, mass), name
    assert max(ct.crit(a, b) for a in airframes.AIRFRAMES for b in airframes.AIRFRAMES if a in ct.AIRFRAME and b in ct.AIRFRAME) < 3.0 < ct.crit("giant", "giant")
    text = open(os.path.join(helpers.CSRC, "collide_work.h")).read()  # LIST_R2 is built from the constants the kernels are compiled with
    assert float(re.search(r"#define MRS_SKIN ([0-9.]+)", text).group(1)) == ct.SKIN
    assert float(re.search(r"SQRT3_UP\s*=\s*([0-9.]+);", text).group(1)) == ct.SQRT3_UP
    assert "INV_CELL_WIDE = 1.0 / (SQRT3_UP + SKIN + 0.0179491924);" in text and ct.WIDE_EDGE_INV == 1.0 / (ct.SQRT3_UP + ct.SKIN + 0.0179491924)
    assert "LIST_R2       = (SQRT3_UP + SKIN) * (SQRT3_UP + SKIN) * (1.0 + 1e-9) + 1e-5;" in text and abs(ct.LIST_R2 - 4.98206) < 1e-5


@pytest.mark.parametrize("planar", [False, True], ids=["space", "plane"])
def test_every_class_is_filled(planar):
    """at least 16 pairs per class and threshold among the near-origin and cell-face anchors; the far-out group gives what it gives"""
    c = ct.cases(planar)
    print(c.report())
    print(f"{c.n} UAVs, {len(c.first)} pairs, {int(c.far.sum())} of them at |x| = 2^17 m")
    c.check_counts()
    assert c.n <= 3000
    assert c.far.sum() > 0, "the far-out group came out empty"
    if planar:
        assert np.all(c.pos[:, 2] == 0.0) and np.all(c.pos[:, :2] != 0.0)
    # no airframe run ends on a 64-UAV block boundary: the asymmetric pairs of the planar set sit in mixed blocks of the step kernels
    ends = [a + m for a, m, _ in runs(c.airframe.tolist())][:-1]
    assert len(ends) >= 11 and all(e % 64 for e in ends), ends
    if not planar:
        assert np.any(np.all(c.pos == 0.0, axis=1)), "the origin itself is an anchor"


def test_fma_emulation():
    assert ct.fma(0.1, 10.0, -1.0) == 5.551115123125783e-17 and 0.1 * 10.0 - 1.0 == 0.0
    for planar in (False, True):
        c = ct.cases(planar)
        flips = []
        for k in np.nonzero(c.cls >= 2)[0]:
            a, b, T = c.pos[c.first[k]], c.pos[c.second[k]], c.T(k)
            w, full = float(ct.d2_written(a, b)), ct.d2_contracted(a, b)[0]
            flips.append([(w < T) != (f < T) for f in full])
            assert any(flips[-1]) and (w < T) == (ct.CLASSES[c.cls[k]] == "fma-in")
            assert float(ct.d2_written(b, a)) == w  # the same from the partner's side
        # whichever product a compiler fuses into the first addition, a good third of the pairs of the fma classes falls for it
        assert min(np.sum(flips, axis=0)) >= 0.4 * len(flips), np.sum(flips, axis=0)


def oracle_result(O, c, crash):
    s = O.OracleSwarm(c.n)
    for a, m, name in runs(c.airframe.tolist()):
        s.construct(a, m, oracle_params(O, name), c.pos[a:a + m], np.zeros(m))
    assert np.array_equal(s.get_state()["x"], c.pos)
    s.handle_collisions(True, crash, 100.0)
    return s.has_crashed(), s.get_external_force()


def class_expectation(c, crash):
    """who is touched, by the rule stated class by class (not by evaluating the predicate again): per UAV True / False.
    at / fma-out pairs: nobody.  below / fma-in pairs: both — except on the two values of an asymmetric crit:
      d2 at the smaller value          : only the side whose crit(actor, other) is the larger one acts
      d2 an ulp below the larger value : the same (that d2 IS the smaller value, the two being neighbours)
    the actor is pushed in elastic mode; the OTHER one crashes in crash mode.  LIST_R2 pairs never touch."""
    hit = np.zeros(c.n, dtype=bool)
    for k in range(len(c.first)):
        name, T, a, b = c.thresholds[c.thr[k]]
        cl = ct.CLASSES[c.cls[k]]
        i, j = c.first[k], c.second[k]  # airframes a, b
        if name == "LIST_R2":
            continue
        inside = cl in ("below", "fma-in")
        if a == b:
            hit[i] = hit[j] = inside
            continue
        big_actor, small_actor = (i, j) if ct.crit(a, b) > ct.crit(b, a) else (j, i)
        lo, hi = sorted((ct.crit(a, b), ct.crit(b, a)))
        w = float(ct.d2_written(c.pos[i], c.pos[j]))  # (the fma classes say on which side of T d2 lies, not how far: that is looked up)
        if name.endswith("smaller"):
            acts = [big_actor, small_actor] if inside else [big_actor] if cl == "at" or w == lo else []
        else:
            acts = [] if not inside else [big_actor] if cl == "below" or w == lo else [big_actor, small_actor]
        for actor in acts:
            other = j if actor == i else i
            hit[other if crash else actor] = True
    return hit


@pytest.mark.parametrize("crash", [False, True], ids=["elastic", "crash"])
@pytest.mark.parametrize("planar", [False, True], ids=["space", "plane"])
def test_restatement_equals_oracle(oracle, planar, crash):
    c = ct.cases(planar)
    arm, prop, mass = ct.constants(c.airframe)
    want = ct.restatement(c.pos, arm, prop, mass, crash)
    crashed, force = oracle_result(oracle, c, crash)
    hit = class_expectation(c, crash)
    if crash:
        assert np.array_equal(crashed, want["crashed"])
        assert np.array_equal(crashed != 0, hit), "the restatement and the rule stated per class disagree"
        assert np.all(force == 0)
    else:
        assert not crashed.any()
        assert np.array_equal(np.abs(force).sum(axis=1) > 0, np.abs(want["force"]).sum(axis=1) > 0)
        assert np.array_equal(np.abs(force).sum(axis=1) > 0, hit), "the restatement and the rule stated per class disagree"
        helpers.assert_close(force, want["force"], FORCE_RTOL, "forces")
    assert all(len(p) <= 1 for p in want["partners"]) and hit.sum() > 0.4 * c.n


def test_asymmetric_crit_literally(oracle):
    """f450/t650: 0.8500000000000001 seen from the f450, 0.85 from the t650; naki/t650: 0.845 from the naki, 0.8450000000000001 from
    the t650.  At d2 == 0.85 the f450 is pushed in elastic mode and the t650 is not; in crash mode the t650 crashes and the f450 does
    not.  For naki/t650 at d2 == 0.845 it is the t650 that is pushed and the naki that crashes."""
    assert (ct.crit("f450", "t650"), ct.crit("t650", "f450")) == (0.8500000000000001, 0.85)
    assert (ct.crit("naki", "t650"), ct.crit("t650", "naki")) == (0.845, 0.8450000000000001)
    assert np.nextafter(0.85, 1.0) == 0.8500000000000001 and np.nextafter(0.845, 1.0) == 0.8450000000000001
    c = ct.cases(False)
    res = {crash: oracle_result(oracle, c, crash) for crash in (False, True)}
    pushed = np.abs(res[False][1]).sum(axis=1) > 0
    crashed = res[True][0] != 0
    for other, lo, first_acts in (("f450", 0.85, True), ("naki", 0.845, False)):
        at_lo = c.pairs_of(f"crit {other}/t650 smaller", "at")
        assert len(at_lo) >= 16
        for k in at_lo:
            i, j = c.first[k], c.second[k]
            assert (c.airframe[i], c.airframe[j]) == (other, "t650") and float(ct.d2_written(c.pos[i], c.pos[j])) == lo
            actor, passive = (i, j) if first_acts else (j, i)
            assert pushed[actor] and not pushed[passive] and crashed[passive] and not crashed[actor], k
        for k in c.pairs_of(f"crit {other}/t650 larger", "at"):
            i, j = c.first[k], c.second[k]
            assert float(ct.d2_written(c.pos[i], c.pos[j])) == np.nextafter(lo, 1.0)
            assert not (pushed[i] or pushed[j] or crashed[i] or crashed[j]), k
        for k in c.pairs_of(f"crit {other}/t650 smaller", "below"):
            i, j = c.first[k], c.second[k]
            assert pushed[i] and pushed[j] and crashed[i] and crashed[j], k


def radius_points(c):
    """the UAVs of the threshold-3.0 pairs (first members, then second members)"""
    k = np.nonzero(c.thr == [x[0] for x in c.thresholds].index("3.0"))[0]
    return np.concatenate([c.pos[c.first[k]], c.pos[c.second[k]]]), c.cls[k]


@pytest.mark.parametrize("planar", [False, True], ids=["space", "plane"])
def test_radius_sets_are_those_of_the_reference_kdtree(oracle, planar):
    """tests/golden/collision_threshold_sets.npz (tests/golden/make_golden.py:collision_threshold_sets): the reference's own nanoflann,
    radiusSearch(3.0), leaf size 10, on the threshold-3.0 cases.  The stored points are the generator's bit for bit; the stored lists
    are the restatement's d2 < 3.0 sets (plus the query point itself), and where oracle/_ref is built the library still returns them."""
    key = "plane" if planar else "space"
    pts, cls = radius_points(ct.cases(planar))
    g = np.load(GOLDEN)
    assert np.array_equal(g[f"{key}_points"], pts), "the stored points are no longer the generator's"
    off, idx, d2 = g[f"{key}_offsets"], g[f"{key}_indices"], g[f"{key}_d2"]
    if oracle.ref_lib() is not None:
        lo, li, ld = oracle.ref_radius_neighbours(pts, 3.0, 10)
        assert np.array_equal(lo, off) and np.array_equal(li, idx) and np.array_equal(ld, d2), "live kd-tree != stored lists"
    n, m = len(pts), len(pts) // 2
    zero = np.zeros(n)
    want = ct.restatement(pts, zero, zero, zero, False)["neighbours"]
    for i in range(n):
        got = sorted(int(j) for j in idx[off[i]:off[i + 1]] if j != i)
        assert i in idx[off[i]:off[i + 1]]
        assert got == want[i].tolist(), f"UAV {i}: kd-tree {got}, restatement {want[i].tolist()}"
    inside = np.isin(cls, [ct.CLASSES.index("below"), ct.CLASSES.index("fma-in")])
    for k in range(m):  # and literally: `at` and `fma-out` pairs are no neighbours, `below` and `fma-in` pairs are
        assert want[k].tolist() == ([k + m] if inside[k] else []) and want[k + m].tolist() == ([k] if inside[k] else [])
    assert inside.sum() >= 32 and (~inside).sum() >= 32


@pytest.mark.parametrize("scenario", ["x500 only", "giant only", "mixed", "deep lists"])
def test_resting_uavs_stay_where_they_are(oracle, scenario):
    """the precondition of the fused GPU tests, on the CPU first: UAVs resting on the ground plane under throttles far below hover
    keep their positions bit for bit through four ticks without force — and the oracle agrees with the restatement on who is
    touched in these planar scenarios"""
    pos, af = fused_scenarios()[scenario]
    st, crashed = oracle_lockstep(oracle, pos, af, [(4, True, False, 0.0)])
    assert np.array_equal(st["x"], pos) and np.all(st["v"] == 0) and not crashed.any()
    for crash in (False, True):
        references(oracle, scenario, pos, af, crash)
    st, crashed = oracle_lockstep(oracle, pos, af, [(1, True, False, 100.0), (1, False, False, 0.0)])
    assert np.array_equal(np.any(st["x"] != pos, axis=1), references(oracle, scenario, pos, af, False)["pushed"])
    assert np.all(st["x"][:, 2] == 0.0)


@pytest.mark.parametrize("crash", [False, True], ids=["elastic", "crash"])
def test_overflow_clusters_leave_the_decision_to_the_threshold_partner(oracle, crash):
    """the clusters of the hit-list overflow GPU test: who can act on whom (cluster_preconditions), and restatement == oracle on them"""
    pos, af, clusters = ct.overflow_clusters()
    cluster_preconditions(pos, af, clusters)
    want = references(oracle, "clusters", pos, af, crash)
    shells = [c for c in clusters if c["kind"] != "fillers"]
    if crash:
        assert [bool(want["crashed"][c["centre"]]) for c in shells] == [c["kind"] == "shell-below" for c in shells]
