"""Collision worlds in the CPU oracle (oracle/uav_oracle.c, orc_swarm_set_worlds): the labelled oracle swarm equals, bit for bit, one
oracle swarm per world that holds the world's UAVs in ascending index (the statement of include/mrs_swarm.h, "collision worlds"), its
partner and crash sets are those of collision_worlds.restatement, a swarm with one label runs the unlabelled loop, and the labels
belong to the slot.  No GPU."""
import numpy as np
import pytest

import collision_thresholds as ct
import collision_worlds as cw
import helpers
from collision_threshold_swarms import REBOUNCE, oracle_swarm

SCENES = {"stacked": lambda: cw.stacked(False), "interleaved": lambda: cw.stacked(True), "many pairs": cw.many_pairs,
          "clusters": lambda: cw.clusters()[:3], "wide": cw.wide}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def one_pass(O, pos, af, world, crash):
    o = oracle_swarm(O, pos, af)
    if world is not None:
        o.set_worlds(world)
    o.handle_collisions(True, crash, REBOUNCE)
    return o.has_crashed(), o.get_external_force()


@pytest.mark.parametrize("crash", [False, True], ids=["elastic", "crash"])
@pytest.mark.parametrize("name", list(SCENES))
def test_labelled_oracle_is_one_oracle_per_world(oracle, name, crash):
    pos, world, af = SCENES[name]()
    n = len(pos)
    crashed, force = one_pass(oracle, pos, af, world, crash)
    want_crashed, want_force = np.zeros(n, dtype=np.int32), np.zeros((n, 3))
    for _, idx in cw.split(world):
        want_crashed[idx], want_force[idx] = one_pass(oracle, pos[idx], af[idx], None, crash)
    assert np.array_equal(crashed, want_crashed), f"{name}: crash flags"
    assert np.array_equal(bits(force), bits(want_force)), f"{name}: forces differ in their bits"
    # the partner and crash sets of the restatement
    arm, prop, mass = ct.constants(af)
    r = cw.restatement(pos, world, arm, prop, mass, crash, REBOUNCE)
    assert np.array_equal(crashed, r["crashed"]), f"{name}: crash set"
    if not crash:
        touched = np.array([len(p) > 0 for p in r["partners"]])
        assert np.array_equal(np.abs(force).sum(axis=1) > 0, np.abs(r["force"]).sum(axis=1) > 0), f"{name}: partner sets"
        assert not np.any(force[~touched]) and np.isfinite(force).all()
        helpers.assert_close(force, r["force"], 1e-14, f"{name}: forces against the restatement")
    if name in ("stacked", "interleaved", "clusters"):  # (the labels matter: without them the coincident copies meet)
        other = one_pass(oracle, pos, af, None, crash)
        assert not (np.array_equal(other[0], crashed) and np.array_equal(bits(other[1]), bits(force)))


@pytest.mark.parametrize("crash", [False, True], ids=["elastic", "crash"])
@pytest.mark.parametrize("label", [0, 7, -2000000000])
def test_one_label_is_the_unlabelled_oracle(oracle, label, crash):
    for name in ("stacked", "wide"):
        pos, _, af = SCENES[name]()
        want = one_pass(oracle, pos, af, None, crash)
        got = one_pass(oracle, pos, af, np.full(len(pos), label, dtype=np.int32), crash)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])), (name, label)
        assert want[0].any() if crash else np.any(want[1])


def test_labels_belong_to_the_slot(oracle):
    pos, world, af = cw.stacked(True)
    n = len(pos)
    o = oracle_swarm(oracle, pos, af)
    assert np.array_equal(o.get_worlds(), np.zeros(n, dtype=np.int32)) and o.get_worlds(10, 0).shape == (0,)
    o.set_worlds(world[20:90], first=20)
    want = np.zeros(n, dtype=np.int32)
    want[20:90] = world[20:90]
    assert np.array_equal(o.get_worlds(), want) and np.array_equal(o.get_worlds(19, 3), want[19:22])
    o.set_worlds(np.zeros(0, dtype=np.int32), first=5)  # (nothing)
    o.construct(30, 40, helpers.oracle_params("x500"), pos[30:70])
    st = o.get_state(0, n)
    o.set_state(0, n, st["x"] + 1.0, st["v"], st["R"], st["omega"], st["motor_rpm"])
    assert np.array_equal(o.get_worlds(), want), "construct / set_state moved a label"
    assert o.get_worlds().dtype == np.int32
