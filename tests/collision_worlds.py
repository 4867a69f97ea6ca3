"""Scenarios and the numpy restatement of collision worlds (include/mrs_swarm.h, "collision worlds"): UAVs interact through the
collision pass, and list each other as nearest neighbours, only if their 32-bit labels are equal.  The restatement is
collision_thresholds.restatement applied world by world, indices mapped back to the swarm's.  Shared by
tests/test_collision_worlds.py (CPU) and tests/test_collision_worlds_gpu.py."""
import functools

import numpy as np

import collision_thresholds as ct

LABELS = (7, -2000000000, 1234567890)  # far apart, one negative: labels are compared for equality and nothing else
AIRFRAMES = ("x500", "f450", "f550", "t650")
LIST_CAP = 24


def restatement(pos, world, arm, prop, mass, crash, rebounce=100.0, radius2=3.0):
    """ct.restatement of every world on its own (its UAVs in ascending index), with the indices mapped back: neighbours[i] and
    partners[i] hold swarm indices, ascending; crashed[n] and force[n, 3] as there"""
    pos, world = np.asarray(pos, dtype=np.float64), np.asarray(world)
    n = len(pos)
    out = dict(neighbours=[None] * n, partners=[None] * n, crashed=np.zeros(n, dtype=np.int32), force=np.zeros((n, 3)))
    for w in np.unique(world):
        idx = np.nonzero(world == w)[0]
        r = ct.restatement(pos[idx], np.asarray(arm)[idx], np.asarray(prop)[idx], np.asarray(mass)[idx], crash, rebounce, radius2)
        for k, i in enumerate(idx):
            out["neighbours"][i] = idx[r["neighbours"][k]]
            out["partners"][i] = idx[r["partners"][k]]
        out["crashed"][idx] = r["crashed"]
        out["force"][idx] = r["force"]
    return out


def list_sets(pos, world):
    """what the neighbour lists of a world-aware search hold: same-world UAVs within the list radius"""
    z = np.zeros(len(pos))
    return restatement(pos, world, z, z, z, False, radius2=ct.LIST_R2)["neighbours"]


def split(world):
    """[(label, indices)] in order of first appearance"""
    world = np.asarray(world)
    seen = list(dict.fromkeys(world.tolist()))
    return [(w, np.nonzero(world == w)[0]) for w in seen]


def _scene(rng, m, side):
    return rng.uniform(-side / 2, side / 2, (m, 3)) + [0.0, 0.0, 20.0]


@functools.lru_cache(maxsize=None)
def stacked(interleaved=False, seed=1801, per_world=50, side=6.0, mixed=True):
    """3 worlds x 50 UAVs in one 6-m box: world 1 is an exact copy of world 0's positions, world 2 another scene.  Contiguous labels
    (i // 50) or interleaved (i % 3); either way world w holds scene w in ascending index.  Returns (pos, world, airframe)."""
    rng = np.random.default_rng(seed)
    a, c = _scene(rng, per_world, side), _scene(rng, per_world, side)
    scenes = [a, a.copy(), c]
    af = np.array([AIRFRAMES[k % 4] if mixed else "x500" for k in range(per_world)], dtype=object)
    n = 3 * per_world
    i = np.arange(n)
    w, k = (i % 3, i // 3) if interleaved else (i // per_world, i % per_world)
    pos = np.array([scenes[w[t]][k[t]] for t in range(n)])
    return pos, np.array(LABELS, dtype=np.int32)[w], af[k]


@functools.lru_cache(maxsize=None)
def many_pairs(worlds=40):
    """40 worlds x 2 UAVs, every world's pair at the same two points 1 m apart (no contact: d2 = 1 > crit = 0.8).  Each UAV has 79
    UAVs inside the list radius — far beyond the list capacity — and 1 in its own world."""
    n = 2 * worlds
    pos = np.array([[0.3 + (i % 2) * 1.0, -0.4, 12.5] for i in range(n)])
    world = (1000003 * (np.arange(n) // 2) - 17).astype(np.int32)
    z = np.zeros(n)
    every = ct.restatement(pos, z, z, z, False, radius2=ct.LIST_R2)["neighbours"]
    own = list_sets(pos, world)
    assert all(len(e) == n - 1 for e in every) and n - 1 > LIST_CAP and all(len(o) == 1 for o in own)
    return pos, world, np.array(["x500"] * n, dtype=object)


@functools.lru_cache(maxsize=None)
def clusters():
    """ct.overflow_clusters() twice, as two worlds at identical coordinates: the search's hit list overflows in both (the fallback
    path), and every bucket of the hash holds both copies.  Returns (pos, world, airframe, clusters of the first copy)."""
    pos, af, cl = ct.overflow_clusters()
    n = len(pos)
    return np.concatenate([pos, pos]), np.array([5] * n + [-5] * n, dtype=np.int32), np.concatenate([af, af]), cl


@functools.lru_cache(maxsize=None)
def wide(seed=1907, n=300, worlds=6, volume=10.0):
    """300 UAVs, 6 worlds of 50 in one box of about 10 m^3 per UAV and world (1.7 m^3 per UAV over all worlds), labels shuffled"""
    rng = np.random.default_rng(seed)
    side = (n // worlds * volume) ** (1 / 3)
    pos = _scene(rng, n, side)
    world = (rng.permutation(n) % worlds * 77777 - 3).astype(np.int32)
    return pos, world, np.array(["x500"] * n, dtype=object)
