"""The generator of test_random_device_sequences_gpu.py (tests/device_sequences.py) against the oracle alone, with a stub in place of the
product that checks every argument tuple against the header's rules and records it; and the reference rows the GPU module compares
observation rows with, against tests/independent_model.py and against Eigen's four quaternion branches.  No GPU.

Step totals (counted here): the 24 sequences of test_random_sequences_gpu.py take 39 .. 76 steps; the sequences of device_sequences.SEEDS
and VARIANTS take at most STEP_CAP = 76, rollout steps included, and so do those of SEEDS_EXT and VARIANTS_EXT (ticks of a tick rollout
count as steps; the largest takes 76).

The extended surface (counted here, over the 20 seeds of SEEDS_EXT, 8 of them with collision worlds): 27 rollout_ticks, 27
rollout_tick_cost, 25 rollout_feedback, 35 rollout_tick_feedback, 49 proximity_cost and 13 set_worlds calls; one seed takes the 66-tick
horizon through a tick rollout.  The first surface draws what it drew before the second existed: the SHA-256 of every op log is
recorded in tests/golden/device_sequence_logs.json.  The two conditions that keep the comparison of the extended seeds honest — no
same-world pair near its contact threshold at a collision pass, no quaternion near a branch boundary where a feedback reads it — are
asserted here, on the oracle alone, so they are properties of the chosen seeds.

The scene surface (counted here, over the 12 seeds of SEEDS_SCENE, 8 of them with collision worlds, and asserted exactly against
device_sequences.SCENE_COUNTS): 16 set_obstacles, 16 nearest_obstacles, 17 obstacle_cost, 18 set_scan_beams, 41 range_scan and 21
range_scan_uavs calls, 16 of them behind a pending collision tick; scans that follow a call with no other scan in between: 9
set_ground_z, 8 set_params, 7 resets, 8 clone swaps, 7 set_worlds, 12 set_obstacles; 10 stale-table shapes (a table-changing call, a
range_scan without the ground, a scan that reads the table); from the restatements on the oracle's state: beams taken by spheres 448,
boxes 614, cylinders 4862, UAVs 2594, the ground 2725, nothing 64699; 2398 beams of range 0; 66 beams a UAV takes from an obstacle, 63
an obstacle keeps from a UAV; 65 query UAVs with found > k; from the cache model: 29 and 53 grids built for the queries and the scans,
4 and 9 cache hits.  Their sequences keep the step budget and the two honesty conditions, and both earlier surfaces draw what they
drew: the op logs of the extended surface, hashed before the scene surface existed, are in tests/golden/device_sequence_logs_ext.json.

The contact surface (counted here, over the 12 seeds of SEEDS_CONTACT, 7 of them with collision worlds and 2 with model-only phases,
and asserted exactly against device_sequences.CONTACT_COUNTS): 34 obstacle_contacts calls without the mark and 59 with it, 12 and 13
of them behind a pending collision tick; 7 marks among the followers of a stall recipe, 25 while a pipelined download was open; from
the restatement on the oracle's state: 302 UAVs touching, 44 of them more than one obstacle, 94 newly marked, 53 of those shown by the
first crash row of a later tick rollout, 27 marks of nobody; contact calls that follow a call with no other contact call in between: 8
set_ground_z, 10 set_params, 8 resets, 10 clone swaps, 5 set_worlds, 12 set_obstacles; from the cache model: 66 grids built for the
third entry, 27 cache hits.  The conditions the seeds were chosen to keep are asserted beside the counts (at least 20 calls of each
form, 5 of each behind a pending tick, 2 marks behind a stall recipe, 40 UAVs newly marked, 5 seen in a crash row, a mark of nobody, a
contact call after each of the six SCAN_MARKS, 3 cache hits and 10 builds, no seed with more than half of its UAVs crashed at its
end), and so are the step cap, the limits of test_the_oracle_stays_usable and all three honesty conditions: the two above and
obstacle_contact_violations == 0 at every marking call.  The op logs of the scene surface, hashed before the contact surface existed,
are in tests/golden/device_sequence_logs_scene.json (the three variant seeds included), and the two older golden files pass unchanged."""
import numpy as np
import pytest

import device_sequences as D
import helpers
import independent_model as IM
import test_random_sequences_gpu as E
from oracle import oracle_swarm as O
from test_rollout_cost_gpu import restate


def dry_run(mrs, seed, split=False):
    surface = D.surface_of(seed)
    _, fast, fleet, long_rollout, model, worlds = D.SEEDS[seed] + (False,) if surface == "base" else D.ext_flags(seed)
    p = D.StubPair(mrs, D.N_UAVS)
    dev = D.Stub(p)
    res = D.run_sequence(p, dev, mrs, np.random.default_rng(D.RNG_BASE + seed), seed, fast, fleet, D.seed_rtol(fast), D.STEP_CAP, split=split,
                         long_rollout=long_rollout, model=model, surface=surface, worlds=worlds)
    st = p.o.get_state()
    res["non_finite_uavs"] = int((~np.isfinite(np.concatenate([st[k].reshape(p.n, -1) for k in st], axis=1))).any(axis=1).sum())
    res["calls"], res["product_calls"] = dev.calls, p.g.calls
    assert not dev.open["outputs"] and not dev.open["poses"], "tickets left open at the end of the sequence"
    return res


@pytest.fixture(scope="module")
def runs(mrs):
    """every sequence the GPU module runs: {(variant or None, seed): result}; a seed's number says which surface it draws from
    (D.surface_of), in every variant"""
    out = {(None, seed): dry_run(mrs, seed) for seed, *_ in D.SEEDS + D.SEEDS_EXT + D.SEEDS_SCENE + D.SEEDS_CONTACT}
    for name, (_, seeds, split) in D.VARIANTS.items():
        for seed in seeds + D.VARIANTS_EXT[name] + (D.VARIANTS_SCENE[name], D.VARIANTS_CONTACT[name]):
            out[name, seed] = dry_run(mrs, seed, split=split)
    return out


def is_ext(key):
    """the sequences that draw the kinds of the extended surface: its own, and those of the scene and the contact surface"""
    return D.surface_of(key[1]) != "base"


def is_contact(key):
    return D.surface_of(key[1]) == "contact"


def is_scene(key):
    return D.surface_of(key[1]) == "scene"


def log_hashes(runs):
    import hashlib
    return {f"{variant},{seed}": hashlib.sha256(repr(r["log"]).encode()).hexdigest() for (variant, seed), r in runs.items()}


def golden(name):
    import json
    import os
    with open(os.path.join(helpers.ROOT, "tests", "golden", name)) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def base_runs(runs):
    return {k: r for k, r in runs.items() if not is_ext(k)}


@pytest.fixture(scope="module")
def ext_runs(runs):
    """the sequences of the extended surface that run in the parent process: D.SEEDS_EXT"""
    return {k: r for k, r in runs.items() if D.surface_of(k[1]) == "ext" and k[0] is None}


@pytest.fixture(scope="module")
def scene_runs(runs):
    """the sequences of the scene surface that run in the parent process: D.SEEDS_SCENE"""
    return {k: r for k, r in runs.items() if is_scene(k) and k[0] is None}


@pytest.fixture(scope="module")
def contact_runs(runs):
    """the sequences of the contact surface that run in the parent process: D.SEEDS_CONTACT"""
    return {k: r for k, r in runs.items() if is_contact(k) and k[0] is None}


def test_step_cap_is_the_largest_total_of_the_existing_sequences(mrs):
    totals = []
    for seed, fast, fleet in E.SEEDS:
        p = D.StubPair(mrs, 150)
        totals.append(E.drive(p, mrs, O, np.random.default_rng(1000 + seed), 150, seed, fast, fleet, 0.0, compare=False))
        assert "step_n" in p.g.calls and "tick_n" in p.g.calls
    print(f"test_random_sequences_gpu.py: steps per seed {totals}")
    assert max(totals) == D.STEP_CAP and min(totals) == 39


def test_every_sequence_keeps_the_step_budget(runs):
    for key, r in runs.items():
        assert r["steps"] <= D.STEP_CAP, (key, r["steps"])
    print("steps per sequence:", {k: r["steps"] for k, r in runs.items()})
    assert max(r["steps"] for r in runs.values()) == 76  # (the figure of the GPU module's docstring)
    for seed, _, _, long_rollout, _ in D.SEEDS:  # the long rollout happened, and left room for nothing but the compares
        longs = [e for e in runs[None, seed]["log"] if len(e) > 4 and e[5] == D.LONG_HORIZON]
        assert len(longs) == int(long_rollout), (seed, longs)
    for seed, _, _, long_rollout, _, _ in D.SEEDS_EXT:  # ... and on the extended surface it is a tick rollout that takes it
        longs = [e[1] for e in runs[None, seed]["log"] if len(e) > 5 and e[5] == D.LONG_HORIZON]
        assert len(longs) == int(long_rollout) and all(name in [D.OP_NAMES[op] for op in D.TICK_ROLLOUTS] for name in longs), (seed, longs)
    assert sum(f[3] for f in D.SEEDS_EXT) == 1


def test_every_op_kind_occurs(base_runs):
    runs = base_runs
    kinds = sum((r["kinds"] for (variant, _), r in runs.items() if variant is None), D.Counter())
    for op in range(D.N_OPS + 2):
        assert kinds[op] >= 5, f"{D.OP_NAMES[op]} occurs {kinds[op]} times over all seeds"
    assert not any(kinds[op] for op in D.EXT_KINDS), "the first surface draws what it always drew"
    # all four entry points of the rollouts take the long horizon once, both dtypes occur, and so do the tensor calls of every kind
    names = [c[0] for r in runs.values() for c in r["calls"]]
    for name in ("set_input", "apply_force", "gather", "crashed", "reset", "save_load", "clone", "nearest", "rollout", "rollout_cost", "async_issue",
                 "async_wait"):
        assert names.count(name) >= 5, name
    assert sum(r["rollouts_behind_pending"] for r in runs.values()) >= 3
    for variant, (_, seeds, split) in D.VARIANTS.items():
        for s in seeds:  # host call 12 occurs in every sequence of the split variants (there in runs of 5 .. 7 launches)
            assert not split or runs[variant, s]["kinds"][12] >= 1, (variant, s)
        assert {D.SEEDS[s][2] for s in seeds} == {"x500", "mixed"}, variant


def test_the_first_surface_draws_what_it_always_drew(base_runs):
    """the op logs of the 28 seeds and the three variants, as they were before the extended surface existed: SHA-256 of repr(log)"""
    assert log_hashes(base_runs) == golden("device_sequence_logs.json")


def test_the_extended_surface_draws_what_it_drew_before_the_scene_surface(runs):
    """the op logs of the 20 extended seeds and their six variant runs, as they were before the scene surface existed"""
    ext = {k: r for k, r in runs.items() if D.surface_of(k[1]) == "ext"}
    assert len(ext) == len(D.SEEDS_EXT) + sum(len(v) for v in D.VARIANTS_EXT.values())
    assert log_hashes(ext) == golden("device_sequence_logs_ext.json")


def test_the_scene_surface_draws_what_it_drew_before_the_contact_surface(runs):
    """the op logs of the 12 scene seeds and their three variant runs, as they were before the contact surface existed"""
    scene = {k: r for k, r in runs.items() if is_scene(k)}
    assert len(scene) == len(D.SEEDS_SCENE) + len(D.VARIANTS_SCENE)
    assert all(D.surface_of(s) == "scene" for s in range(200, 400)), "the variant seeds 310 and 317 stay scene seeds"
    assert log_hashes(scene) == golden("device_sequence_logs_scene.json")


def test_every_kind_of_the_extended_surface_occurs(runs, ext_runs):
    """the counts of the module docstrings, over D.SEEDS_EXT"""
    assert len(ext_runs) == len(D.SEEDS_EXT) >= 15 and min(D.EXT_SEED_NUMBERS) > len(D.SEEDS)
    assert 3 * sum(f[5] for f in D.SEEDS_EXT) >= len(D.SEEDS_EXT), "at least a third of the seeds carry world labels"
    kinds = sum((r["kinds"] for r in ext_runs.values()), D.Counter())
    print("extended surface, calls per kind:", {D.OP_NAMES[op]: kinds[op] for op in D.EXT_KINDS}, "steps:", [r["steps"] for r in ext_runs.values()])
    for op in D.EXT_KINDS:
        assert kinds[op] >= 5, f"{D.OP_NAMES[op]} occurs {kinds[op]} times over the seeds of the extended surface"
    calls = [c for r in ext_runs.values() for c in r["calls"]]
    by_name = {name: [c for c in calls if c[0] == name] for name in ("rollout_ticks", "rollout_tick_cost", "rollout_feedback", "rollout_tick_feedback",
                                                                     "proximity_cost", "set_worlds")}
    for name, cs in by_name.items():
        assert len(cs) >= 5, (name, len(cs))
    # crash mode and groups == 0 in the tick rollouts; both gain layouts, a gain block per command block, every cost form
    assert any(c[7] for c in by_name["rollout_ticks"]) and any(c[4] == 0 for c in by_name["rollout_ticks"])
    assert {c[9] for c in by_name["rollout_ticks"]} == {"bool", "uint8", None}
    assert any(c[9] for c in by_name["rollout_tick_cost"]) and any(c[4] == 0 for c in by_name["rollout_tick_cost"])
    fb = by_name["rollout_feedback"] + by_name["rollout_tick_feedback"]
    assert {len(c[5]) for c in fb} == {3, 4}, "shared and per-UAV gains"
    assert any(c[5][0] == c[2][0] > 1 for c in fb), "Bg = B"
    assert any(c[6][1] == 1 for c in fb) and any(c[6][1] > 1 for c in fb), "shared and per-UAV setpoints"
    assert {(c[7] != 0, c[12]) for c in by_name["rollout_feedback"]} == {(True, True), (False, False)}
    assert {(c[7] != 0, c[12]) for c in by_name["rollout_tick_feedback"]} == {(True, True), (False, False), (False, True)}
    assert any(c[10][0] for c in by_name["rollout_tick_feedback"]), "crash mode under feedback"
    assert {c[3] for c in by_name["proximity_cost"]} == {0, 1, 2} and any(c[1] == 32 for c in by_name["proximity_cost"])
    assert {c[8] for c in by_name["proximity_cost"]} == {False, True} == {c[9] for c in by_name["proximity_cost"]}
    # both world-setting paths, and only where the seed says so
    for (_, seed), r in ext_runs.items():
        worlds = D.ext_flags(seed)[5]
        assert (r["kinds"][D.SET_WORLDS] > 0) <= worlds and ("set_worlds" in r["product_calls"]) == worlds, seed
    assert sum(r["world_sets"][0] for r in ext_runs.values()) >= 2 and sum(r["world_sets"][1] for r in ext_runs.values()) >= 2
    assert sum("set_worlds" == c[0] for c in calls) == sum(r["world_sets"][1] for r in ext_runs.values())
    # what the hooks are for
    assert sum(r["ext_rollouts_behind_pending"] for r in ext_runs.values()) >= 3
    assert sum(r["proximity_behind_pending"] for r in ext_runs.values()) >= 3
    assert sum(r["measured_tick_rollouts"] for r in ext_runs.values()) >= 5
    # the child-process variants: two seeds each, one per fleet and one of them with worlds; host call 12 where step_n is split
    for variant, (_, _, split) in D.VARIANTS.items():
        seeds = D.VARIANTS_EXT[variant]
        assert len(seeds) == 2 and {D.ext_flags(s)[2] for s in seeds} == {"x500", "mixed"} and sum(D.ext_flags(s)[5] for s in seeds) == 1, variant
        for s in seeds:
            assert not split or runs[variant, s]["kinds"][12] >= 1, (variant, s)
            assert sum(runs[variant, s]["kinds"][op] for op in D.ROLLOUTS_EXT[4:]) >= 2, (variant, s)


def test_every_kind_of_the_scene_surface_occurs(runs, scene_runs):
    """the counts of the module docstrings, over D.SEEDS_SCENE: D.SCENE_COUNTS exactly, and what the seeds were chosen to show"""
    flags = D.SEEDS_SCENE
    assert len(scene_runs) == len(flags) == 12 and min(D.SCENE_SEED_NUMBERS) >= 200
    assert 3 * sum(f[5] for f in flags) >= len(flags), "at least a third of the seeds carry world labels"
    assert {f[1] for f in flags} == {False, True} and {f[2] for f in flags} == {"x500", "mixed"} and {f[0] % 2 for f in flags} == {0, 1}
    total = D.scene_totals(scene_runs.values())
    print("scene surface:", total)
    assert total == D.SCENE_COUNTS
    for op in D.SCENE_KINDS:
        assert total[D.OP_NAMES[op]] >= 8, f"{D.OP_NAMES[op]} occurs {total[D.OP_NAMES[op]]} times over the seeds of the scene surface"
    assert total["scene_behind_pending"] >= 3
    for mark in D.SCAN_MARKS.values():
        assert total["scan_after_" + mark] >= 5, mark
    assert total["stale_table_shapes"] >= 3
    for name in ("hit_sphere", "hit_box", "hit_cylinder", "hit_uav", "hit_ground", "hit_none", "range_zero", "uav_takes_from_obstacle",
                 "obstacle_keeps_from_uav", "found_over_k", "query_grid_builds", "query_cache_hits", "scan_grid_builds", "scan_cache_hits"):
        assert total[name] >= 1, name
    calls = [c for r in scene_runs.values() for c in r["calls"]]
    by_name = {name: [c for c in calls if c[0] == name] for name in ("set_obstacles", "set_scan_beams", "nearest_obstacles", "obstacle_cost",
                                                                     "range_scan", "range_scan_uavs")}
    # each set through the host call and through the tensor call; every size of a set and of a pattern
    assert {c[2] for c in by_name["set_obstacles"]} == {False, True} == {c[2] for c in by_name["set_scan_beams"]}
    assert {c[1] for c in by_name["set_obstacles"]} == set(D.OBSTACLE_COUNTS) and {c[1] for c in by_name["set_scan_beams"]} == set(D.BEAM_COUNTS) | {9}
    # queries: both dtypes, k = 32, rows present and absent, every radius; costs: both kinds, a start vector or none, found or not
    q = by_name["nearest_obstacles"]
    assert {c[6] for c in q} == {False, True} and {c[3] != 0 for c in q} == {False, True} and any(c[1] == 32 for c in q)
    assert {c[2] for c in q + by_name["obstacle_cost"]} == set(D.PALETTE) and any(max(c[7]) > 0 for c in q)
    c = by_name["obstacle_cost"]
    assert {v[3] for v in c} == {0, 2} and {v[7] for v in c} == {False, True} == {v[8] for v in c} and any(v[1] == 32 for v in c)
    # scans: both dtypes, both frames, the ground on and off, every range, hits and UAV indices present and absent
    for name in ("range_scan", "range_scan_uavs"):
        s = by_name[name]
        assert {v[5] for v in s} == {False, True} and {v[2] for v in s} == {0, 1, 2, 3} and {v[1] for v in s} == set(D.PALETTE), name
        assert {v[8] for v in s} == {False, True} and any(max(v[7]) > 0 for v in s), name
    assert {v[9] for v in by_name["range_scan_uavs"]} == {False, True} and not any(v[9] for v in by_name["range_scan"])
    assert any(v[6] == 65 for v in by_name["range_scan_uavs"]), "a second beam group with one live lane"
    # the child-process variants: one seed each; host call 12 where step_n is split
    assert sorted(D.VARIANTS_SCENE) == sorted(D.VARIANTS)
    for variant, (_, _, split) in D.VARIANTS.items():
        r = runs[variant, D.VARIANTS_SCENE[variant]]
        assert not split or r["kinds"][12] >= 1, variant
        assert sum(r["kinds"][op] for op in D.SCANS) >= 2 and sum(r["kinds"][op] for op in D.SCENE_KINDS) >= 6, variant


def test_every_kind_of_the_contact_surface_occurs(runs, contact_runs):
    """the counts of the module docstrings, over D.SEEDS_CONTACT: D.CONTACT_COUNTS exactly, and the conditions the seeds were chosen to
    keep (conditions, not measurements: a seed that breaks one is replaced by another candidate)"""
    flags = D.SEEDS_CONTACT
    assert len(contact_runs) == len(flags) == 12 and min(D.CONTACT_SEED_NUMBERS) >= 400
    assert sum(f[5] for f in flags) >= 6 and sum(f[4] for f in flags) >= 2, "at least six seeds with worlds, two with model-only phases"
    assert {f[1] for f in flags} == {False, True} and {f[2] for f in flags} == {"x500", "mixed"} and {f[0] % 2 for f in flags} == {0, 1}
    assert not any(f[3] for f in flags), "none takes the long horizon"
    total = D.contact_totals(contact_runs.values())
    print("contact surface:", total)
    print("contact surface, the scene kinds along the way:", D.scene_totals(contact_runs.values()))
    assert total == D.CONTACT_COUNTS
    assert total["obstacle_contacts"] >= 20 and total["contact_mark"] >= 20
    assert total["contacts_behind_pending"] >= 5 and total["marks_behind_pending"] >= 5
    assert total["marks_behind_stall"] >= 2 and total["marks_with_open_ticket"] >= 2
    assert total["uavs_newly_marked"] >= 40 and total["marked_seen_in_crash_row"] >= 5 and total["marks_of_nobody"] >= 1
    assert total["uavs_touching"] >= total["uavs_newly_marked"] and total["uavs_touching_several"] >= 1
    for mark in D.SCAN_MARKS.values():
        assert total["contact_after_" + mark] >= 1, mark
    assert total["contact_cache_hits"] >= 3 and total["contact_grid_builds"] >= 10
    for (_, seed), r in contact_runs.items():  # the sequence stays a test of flying UAVs
        assert 2 * r["crashed_at_end"] <= D.N_UAVS, (seed, r["crashed_at_end"])
    # the calls as drawn: every margin of each form, every output alone or with others, vectors to fill and new ones, a cost or none,
    # a mark with no output at all, and the scene kinds still drawn beside them
    calls = [c for r in contact_runs.values() for c in r["calls"] if c[0] == "obstacle_contacts"]
    assert len(calls) == total["obstacle_contacts"] + total["contact_mark"]
    plain, marks = [c for c in calls if not c[2]], [c for c in calls if c[2]]
    assert {c[1] for c in plain} == set(D.MARGINS) and {c[1] for c in marks} == set(D.MARK_MARGINS) == {0.0, 0.25}
    assert all(c[5] or c[7] for c in plain), "the read-only form always asks for something"
    assert any(not c[5] and not c[7] for c in marks), "the mark alone"
    for form in (plain, marks):
        assert {name for c in form for name in c[5]} == set(D.CONTACT_OUTPUTS)
        assert {c[6] for c in form} == {False, True} == {c[7] for c in form}
    kinds = sum((r["kinds"] for r in contact_runs.values()), D.Counter())
    for op in D.SCENE_KINDS + D.EXT_KINDS[:5]:
        assert kinds[op] >= 5, f"{D.OP_NAMES[op]} occurs {kinds[op]} times over the seeds of the contact surface"
    # the forced shapes, read from the op logs: a tick rollout right behind a mark, a contact call right behind a table-changing call
    names = [[e[1] for e in r["log"]] for r in contact_runs.values()]
    pairs = D.Counter((a, b) for seq in names for a, b in zip(seq, seq[1:]))
    assert sum(pairs["contact_mark", b] for b in ("rollout_ticks", "rollout_tick_cost")) >= 3
    assert sum(pairs[a, b] for a in D.TABLE_CALLS.values() for b in ("obstacle_contacts", "contact_mark")) >= 3
    assert sum(pairs[a, "contact_mark"] for a in ("async_outputs", "async_poses")) >= 2
    # the child-process variants: one seed each; host call 12 where step_n is split; both forms, and somebody marked
    assert sorted(D.VARIANTS_CONTACT) == sorted(D.VARIANTS)
    for variant, (_, _, split) in D.VARIANTS.items():
        r = runs[variant, D.VARIANTS_CONTACT[variant]]
        assert not split or r["kinds"][12] >= 1, variant
        assert r["kinds"][D.OBSTACLE_CONTACTS] >= 1 and r["kinds"][D.CONTACT_MARK] >= 4 and r["scene"]["uavs_newly_marked"] >= 5, variant
        assert 2 * r["crashed_at_end"] <= D.N_UAVS, variant


def test_the_extended_seeds_keep_their_comparison_honest(runs):
    """the two conditions of device_sequences' docstring, for every sequence of the extended surface: no same-world pair within twice the
    compare's reach of its contact threshold at any collision pass, and no UAV near a branch boundary of the quaternion where a
    feedback reads it.  A seed that breaks one is replaced by another (D.EXT_SEED_NUMBERS); no tolerance moves."""
    passes = 0
    for key, r in runs.items():
        if is_ext(key):
            assert r["contact_violations"] == 0, (key, r["contact_violations"])
            assert r["feedback_near_quat_branch"] == 0, (key, r["feedback_near_quat_branch"])
            passes += sum(r["kinds"][op] for op in (13, 14, D.TICK_LONG) + D.TICK_ROLLOUTS)
    assert passes >= 100


def test_the_contact_seeds_keep_their_marks_honest(runs):
    """the third condition, for every sequence of the contact surface: at no marking call is an applicable (UAV, obstacle) pair of the
    range within 2 sqrt(3) delta of its threshold (D.obstacle_contact_violations), so the product's touching set is the oracle's"""
    marks = 0
    for key, r in runs.items():
        assert r["obstacle_contact_violations"] == 0, (key, r["obstacle_contact_violations"])
        marks += r["kinds"][D.CONTACT_MARK] if is_contact(key) else 0
        assert is_contact(key) or not (r["kinds"][D.CONTACT_MARK] or r["kinds"][D.OBSTACLE_CONTACTS]), "the earlier surfaces draw no contact call"
    assert marks >= 30


def test_obstacle_contact_violations_counts_pairs_near_their_threshold(oracle):
    from test_obstacles import ALL_WORLDS, BOX, SPHERE, obstacles
    o = oracle.OracleSwarm(4)
    o.construct(0, 4, helpers.oracle_params("x500"))
    par = o.get_params(0)
    rad = par.arm_length + par.prop_radius
    st = o.get_state()
    ob = obstacles([(SPHERE, (0.0, 0.0, 5.0), (1.0, 0, 0), 0), (BOX, (40.0, 0.0, 5.0), (1.0, 1.0, 1.0), 7)])

    def at(sd, world=0):  # UAV 0 at signed distance sd from the sphere, along x; UAV 1 as far from the box of world 7; the others far away
        x = np.array([[1.0 + sd, 0.0, 5.0], [41.0 + sd, 0.0, 5.0], [0.0, 80.0, 5.0], [0.0, 90.0, 5.0]])
        o.set_state(0, 4, x, st["v"], st["R"], st["omega"], st["motor_rpm"])
        o.set_worlds([0, world, 0, 0])
    margin = 0.25
    thr = rad + margin
    reach = np.sqrt(3.0) * 1e-7 * 5.0  # sqrt(3) delta, delta = rtol * |x|_inf of UAV 0
    for off, want in ((0.0, 1), (1.5 * reach, 1), (-1.5 * reach, 1), (3.0 * reach, 0), (-3.0 * reach, 0)):
        at(thr + off)
        assert D.obstacle_contact_violations(o, ob, rad, margin, 0, 4, 1e-7) == want, off
        assert D.obstacle_contact_violations(o, ob, rad, margin, 0, 4, 1e-11) == (1 if off == 0.0 else 0), off
        assert D.obstacle_contact_violations(o, ob, rad, margin, 1, 3, 1e-7) == 0, "UAV 0 is outside the range"
        assert D.obstacle_contact_violations(o, ob, rad, 0.0, 0, 4, 1e-7) == 0, "another margin, another threshold"
    at(thr, world=7)  # the box applies to UAV 1 now; its |x|_inf is 41, so its reach is larger
    assert D.obstacle_contact_violations(o, ob, rad, margin, 0, 4, 1e-7) == 2
    assert D.obstacle_contact_violations(o, ob, np.full(4, rad), margin, 1, 1, 1e-7) == 1, "per-UAV radii"
    ob["flags"][1] = ALL_WORLDS
    at(thr)
    assert D.obstacle_contact_violations(o, ob, rad, margin, 0, 4, 1e-7) == 2, "an ALL_WORLDS obstacle applies whatever the label"
    assert D.obstacle_contact_violations(o, ob[:0], rad, margin, 0, 4, 1e-7) == 0


def test_contact_violations_counts_pairs_near_their_threshold(oracle):
    o = oracle.OracleSwarm(4)
    o.construct(0, 4, helpers.oracle_params("x500"))
    par = o.get_params(0)
    crit = 2.0 * (par.arm_length + par.prop_radius)
    st = o.get_state()

    def at(d2, far=50.0):
        x = np.array([[0.0, 0.0, 5.0], [np.sqrt(d2), 0.0, 5.0], [far, 0.0, 5.0], [far, 3.0, 5.0]])
        o.set_state(0, 4, x, st["v"], st["R"], st["omega"], st["motor_rpm"])
    reach = 2.0 * np.sqrt(crit) * 2.0 * 1e-7 * 5.0  # 2 d (delta_i + delta_j), delta = rtol * |x|_inf
    for off, want in ((0.0, 1), (1.5 * reach, 1), (-1.5 * reach, 1), (3.0 * reach, 0), (-3.0 * reach, 0)):
        at(crit + off)
        assert D.contact_violations(o, 1e-7) == want, off
        assert D.contact_violations(o, 1e-11) == (1 if off == 0.0 else 0), off
    at(crit)
    o.set_worlds([0, 1, 0, 0])
    assert D.contact_violations(o, 1e-7) == 0, "UAVs of two worlds do not meet"


def test_fast_uavs_are_followed_by_ticks_and_calls_that_replay_them(runs):
    n, seen, followers = 0, set(), [D.OP_NAMES[op] for op in D.STALL_FOLLOWERS]
    stallers = D.Counter()
    for key, r in runs.items():
        names = [e[1] for e in r["log"]]
        ticks = ["tick_long"] + ([D.OP_NAMES[op] for op in D.STALL_ROLLOUTS] if is_ext(key) else [])
        for i, name in enumerate(names[:-3]):
            if name == "fast_uavs" and names[i + 1] in ticks:
                allowed = followers + (["contact_mark"] if is_contact(key) else [])  # (the mark that has to replay the stall)
                assert names[i + 2] in allowed and names[i + 3] in allowed
                if names[i + 1] != "tick_long":
                    assert r["log"][i + 1][5] >= 4, "a stall needs a run of ticks"
                    stallers[names[i + 1]] += int(key[0] is None)  # (over D.SEEDS_EXT: the variants repeat some of them)
                elif not is_ext(key):
                    n += 1
                    seen.update(names[i + 2:i + 4])
    assert n >= 10 and seen == set(followers), (n, seen)
    assert all(stallers[D.OP_NAMES[op]] >= 3 for op in D.STALL_ROLLOUTS), stallers


def test_the_oracle_stays_usable(runs):
    for key, r in runs.items():
        assert r["non_finite_uavs"] <= D.N_UAVS // 10, (key, r["non_finite_uavs"])
        assert r["worst_cost_ratio"] <= 1e-3, (key, r["worst_cost_ratio"])
    assert max(r["worst_cost_ratio"] for r in runs.values()) > 0.0  # (costs were evaluated at all)


# ---- the reference rows ------------------------------------------------------------------------------------------------------------

def eigen_quaternion(R):
    """Eigen::Quaterniond(Matrix3d), (x, y, z, w), and the branch taken: 3 for a positive trace, else the index of the largest diagonal entry"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[:3] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
        return q, 3
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3], q[j], q[k] = (R[k, j] - R[j, k]) * t, (R[j, i] + R[i, j]) * t, (R[k, i] + R[i, k]) * t
    return q, i


@pytest.mark.parametrize("airframe", ["x500", "f550"])
def test_reference_rows_against_the_independent_model(airframe):
    from test_independent_restatement import make_pair
    rng = np.random.default_rng(77)
    o, u, po = make_pair(O, airframe, rng, ground_enabled=True, ground_z=0.0)
    nm = int(po.n_motors)
    st = helpers.random_state(rng, 1, nm, tilted=True)
    o.set_state(0, 1, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    u.x, u.v, u.R, u.omega, u.motor_rpm = st["x"][0].copy(), st["v"][0].copy(), st["R"][0].copy(), st["omega"][0].copy(), st["motor_rpm"][0][:nm].copy()
    cmd = np.concatenate([rng.uniform(-2, 2, 3), rng.uniform(-1, 1, 1)])
    o.set_input(0, 1, O.VELOCITY_HDG_CMD, cmd[None, :])
    u.set_input(IM.VELOCITY_HDG_CMD, cmd)
    for _ in range(40):
        o.step(0.001)
        u.make_step(0.001)
    rows, R = D.ref_rows(o, 0, 1, 0xFF)
    assert rows.shape == (1, 36) == (1, D.gather_width(0xFF)) and R.shape == (1, 3, 3)
    q, _ = eigen_quaternion(u.R)
    want = np.concatenate([u.x, u.v, u.R.T @ u.v, u.R.reshape(9), q, u.omega, u.imu, u.motor_rpm, np.zeros(8 - nm)])
    assert np.abs(u.imu).max() > 0 and np.abs(u.omega).max() > 0
    scale = np.maximum(np.abs(want), D.group_floors(0xFF))
    assert (np.abs(rows[0] - want) / scale).max() <= 1e-9
    # a subset of the groups: bit order, the columns of the full row
    sub, _ = D.ref_rows(o, 0, 1, 0x91)  # POS | QUAT | RPM
    assert np.array_equal(sub[0], np.concatenate([rows[0, 0:3], rows[0, 18:22], rows[0, 28:36]]))
    assert D.gather_width(0x91) == 15 and len(D.group_floors(0x91)) == 15


def test_reference_quaternions_take_all_four_branches():
    from scipy.spatial.transform import Rotation
    from test_pose_payload_gpu import rotations
    rng = np.random.default_rng(5)
    n = 64
    o = O.OracleSwarm(n)
    o.construct(0, n, helpers.oracle_params("x500"))
    Rs = rotations(rng, n)
    st = helpers.random_state(rng, n, 4)
    o.set_state(0, n, st["x"], st["v"], Rs, st["omega"], st["motor_rpm"])
    rows, R = D.ref_rows(o, 0, n, 1 << D.QUAT_BIT)
    assert np.array_equal(R, Rs)
    branches = set()
    for i in range(n):
        q, branch = eigen_quaternion(Rs[i])
        branches.add(branch)
        assert np.abs(rows[i] - q).max() <= 4e-16, i
        ref = Rotation.from_matrix(Rs[i]).as_quat()
        assert min(np.abs(rows[i] - ref).max(), np.abs(rows[i] + ref).max()) <= 1e-12, i
    assert branches == {0, 1, 2, 3}


def test_branch_boundaries_of_the_quaternion():
    from scipy.spatial.transform import Rotation
    third = Rotation.from_rotvec(np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0) * (2.0 * np.pi / 3.0)).as_matrix()  # trace 0
    half_xy = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])  # half a turn about (1, 1, 0): R00 == R11 are the largest
    cases = [(np.eye(3), False), (np.diag([1.0, -1.0, -1.0]), False), (third, True), (half_xy, True),
             (Rotation.from_rotvec([0.3, -0.2, 2.0]).as_matrix(), False)]
    got = D.near_quat_branch(np.array([c[0] for c in cases]))
    assert list(got) == [c[1] for c in cases]
    # a quaternion of the other sign passes at a boundary and nowhere else
    q = np.array([[0.5, 0.5, 0.5, 0.5]])
    assert D.compare_rows(-q, q, third[None], 1 << D.QUAT_BIT, 1e-11, False, "boundary") == 1
    with pytest.raises(AssertionError, match="quat"):
        D.compare_rows(-q, q, np.eye(3)[None], 1 << D.QUAT_BIT, 1e-11, False, "no boundary")


def test_compare_rows_measures_every_group_on_its_own_scale():
    rng = np.random.default_rng(9)
    o = O.OracleSwarm(8)
    o.construct(0, 8, helpers.oracle_params("x500"))
    st = helpers.random_state(rng, 8, 4, tilted=True)
    o.set_state(0, 8, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    want, R = D.ref_rows(o, 0, 8, 0xFF)
    assert D.compare_rows(want.copy(), want, R, 0xFF, 1e-11, False, "same") == 0
    assert D.compare_rows(want.astype(np.float32), want, R, 0xFF, 1e-11, True, "one float rounding") == 0
    with pytest.raises(AssertionError):
        D.compare_rows(want.astype(np.float32), want, R, 0xFF, 1e-11, False, "FP32 rows at the FP64 tolerance")
    for col, name in ((1, "x"), (10, "R"), (23, "omega"), (30, "rpm")):
        off = want.copy()
        off[3, col] += 3e-11 * max(abs(want[3, col]), 1000.0 if name == "rpm" else 1.0) * 10
        with pytest.raises(AssertionError, match=name):
            D.compare_rows(off, want, R, 0xFF, 1e-11, False, "perturbed")
    off = want.copy()
    off[3, 30] += 5e-9  # far below the rpm group's scale, though above 1e-11 of a unit
    assert D.compare_rows(off, want, R, 0xFF, 1e-11, False, "rpm scale") == 0
    nan = want.copy()
    nan[2, 4] = np.nan
    with pytest.raises(AssertionError, match="NaN pattern"):
        D.compare_rows(nan, want, R, 0xFF, 1e-11, False, "NaN")


def test_cost_bound_covers_a_perturbation_of_the_rows():
    rng = np.random.default_rng(13)
    groups, rtol = 0x83, 1e-7  # POS | VEL | RPM
    w = D.gather_width(groups)
    rows = np.concatenate([rng.normal(0, 5, (4, 10, 6)), rng.uniform(2000, 5000, (4, 10, 8))], axis=2)
    targets = rows + rng.uniform(0.5, 3.0, rows.shape) * rng.choice([-1.0, 1.0], rows.shape) * D.group_floors(groups)
    for weights in (rng.uniform(0.1, 2.0, (4, w)), rng.uniform(0.1, 2.0, (1, w))):
        cost, bound = restate(rows, targets, weights), D.cost_bound(rows, targets, weights, groups, rtol)
        assert (bound > 0).all() and (bound <= 1e-3 * cost).all()
        delta = rtol * np.maximum(np.abs(rows), D.group_floors(groups))
        for sign in (rng.choice([-1.0, 1.0], rows.shape), np.sign(rows - targets)):
            moved = restate(rows + sign * delta, targets, weights)
            assert (np.abs(moved - cost) <= bound * (1 + 1e-9)).all()
        worst = restate(rows + np.sign(rows - targets) * delta, targets, weights)
        assert (np.abs(worst - cost) >= 0.99 * bound).all()  # the bound is attained, not generous
