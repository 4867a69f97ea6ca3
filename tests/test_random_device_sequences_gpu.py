"""Differential test of the device-resident call surface under random call sequences (tests/device_sequences.py): the frame of
test_random_sequences_gpu.py — about 150 UAVs in two fleets, dense enough to collide all the time, the ground enabled, both arithmetic
flavours, all 18 host calls of that module — with the device-resident calls mixed in: commands and forces from FP64 / FP32 rows with
padded strides, observation rows, crash flags, masked resets, snapshot round trips, clone swaps, nearest-neighbour rows, the four rollout
entry points (FP64 and FP32, held commands, strided observation / cost rows, force rows, once 66 steps), pipelined output and pose
downloads waited for one to six calls later, and UAVs made fast enough to stall the lazily evaluated collision ticks.  The last eight
seeds put the whole swarm under actuator commands every fifth call, so that the calls that follow meet the model-only step kernels and
have to move the launches back to the cascade kernels themselves.  The CPU oracle and
plain numpy are the only references: no twin product swarm.  State, PIDs, IMU, forces and crash flags are compared after every five
calls, observation rows per group on the group's own scale, costs against the first-order bound of their restatement.

Odd seeds run every tensor call under a torch stream of their own: the library's fences are then what orders the data.

Tolerances are those of test_random_sequences_gpu.py (RTOL_LITERAL, 1e-7 for FAST), which were set for its step totals: the largest of
its 24 sequences takes 76 steps, and no sequence here takes more (rollout steps included; the largest takes 76).
test_random_device_sequences.py counts both on the CPU and checks the generator against the oracle alone.

After the seeds, the counters of the library summed over them must show what the sequences are there for: a stall that was replayed, a
pipelined download re-issued by a replay and then waited for, a rollout behind a collision tick that was still pending.  Three variants
run in child processes (two seeds each, one per fleet): the two-stream form of step_n (MRS_SPLIT_MIN_BLOCKS=1: three blocks), the
pointer-addressed kernels (MRS_NO_BUFFER_ADDRESSING=1), and both.

The extended surface (device_sequences.SEEDS_EXT: 20 more seeds under test ids of their own, 8 of them with collision worlds, and two
more seeds per child-process variant, one per fleet and one of them with worlds) mixes in what came after: tensors.rollout_ticks,
rollout_tick_cost, rollout_feedback, rollout_tick_feedback and proximity_cost, and world labels set in the middle of a run that goes on
through list ticks, fused launches, nearest() and tick rollouts.  Over the 20 seeds (counted by test_random_device_sequences.py): 27
rollout_ticks, 27 rollout_tick_cost, 25 rollout_feedback, 35 rollout_tick_feedback, 49 proximity_cost and 13 set_worlds calls; the largest
sequence takes 76 steps, ticks of tick rollouts included, and one takes a tick rollout of 66 ticks.  The oracle runs the loops of the header
comments literally (set_input at block starts — from the feedback law restated in numpy where there is one —, step, rows and crash
flags at the evaluations, handle_collisions); rows are compared like gathered rows, crash rows exactly, the term of a cost within the
first-order bound of its rows and the crash cost exactly, a proximity cost bit for bit against numpy on the positions the product
holds.  Their counters must show a tick rollout that stalled and replayed a launch, a proximity cost and a rollout of the new kinds
behind a collision tick that was still pending.  The stall and replay counters of a tick rollout are read around the call, and those
reads evaluate a pending tick: the generator takes them where none is pending before the call, and treats none as pending behind it.

The scene surface (device_sequences.SEEDS_SCENE: 12 more seeds under test ids of their own, 8 of them with collision worlds, and one
more seed per child-process variant) mixes in the static obstacles and the range scans: set_obstacles, nearest_obstacles, obstacle_cost,
set_scan_beams, range_scan and range_scan_uavs, between calls that change what they read under them — set_ground_z, set_params,
set_mass and masked resets (the airframe table), set_obstacles (both grid cache entries), set_worlds (the kernel instantiation), clone
swaps (set, pattern and labels must travel).  Every query and scan is compared bit for bit with the numpy restatements on the
positions and attitudes gathered right before the call; grid_builds is asserted against a model of the two-entry cache after every
scene call; get_obstacles() and get_scan_beams() against the generator's copies at every compare.  Over the 12 dry runs (counted by
test_random_device_sequences.py on the oracle's state): 16 set_obstacles, 16 nearest_obstacles, 17 obstacle_cost, 18 set_scan_beams, 41
range_scan, 21 range_scan_uavs, 16 of them behind a pending tick; 10 stale-table shapes; beams taken by spheres 448, boxes 614,
cylinders 4862, UAVs 2594, the ground 2725, nothing 64699, 2398 of range 0; 66 a UAV takes from an obstacle, 63 an obstacle keeps from
a UAV; 65 query UAVs with found > k; 29 + 53 grids built, 4 + 9 cache hits.  This module counts the same figures from the restatement
of the product's own state and asserts each at about half (scene_floor).  A scene seed takes 0.1 to 0.2 s on an MI355X.

The contact surface (device_sequences.SEEDS_CONTACT: 12 more seeds under test ids of their own, 7 of them with collision worlds, and
one more seed per child-process variant) mixes in tensors.obstacle_contacts in both forms: the read-only one, which must leave a
pending collision tick pending, and the marking one (crash=True), the only scenery call that writes simulation state — it evaluates the
pending tick, ORs the crashed bit into the flag words, reads the airframe table it has just uploaded and makes a third grid cache
entry current.  Every requested vector (hit, index, sd, counts, the cost vector) is compared bit for bit with the numpy restatement on
the positions gathered around the call; the UAVs the product's positions touch must be the UAVs the oracle's positions touch (the
third honesty condition, asserted by the dry runs, makes that a fair demand), and those are crashed on the oracle, so that the next
crashed() call, the crash rows and crash costs of the tick rollouts forced behind a mark and the five-call compare see every mark.
Marks stand among the calls that have to replay a stalled run of ticks, behind pending ticks, behind table-changing calls, clone
swaps, set_worlds and set_obstacles, and between the issue and the wait of a pipelined download; grid_builds is asserted against the
three-entry cache model after every scene and contact call.  Over the 12 dry runs (device_sequences.CONTACT_COUNTS): 34 read-only and
59 marking calls, 12 and 13 of them behind a pending tick, 7 marks behind a stall recipe, 302 UAVs touching, 94 newly marked, 53 of
them seen in a later crash row, 27 marks of nobody, 66 grids built and 27 cache hits; this module asserts each at scene_floor, and
that a stall was replayed in these sequences (measured: every figure equals the dry runs'; 91 stalls, 135 replayed launches).  A
contact seed takes 0.1 to 0.3 s on an MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from device_sequences import (CONTACT_COUNTS, N_UAVS, RNG_BASE, SCENE_COUNTS, SEEDS, SEEDS_CONTACT, SEEDS_EXT, SEEDS_SCENE, STEP_CAP, VARIANTS,
                              VARIANTS_CONTACT, VARIANTS_EXT, VARIANTS_SCENE, Device, contact_totals, ext_flags, run_sequence, scene_totals, seed_rtol,
                              surface_of)
from helpers import Pair

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CHILD_TIMEOUT = 300
STAT_NAMES = ("fused", "stalls", "replayed", "ahead", "packs", "reissued", "split_steps")
EXT_FIGURES = ("stalls_in_tick_rollouts", "replayed_in_tick_rollouts", "proximity_behind_pending", "ext_rollouts_behind_pending")

_results = {}  # seed -> what run_sequence returned (the seeds of the extended surface too: their numbers are their own)
_dead = []     # the first child process that died by a signal or timed out: nothing more is started on the GPU


def run_seed(mrs, seed, split=False):
    surface = surface_of(seed)
    _, fast, fleet, long_rollout, model, worlds = SEEDS[seed] + (False,) if surface == "base" else ext_flags(seed)
    p = Pair(mrs, N_UAVS, arith=mrs.ARITH_FAST if fast else mrs.ARITH_LITERAL)
    dev = Device(p, side=bool(seed % 2))
    res = run_sequence(p, dev, mrs, np.random.default_rng(RNG_BASE + seed), seed, fast, fleet, seed_rtol(fast), STEP_CAP, split=split,
                       long_rollout=long_rollout, model=model, surface=surface, worlds=worlds)
    assert p.g.get_diag() == p.o.get_diag()
    return res


def figures(res):
    st = dict(zip(STAT_NAMES, (int(v) for v in res["stats"])))
    return dict(steps=res["steps"], stalls=st["stalls"], replayed=st["replayed"], reissued=st["reissued"], tickets_waited=res["tickets_waited"],
                quat_sign_cases=res["quat_sign_cases"], rollouts_behind_pending=res["rollouts_behind_pending"], split_steps=st["split_steps"],
                fused=st["fused"], **{k: res[k] for k in EXT_FIGURES})


@pytest.mark.parametrize("seed,fast,fleet,long_rollout,model", SEEDS)
def test_random_device_sequences_match_oracle(mrs, seed, fast, fleet, long_rollout, model):
    res = run_seed(mrs, seed)
    print(f"seed {seed} ({'FAST' if fast else 'LITERAL'}, {fleet}): {figures(res)}")
    _results[seed] = res


@pytest.mark.parametrize("seed,fast,fleet,long_rollout,model,worlds", SEEDS_EXT)
def test_random_sequences_of_the_extended_surface_match_oracle(mrs, seed, fast, fleet, long_rollout, model, worlds):
    res = run_seed(mrs, seed)
    print(f"seed {seed} ({'FAST' if fast else 'LITERAL'}, {fleet}{', worlds' if worlds else ''}): {figures(res)}")
    _results[seed] = res


@pytest.mark.parametrize("seed,fast,fleet,long_rollout,model,worlds", SEEDS_SCENE)
def test_random_sequences_of_the_scene_surface_match_oracle_and_numpy(mrs, seed, fast, fleet, long_rollout, model, worlds):
    import time
    t0 = time.perf_counter()
    res = run_seed(mrs, seed)
    print(f"seed {seed} ({'FAST' if fast else 'LITERAL'}, {fleet}{', worlds' if worlds else ''}), {time.perf_counter() - t0:.1f} s: {figures(res)}\n"
          f"scene: {scene_totals([res])}")
    _results[seed] = res


@pytest.mark.parametrize("seed,fast,fleet,long_rollout,model,worlds", SEEDS_CONTACT)
def test_random_sequences_of_the_contact_surface_match_oracle_and_numpy(mrs, seed, fast, fleet, long_rollout, model, worlds):
    import time
    t0 = time.perf_counter()
    res = run_seed(mrs, seed)
    print(f"seed {seed} ({'FAST' if fast else 'LITERAL'}, {fleet}{', worlds' if worlds else ''}), {time.perf_counter() - t0:.1f} s: {figures(res)}\n"
          f"contact: {contact_totals([res])}")
    assert res["obstacle_contact_violations"] == 0, "no pair of a marking call is near its threshold on the oracle's positions"
    _results[seed] = res


def scene_floor(count):
    """what the GPU module asks of a figure that the CPU dry runs measured as `count`: about half (the restatement runs on the product's
    own state here, which differs from the oracle's within the compare's tolerance)"""
    return (count + 1) // 2


def test_the_sequences_met_what_they_are_for():
    n_seeds = len(SEEDS) + len(SEEDS_EXT) + len(SEEDS_SCENE) + len(SEEDS_CONTACT)
    assert len(_results) == n_seeds, f"only {len(_results)} of the {n_seeds} seeds ran to their end: this check speaks for all of them"
    first = [r for s, r in _results.items() if surface_of(s) == "base"]
    total = {k: sum(figures(r)[k] for r in first) for k in figures(first[0])}
    print(f"all seeds: {total}")
    assert total["stalls"] >= 1 and total["replayed"] >= 1, f"no stall of the lazy collision ticks was replayed: {total}"
    assert total["reissued"] >= 1 and total["tickets_waited"] >= 1, f"no pipelined download was re-issued by a replay and waited for: {total}"
    assert total["rollouts_behind_pending"] >= 1, f"no rollout followed a collision tick that was still pending: {total}"
    ext = [r for s, r in _results.items() if surface_of(s) == "ext"]
    total = {k: sum(figures(r)[k] for r in ext) for k in figures(ext[0])}
    print(f"the seeds of the extended surface: {total}")
    assert total["stalls_in_tick_rollouts"] >= 1 and total["replayed_in_tick_rollouts"] >= 1, f"no tick rollout stalled and replayed a launch: {total}"
    assert total["proximity_behind_pending"] >= 1, f"no proximity cost followed a collision tick that was still pending: {total}"
    assert total["ext_rollouts_behind_pending"] >= 1, f"no tick or feedback rollout followed a collision tick that was still pending: {total}"
    # the scene surface: every figure the CPU dry runs pinned (device_sequences.SCENE_COUNTS), here from the restatement of the product's state
    total = scene_totals(r for s, r in _results.items() if surface_of(s) == "scene")
    print(f"the seeds of the scene surface: {total}")
    assert sorted(total) == sorted(SCENE_COUNTS)
    for name, count in SCENE_COUNTS.items():
        assert total[name] >= scene_floor(count), f"{name}: {total[name]} over the scene seeds, the dry runs on the oracle counted {count}"
    # the contact surface: device_sequences.CONTACT_COUNTS likewise; and a stall of the lazy ticks was replayed in its sequences, where
    # marking calls stand among the calls that have to replay it
    contact = [r for s, r in _results.items() if surface_of(s) == "contact"]
    total = contact_totals(contact)
    print(f"the seeds of the contact surface: {total}; {({k: sum(figures(r)[k] for r in contact) for k in ('stalls', 'replayed')})}")
    assert sorted(total) == sorted(CONTACT_COUNTS)
    for name, count in CONTACT_COUNTS.items():
        assert total[name] >= scene_floor(count), f"{name}: {total[name]} over the contact seeds, the dry runs on the oracle counted {count}"
    assert sum(figures(r)["stalls"] for r in contact) >= 1 and sum(figures(r)["replayed"] for r in contact) >= 1, "no stall was replayed"


def child_main(out_path, variant):
    import mrs_multirotor_simulator_amd as M
    M.load_library()
    _, seeds, split = VARIANTS[variant]
    out = {}
    for seed in seeds + VARIANTS_EXT[variant] + (VARIANTS_SCENE[variant], VARIANTS_CONTACT[variant]):
        out[str(seed)] = figures(run_seed(M, seed, split=split))
        print(f"{variant}: seed {seed}: {out[str(seed)]}", flush=True)
    with open(out_path, "w") as f:
        json.dump(out, f)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variant_in_a_child_process(mrs, tmp_path, variant):
    if _dead:
        pytest.fail(f"an earlier child process of this module died ({_dead[0]}): no further GPU process is started")
    env_add, seeds, split = VARIANTS[variant]
    out = str(tmp_path / "variant.json")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MRS_")}
    env.update(env_add)
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import test_random_device_sequences_gpu as T; T.child_main({out!r}, {variant!r})"
    try:
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _dead.append(f"{variant} child timed out after {CHILD_TIMEOUT} s")
        pytest.fail(_dead[0])
    if p.returncode < 0:
        _dead.append(f"{variant} child ended by signal {-p.returncode}")
        pytest.fail(f"{_dead[0]}\n{p.stderr[-3000:]}")
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    with open(out) as f:
        got = json.load(f)
    assert sorted(got) == sorted(str(s) for s in seeds + VARIANTS_EXT[variant] + (VARIANTS_SCENE[variant], VARIANTS_CONTACT[variant]))
    for seed, fig in got.items():
        if split:  # the two-stream form was taken: steps launched as two half-swarm launches
            assert fig["split_steps"] >= 4, f"{variant}, seed {seed}: step_n never took the two-stream form: {fig}"
        else:
            assert fig["split_steps"] == 0, f"{variant}, seed {seed}: {fig}"
