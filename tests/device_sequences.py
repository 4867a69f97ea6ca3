"""Random call sequences over the whole call surface, the device-resident calls included (test_random_device_sequences*.py).

`run_sequence` is the frame of test_random_sequences_gpu.py (its fleets, its 18 host calls, its compare after every few calls) with the
device-resident calls of include/mrs_swarm.h mixed in: commands, forces, observation rows, crash flags, masked resets, snapshot round
trips, clone swaps, nearest-neighbour rows, the four rollout entry points and the pipelined downloads.  The oracle and plain numpy are
the only references.  The product is reached through a `Device` (torch tensors on the swarm's GPU) or a `Stub` that checks every argument
tuple against the header's rules and records it: the generator draws the same numbers for both, so the CPU test of the generator speaks
for the GPU test's sequences.

Steps are budgeted: a sequence never takes more than `cap` steps (rollout steps included), because the tolerances of the compare were
set for the step totals of test_random_sequences_gpu.py; a stepping call that no longer fits is drawn shorter or becomes a gather.

Two surfaces.  SEEDS and VARIANTS draw from the 33 kinds above and draw what they always drew.  SEEDS_EXT and VARIANTS_EXT
(run_sequence(surface="ext")) draw from 39: tensors.rollout_ticks, rollout_tick_cost, rollout_feedback, rollout_tick_feedback and
proximity_cost, and, in the seeds that carry the `worlds` flag, collision-world labels set in the middle of the run (the whole swarm is
labelled i % 3 before the first call, so that every collision pass, list tick, fused launch, nearest() and rollout of the sequence runs
the world-aware kernels).  Ticks of a tick rollout count as steps.  SEEDS_EXT holds 20 seeds, 8 of them with worlds; the largest takes 76
steps, and over all of them there are 27 rollout_ticks, 27 rollout_tick_cost, 25 rollout_feedback, 35 rollout_tick_feedback, 49
proximity_cost and 13 set_worlds calls (counted by test_random_device_sequences.py).  Two conditions keep the comparison of these seeds honest, and the
CPU dry run asserts both, so they are properties of the chosen seeds (contact_violations; near_quat_branch at the block starts of a
feedback on the quaternion).

A third surface.  SEEDS_SCENE and VARIANTS_SCENE (run_sequence(surface="scene"), seed numbers from 200 up, the flags of ext_flags) draw
from everything the extended surface draws plus six kinds: set_obstacles, nearest_obstacles, obstacle_cost, set_scan_beams, range_scan
and range_scan_uavs.  The oracle has neither obstacles nor beams: the generator keeps its own copies (draw_obstacles, draw_beams), sets
both before the first call, replaces them in the middle of the run (the host call and the tensor call in turn) and compares
get_obstacles() and get_scan_beams() with them, bit for bit, at every compare.  Each query and each scan is checked bit for bit
against the restatements of test_obstacles.py, test_range_scan.py and test_range_scan_uavs.py on what the call reads: the FP64
positions and attitudes of the whole swarm gathered right before it under the same stream context (a gather keeps a pending tick
pending; the dry run takes the oracle's), the oracle's labels, and ground_z and arm_length + prop_radius of the oracle's parameters.
Radius and max_range come from PALETTE.  All six kinds keep a pending collision tick pending; half of the time one of them is forced
where a proximity cost is forced on the extended surface.  Behind a call that re-interns airframe types (TABLE_CALLS) the generator
forces, half of the time, a range_scan without the ground flag and then a scan that reads the airframe table (the stale-table shape:
only the second uploads it); behind a clone swap, set_worlds and set_obstacles, a scan.
The grid cache is modelled as csrc/obstacle_set.h states it — two entries, the queries' keyed by radius and the scans' by max_range,
both dropped by set_obstacles — and obstacle_stats()["grid_builds"] (which takes the lock only) is asserted against the model after
every scene call.  What the header leaves open was read from csrc/obstacles.hip: set_obstacles itself builds nothing (it only marks
both entries); an empty set is built and cached like any other (ensure() does not look at the size, and both scans call it); a clone
adopts the set into an ObstacleSet of its own, so it starts with grid_builds == 0 and both entries empty (the clone of a swarm with an
empty set has no set at all until a call needs one); mrs_swarm_obstacle_stats describes the queries' entry only.  Code and header
agree.
Over the 12 seeds of SEEDS_SCENE, 8 of them with worlds (SCENE_COUNTS, asserted exactly by test_random_device_sequences.py): 16
set_obstacles, 16 nearest_obstacles, 17 obstacle_cost, 18 set_scan_beams, 41 range_scan and 21 range_scan_uavs calls, 16 of them behind
a pending tick; scans that follow a call with no other scan in between: 9 set_ground_z, 8 set_params, 7 resets, 8 clone swaps, 7
set_worlds, 12 set_obstacles; 10 stale-table shapes; beams taken by spheres 448, boxes 614, cylinders 4862, UAVs 2594, the ground 2725,
nothing 64699; 2398 beams of range 0; 66 beams a UAV takes from an obstacle and 63 an obstacle keeps from a UAV; 65 query UAVs with
found > k; grids built 29 (queries) and 53 (scans), cache hits 4 and 9.

A fourth surface.  SEEDS_CONTACT and VARIANTS_CONTACT (run_sequence(surface="contact"), seed numbers from 400 up — everything in
[200, 400) stays a scene seed —, the flags of ext_flags) draw from everything the scene surface draws plus two kinds, both
tensors.obstacle_contacts: OBSTACLE_CONTACTS, the read-only form, and CONTACT_MARK, the call with crash=True, the one scenery call that
writes simulation state.  Range as every call draws it; margin from test_obstacle_contacts.MARGINS, for the marking form from
MARK_MARGINS only (a margin of 1.0 would crash up to two thirds of the fleet); a random subset of hit / index / sd / counts, vectors to
fill and True in turn, never empty for the read-only form, and one mark in four asks for nothing at all; half of the time a cost
vector with a random hit_cost.  Every requested vector is compared bit for bit with restate_contacts and cost_after of
test_obstacle_contacts.py on the FP64 positions gathered right before the call (scene_inputs), the oracle's labels and arm_length +
prop_radius of the oracle's parameters.  Evaluating the pending tick moves no position: settle() drains — the same replay the gather
has already made — and runs collide_now, which reads positions and writes forces and flag words (tick_single.hip), so the gather
before a marking call sees what its kernel reads.  Behind the stall recipe the gather is made after the call instead (the mark writes
flag words only), so that the marking call itself is the one that meets the stalled log.
The oracle has no obstacles: the marking form crashes, on the oracle, the touching set of the restatement on the oracle's own
positions (o.crash() on its runs), and the product's set — the restatement on the product's positions — must be that set.  A third
honesty condition makes this a fair demand: signed distance is 1-Lipschitz in the position, positions that agree within delta_i = rtol
* max(|x_i|_inf, FIELD_FLOOR["x"]) per component move sd by at most sqrt(3) delta_i, and obstacle_contact_violations counts the
applicable pairs of a marking call's range with |sd - thr| < 2 sqrt(3) delta_i; the dry runs assert 0 for every contact seed.  After a
mark no tick is pending (the kind is not in KEEP_PENDING; the read-only kind is), and the next crashed() call, crash rows, crash costs
and the five-call compare see the marks.
Forced, each half of the time where it applies: a mark as one of the two followers of the FAST_UAVS recipe behind a run of ticks (the
stall is replayed before the mark, and no replayed launch may lose the marks); either form right behind a pending tick (13, 14,
ROLL_TICK); behind a mark that newly crashed somebody a ROLL_TICK or ROLL_TICK_COST whose range covers one of them, with the crash
rows asked for and a crash cost charged; a contact call behind TABLE_CALLS, a clone swap, set_worlds and set_obstacles (where the
scene surface forces a scan, in turn with it); a mark right behind an async download that is still open two calls later.
The cache model has a third entry, cache["contact"], keyed by fl(rmax + margin).  rmax is the maximum of arm_length + prop_radius over
the airframe table, which never forgets: intern_type only appends, index 0 is the default parameter set, upload_types sends the whole
table, and mrs_swarm_clone_resized copies keys and tparams whole while the clone's set starts with three empty entries and
grid_builds == 0.  The generator keeps the running maximum over the default set and the oracle's parameters after every call (a call
gives a UAV at most one new set); it never reads rmax back from the product.
Over the 12 seeds of SEEDS_CONTACT, 7 of them with worlds, 2 with model-only phases (CONTACT_COUNTS, asserted exactly by
test_random_device_sequences.py): 34 read-only and 59 marking calls, 12 and 13 of them behind a pending tick; 7 marks among the
followers of a stall recipe, 25 while a download was open; 302 UAVs touching, 44 of them more than one obstacle, 94 newly marked, 53
of those shown by the first crash row of a later tick rollout; 27 marks of nobody; contact calls that follow a call with no other
contact call in between: 8 set_ground_z, 10 set_params, 8 resets, 10 clone swaps, 5 set_worlds, 12 set_obstacles; 66 grids built for
the third entry, 27 cache hits.  No seed ends with more than half of its UAVs crashed."""
import contextlib
from collections import Counter

import numpy as np

import helpers
from helpers import FIELD_FLOOR, Pair
from oracle import oracle_swarm as O
from test_device_io_gpu import _runs
from test_nearest_gpu import compare_with_numpy
from test_obstacle_contacts import MARGINS, cost_after, restate_contacts
from test_obstacles import ALL_WORLDS, CYLINDER, OBSTACLE, restate_cost, restate_obstacles, restate_rows, signed_distances
from test_obstacles import add_bits as obstacle_add_bits
from test_obstacles import same_bits as same_typed_bits
from test_proximity_cost import add_bits, proximity_ref, same_bits
from test_random_sequences_gpu import DT, build_fleet, check, compare_outputs, host_op, payload, rng_range
from test_range_scan import BODY_FRAME, GROUND, HIT_GROUND, HIT_NONE, MAX_BEAMS, mixed_beams, restate_scan
from test_range_scan_uavs import HIT_UAV, NO_OBSTACLES, restate_scan_uavs
from test_rollout_cost_gpu import restate
from test_rollout_feedback_gpu import restate_feedback
from test_rollout_tick_cost_gpu import restate_ticks

N_UAVS = 150
N_ITER = 50        # calls of a sequence
N_ITER_LONG = 25   # ... of one whose rollout of LONG_HORIZON steps uses the step budget up
# observation groups in bit order: (name, width, the field of helpers.FIELD_FLOOR whose floor the group takes)
GROUPS = (("x", 3, "x"), ("v", 3, "v"), ("velocity_body", 3, "v"), ("R", 9, "R"), ("quat", 4, "R"), ("omega", 3, "omega"), ("imu", 3, "imu"),
          ("rpm", 8, "motor_rpm"))
QUAT_BIT = 4
WIDTH = {0: 0, 1: 8, 2: 4, 3: 4, 4: 10, 5: 5, 6: 4, 7: 4, 8: 4, 9: 4, 10: 4}  # command columns per mode (ACTUATOR: 8 serve every airframe)
HORIZONS = (1, 5, 12, 24)
LONG_HORIZON = 66  # kRolloutMaxSteps + 2: one step-kernel launch past the cap
BRANCH_EPS = 1e-9

# op kinds: 0 .. 17 are the host calls of test_random_sequences_gpu.host_op
(DEV_SET_INPUT, DEV_FORCE, GATHER, CRASHED, RESET, SNAPSHOT, CLONE, NEAREST, ROLL_PLAIN, ROLL_RATE, ROLL_FORCE, ROLL_COST, ASYNC_OUTPUTS, ASYNC_POSES,
 FAST_UAVS) = range(18, 33)
N_OPS = 33
TICK_LONG = 33  # never drawn: the run of ticks that follows FAST_UAVS
MODEL_ALL = 34  # never drawn: ACTUATOR_CMD for the whole swarm, which puts the step launches on the model-only kernels
OP_NAMES = {**{k: f"host{k}" for k in range(18)}, DEV_SET_INPUT: "dev_set_input", DEV_FORCE: "dev_force", GATHER: "gather", CRASHED: "crashed",
            RESET: "reset", SNAPSHOT: "snapshot", CLONE: "clone", NEAREST: "nearest", ROLL_PLAIN: "rollout", ROLL_RATE: "rollout_rate",
            ROLL_FORCE: "rollout_force", ROLL_COST: "rollout_cost", ASYNC_OUTPUTS: "async_outputs", ASYNC_POSES: "async_poses", FAST_UAVS: "fast_uavs",
            TICK_LONG: "tick_long", MODEL_ALL: "model_all"}
ROLLOUTS = (ROLL_PLAIN, ROLL_RATE, ROLL_FORCE, ROLL_COST)
STALL_FOLLOWERS = (ASYNC_OUTPUTS, ASYNC_POSES, GATHER, NEAREST, DEV_SET_INPUT)
# the kinds of the extended surface (drawn by SEEDS_EXT and VARIANTS_EXT only; SET_WORLDS only in their seeds with the `worlds` flag)
ROLL_TICK, ROLL_TICK_COST, ROLL_FEEDBACK, ROLL_TICK_FEEDBACK, PROXIMITY, SET_WORLDS = range(35, 41)
EXT_KINDS = (ROLL_TICK, ROLL_TICK_COST, ROLL_FEEDBACK, ROLL_TICK_FEEDBACK, PROXIMITY, SET_WORLDS)
OP_NAMES.update({ROLL_TICK: "rollout_ticks", ROLL_TICK_COST: "rollout_tick_cost", ROLL_FEEDBACK: "rollout_feedback",
                 ROLL_TICK_FEEDBACK: "rollout_tick_feedback", PROXIMITY: "proximity_cost", SET_WORLDS: "set_worlds"})
TICK_ROLLOUTS = (ROLL_TICK, ROLL_TICK_COST, ROLL_TICK_FEEDBACK)
ROLLOUTS_EXT = ROLLOUTS + (ROLL_TICK, ROLL_TICK_COST, ROLL_FEEDBACK, ROLL_TICK_FEEDBACK)
STALL_ROLLOUTS = (ROLL_TICK_COST, ROLL_TICK_FEEDBACK)  # what the FAST_UAVS recipe forces in place of TICK_LONG, half of the time
STALL_HORIZONS = (5, 12)                               # ... of at least four ticks
WORLD_LABELS = (0, 7, -2000000000, 1234567890)
OBS_POS, OBS_R = 1, 8
# the kinds of the scene surface (drawn by SEEDS_SCENE and VARIANTS_SCENE only, on top of everything the extended surface draws)
SCENE_KINDS = (SET_OBSTACLES, NEAREST_OBSTACLES, OBSTACLE_COST, SET_BEAMS, RANGE_SCAN, RANGE_SCAN_UAVS) = tuple(range(41, 47))
SCAN_BLIND, SCAN_TABLE = 47, 48  # never drawn, forced behind a table-changing call: a range_scan without the ground; a scan that reads the table
SCANS = (RANGE_SCAN, RANGE_SCAN_UAVS)
OP_NAMES.update({SET_OBSTACLES: "set_obstacles", NEAREST_OBSTACLES: "nearest_obstacles", OBSTACLE_COST: "obstacle_cost", SET_BEAMS: "set_scan_beams",
                 RANGE_SCAN: "range_scan", RANGE_SCAN_UAVS: "range_scan_uavs"})
PALETTE = (1.5, 3.0, 6.0)                       # radius and max_range: few enough values that cache hits and rebuilds both happen
OBSTACLE_COUNTS = (0, 1, 5, 5, 24, 24, 48, 48)  # M of a drawn set: 0 one time in eight
BEAM_COUNTS = (1, 7, 16, 64, 65)                # mixed_beams(nb); 65: a second beam group of the UAV scan with one live lane
OBST_MAX = 512
PAD_INT = -77  # what the slack columns of a padded int32 tensor hold, and a vector the call must overwrite
ON_WIDTHS = (3, 3, 1)
# host calls and device calls that re-intern airframe types: the device table is stale until some call uploads it
TABLE_CALLS = {7: "set_mass", 8: "set_ground_z", 17: "set_params", RESET: "reset"}
# what a scan is counted as following when none of the scans came in between
SCAN_MARKS = {8: "set_ground_z", 17: "set_params", RESET: "reset", CLONE: "clone", SET_WORLDS: "set_worlds", SET_OBSTACLES: "set_obstacles"}
# calls that enter through MRS_ENTER_COMMANDS (or do not enter at all): a collision tick that is pending stays pending across them
KEEP_PENDING = (0, 1, 2, 3, 9, 15, DEV_SET_INPUT, GATHER, ASYNC_OUTPUTS, ASYNC_POSES, PROXIMITY) + SCENE_KINDS
# scene calls that upload no airframe table (a range_scan does under MRS_SCAN_GROUND, a UAV scan always; so do both contact calls)
NO_TABLE_UPLOAD = (SET_OBSTACLES, NEAREST_OBSTACLES, OBSTACLE_COST, SET_BEAMS)
# the kinds of the contact surface (drawn by SEEDS_CONTACT and VARIANTS_CONTACT only, on top of everything the scene surface draws):
# tensors.obstacle_contacts without the mark (enters like obstacle_cost: a pending tick stays pending) and with crash=True (enters
# through settle(): the pending tick is evaluated first, so the kind is not in KEEP_PENDING)
CONTACT_KINDS = (OBSTACLE_CONTACTS, CONTACT_MARK) = (49, 50)
MARK_BEHIND_STALL = 51  # never drawn, forced in place of a follower of the FAST_UAVS recipe: a CONTACT_MARK that must replay the stall
OP_NAMES.update({OBSTACLE_CONTACTS: "obstacle_contacts", CONTACT_MARK: "contact_mark"})
KEEP_PENDING += (OBSTACLE_CONTACTS,)
# margins of the marking form: on the sequence fleets with the 48-obstacle sets of draw_obstacles a margin of 1.0 touches up to 99 of the
# 150 UAVs, 0.25 at most 52, 0.0 at most 31 (counted on the CPU over 48 fleet / set draws): the sequence must stay one of flying UAVs
MARK_MARGINS = (0.0, 0.25)
CONTACT_OUTPUTS = ("hit", "index", "sd", "counts")
CONTACT_SENTINEL = {"hit": 3, "index": PAD_INT, "sd": 7.25, "counts": PAD_INT}  # what a vector to fill holds before the call


def gather_width(groups):
    return sum(w for b, (_, w, _) in enumerate(GROUPS) if groups >> b & 1)


def group_floors(groups):
    """the floor of every column of a row of `groups`"""
    return np.concatenate([np.full(w, FIELD_FLOOR[f]) for b, (_, w, f) in enumerate(GROUPS) if groups >> b & 1])


def ref_rows(o, first, count, groups):
    """the FP64 observation rows [count, gather_width(groups)] of the oracle's UAVs, and their R [count, 3, 3]"""
    st, out, imu = o.get_state(first, count), o.get_outputs(first, count), o.get_imu(first, count)
    nm = np.array([o.get_params(first + k).n_motors for k in range(count)])
    rpm = np.where(np.arange(O.MAX_MOTORS)[None, :] < nm[:, None], st["motor_rpm"], 0.0)
    parts = (st["x"], st["v"], out["velocity_body"], st["R"].reshape(count, 9), out["orientation"], st["omega"], imu, rpm)
    return np.concatenate([a for b, a in enumerate(parts) if groups >> b & 1], axis=1), st["R"]


def near_quat_branch(R):
    """True where R [.., 3, 3] is within BRANCH_EPS of a branch boundary of Eigen's Quaterniond(Matrix3d): a trace of 0, or, where the
    diagonal decides (trace <= 0), a tie of its two largest entries.  There the quaternion is defined up to its overall sign only."""
    d = np.diagonal(R, axis1=-2, axis2=-1)
    tr = (d[..., 0] + d[..., 1]) + d[..., 2]
    s = np.sort(d, axis=-1)
    return (np.abs(tr) < BRANCH_EPS) | ((tr <= BRANCH_EPS) & (s[..., 2] - s[..., 1] < BRANCH_EPS))


def compare_rows(got, want, R, groups, rtol, f32, what):
    """observation rows of the product against the oracle's, every group on its own scale: per UAV, max |difference| over the group's
    columns <= tol * max(max |reference| over them, the group's floor); tol = rtol, plus one float rounding 2^-24 for FP32 rows.
    NaN / inf patterns must agree.  Returns the number of quaternions compared up to their sign (near_quat_branch)."""
    W = gather_width(groups)
    got, want, R = np.asarray(got, dtype=np.float64).reshape(-1, W), np.asarray(want, dtype=np.float64).reshape(-1, W), np.asarray(R).reshape(-1, 3, 3)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    tol = rtol + (2.0 ** -24 if f32 else 0.0)
    col = sign_cases = 0
    for b, (name, w, f) in enumerate(GROUPS):
        if not groups >> b & 1:
            continue
        a, r = got[:, col:col + w], want[:, col:col + w]
        col += w
        bad = ~np.isfinite(r)
        assert np.array_equal(np.isnan(a), np.isnan(r)), f"{what}: {name}: NaN pattern differs"
        assert np.array_equal(a[bad & ~np.isnan(r)], r[bad & ~np.isnan(r)]), f"{what}: {name}: inf pattern differs"
        with np.errstate(invalid="ignore"):
            diff = np.where(bad, 0.0, np.abs(a - r)).max(axis=1)
            if b == QUAT_BIT:
                near = near_quat_branch(R)
                sign_cases += int(near.sum())
                diff = np.where(near, np.minimum(diff, np.where(bad, 0.0, np.abs(a + r)).max(axis=1)), diff)
        scale = np.maximum(np.where(bad, 0.0, np.abs(r)).max(axis=1), FIELD_FLOOR[f])
        err = diff / scale
        i = int(np.argmax(err))
        assert err[i] <= tol, f"{what}: {name}: row {i} is off by {err[i]:.3e} > {tol:.3e} relative to its own scale"
    return sign_cases


def cost_bound(rows, targets, weights, groups, rtol):
    """first-order bound of the cost restatement's change when every row value moves by delta = rtol * max(|value|, its group's floor):
    sum over evaluations and columns of |w| * (2 |d| delta + delta^2), d = row - target"""
    rows = np.asarray(rows, dtype=np.float64)
    tg, wt = np.asarray(targets).astype(np.float64), np.asarray(weights).astype(np.float64)
    E, count, w = rows.shape
    wt = np.broadcast_to(wt[:, None, :w], (E, count, w))  # (one row serves every evaluation)
    with np.errstate(invalid="ignore", over="ignore"):
        delta = rtol * np.maximum(np.abs(rows), group_floors(groups)[None, None, :])
        d = np.abs(rows - tg[:, :, :w])
        return (np.abs(wt) * (2.0 * d * delta + delta * delta)).sum(axis=(0, 2))


def contact_violations(o, rtol):
    """the same-world pairs of the oracle swarm `o` that a collision pass could decide the other way within the compare's tolerance.
    Crash rows, crash costs and rebounce forces jump where a pair's squared distance d2 crosses its contact threshold crit.  Positions
    that agree within delta = rtol * max(|x|_inf, FIELD_FLOOR["x"]) per UAV move d2 by at most 2 d (delta_i + delta_j) to first order;
    a pair counts unless |d2 - crit| is at least twice that (the 2 is margin over the derived bound, not a measurement)."""
    n = o.n
    x, w = o.get_state()["x"], o.get_worlds()
    par = [o.get_params(i) for i in range(n)]
    r = np.array([q.arm_length + q.prop_radius for q in par])
    fin = np.isfinite(x).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[:, None, :] - x[None, :, :]
        d2 = (d * d).sum(axis=2)
        delta = rtol * np.maximum(np.abs(x).max(axis=1), FIELD_FLOOR["x"])
        moves = 2.0 * np.sqrt(d2) * (delta[:, None] + delta[None, :])
        close = np.abs(d2 - (r[:, None] + r[None, :])) < 2.0 * moves
    pair = (w[:, None] == w[None, :]) & fin[:, None] & fin[None, :]
    return int(np.triu(close & pair, 1).sum())


def airframes_of(o):
    """(ground_z [n], arm_length + prop_radius [n]) of the oracle swarm's parameters, the radius as contact_violations forms it"""
    par = [o.get_params(i) for i in range(o.n)]
    return np.array([q.ground_z for q in par]), np.array([q.arm_length + q.prop_radius for q in par])


def obstacle_contact_violations(o, ob, rad, margin, first, count, rtol):
    """the (UAV, obstacle) pairs of the range that a marking contact call could decide the other way within the compare's tolerance.
    The signed distance of every obstacle kind is 1-Lipschitz in the position, so positions that agree within delta_i = rtol *
    max(|x_i|_inf, FIELD_FLOOR["x"]) per component move sd by at most sqrt(3) delta_i; an applicable pair (the obstacle is ALL_WORLDS or
    carries the UAV's label; the position is finite) counts unless |sd - thr_i| is at least twice that, thr_i = rad_i + margin (the 2
    is margin over the derived bound, as in contact_violations, not a measurement)."""
    if len(ob) == 0 or count == 0:
        return 0
    sl = slice(first, first + count)
    x, w = o.get_state()["x"][sl], o.get_worlds()[sl]
    thr = np.broadcast_to(np.asarray(rad, np.float64), (o.n,))[sl] + np.float64(margin)
    with np.errstate(invalid="ignore", over="ignore"):
        sd, _ = signed_distances(x, ob)
        delta = rtol * np.maximum(np.abs(x).max(axis=1), FIELD_FLOOR["x"])
        close = np.abs(sd - thr[:, None]) < 2.0 * np.sqrt(3.0) * delta[:, None]
    applies = ((ob["flags"] & ALL_WORLDS) != 0)[None, :] | (ob["world"][None, :] == w[:, None].astype(np.int32))
    return int((close & applies & np.isfinite(x).all(axis=1)[:, None]).sum())


# ---- the product side --------------------------------------------------------------------------------------------------------------

class RecordingSwarm:
    """stands where the product's Swarm stands when a sequence runs against the oracle alone: every call is recorded by name"""

    def __init__(self, n, o):
        self.n, self.o, self.calls = n, o, []

    def input_staging(self, count, stride):
        self.calls.append("input_staging")
        return np.zeros((count, stride))

    def get_outputs_view(self, first, count):  # (so that host call 16 has something to compare: the oracle with itself)
        self.calls.append("get_outputs_view")
        return self.o.get_outputs(first, count)

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append(name)
        return call


class StubPair(Pair):
    """a Pair whose product is a RecordingSwarm"""

    def __init__(self, M, n):
        self.M, self.n = M, n
        self.o = O.OracleSwarm(n)
        self.g = RecordingSwarm(n, self.o)

    def compare(self, *a, **kw):
        return 0.0


class Stub:
    """the device-resident calls as argument checks: what include/mrs_swarm.h and tensors.py accept, asserted; every tuple is recorded"""
    real = False
    tick_rollout_stats = (0, 0)

    def __init__(self, p):
        self.p, self.calls, self.open = p, [], {"outputs": [], "poses": []}
        self.next_ticket = 0

    def _range(self, first, count):
        assert 0 <= first and count >= 1 and first + count <= self.p.n, (first, count)

    def _motors(self, first, count):
        return max(self.p.o.get_params(first + k).n_motors for k in range(count))

    def _commands(self, mode, rows, first, pad):
        count, w = rows.shape[-2], rows.shape[-1]
        self._range(first, count)
        assert 0 <= mode <= 10 and pad >= 0
        if mode == O.ACTUATOR_CMD:
            assert pad == 0 and self._motors(first, count) <= w <= O.MAX_MOTORS, "actuator rows: dense, and as wide as n_motors"
        else:
            assert w >= max(WIDTH[mode], 1)
        assert np.isfinite(rows).all()

    def set_input(self, mode, rows, first, f32, pad):
        assert rows.ndim == 2
        self._commands(mode, rows, first, pad)
        self.calls.append(("set_input", mode, rows.shape, first, f32, pad))

    def apply_force(self, rows, first, f32, pad):
        assert rows.ndim == 2 and rows.shape[1] == 3 and pad >= 0
        self._range(first, rows.shape[0])
        self.calls.append(("apply_force", rows.shape, first, f32, pad))

    def gather(self, groups, first, count, f32, pad):
        self._range(first, count)
        assert 1 <= groups <= 255 and pad >= 0
        self.calls.append(("gather", groups, first, count, f32, pad))

    def crashed(self, first, count):
        self._range(first, count)
        self.calls.append(("crashed", first, count))

    def reset(self, mask, pos, heading, takeoff, first, f32, u8):
        count = len(mask)
        self._range(first, count)
        assert mask.dtype == bool and mask.any() and pos.shape == (count, 3) and (heading is None or heading.shape == (count,))
        self.calls.append(("reset", int(mask.sum()), first, count, heading is not None, takeoff, f32, u8))

    def save_load(self, first, count, index):
        self._range(first, count)
        if index is not None:
            assert index.shape == (count,) and ((index == -1) | (index == np.arange(count))).all()
        self.calls.append(("save_load", first, count, None if index is None else int((index < 0).sum())))

    def clone_swap(self):
        assert not self.open["outputs"] and not self.open["poses"], "a ticket would outlive its swarm"
        self.calls.append(("clone",))

    def nearest(self, k, radius, fields, first, count, f32, worlds=None):
        self._range(first, count)
        assert 1 <= k <= 32 and radius > 0 and 0 <= fields <= 31
        self.calls.append(("nearest", k, radius, fields, first, count, f32))

    def _rates(self, steps, hold, every, blocks):
        assert steps >= 1 and hold >= 1 and every >= 1 and steps % hold == 0 and steps % every == 0 and blocks * hold == steps, (steps, hold, every, blocks)

    def rollout(self, mode, cmd, first, groups, hold, every, forces, fhold, f32, pads):
        assert cmd.ndim == 3
        self._commands(mode, cmd, first, pads[0])
        steps = cmd.shape[0] * hold
        self._rates(steps, hold, every, cmd.shape[0])
        assert 0 <= groups <= 255 and min(pads) >= 0
        if forces is not None:
            assert forces.shape[1:] == (cmd.shape[1], 3) and fhold >= 1 and forces.shape[0] * fhold == steps, (forces.shape, fhold, steps)
        self.calls.append(("rollout", mode, cmd.shape, first, groups, hold, every, None if forces is None else (forces.shape, fhold), f32, pads))

    def rollout_cost(self, mode, cmd, first, groups, targets, weights, hold, every, start, f32, pads):
        assert cmd.ndim == 3
        self._commands(mode, cmd, first, pads[0])
        steps, count = cmd.shape[0] * hold, cmd.shape[1]
        self._rates(steps, hold, every, cmd.shape[0])
        E, w = steps // every, gather_width(groups)
        assert 1 <= groups <= 255 and targets.shape == (E, count, w) and weights.shape in ((E, w), (1, w)) and min(pads) >= 0
        assert start is None or start.shape == (count,)
        self.calls.append(("rollout_cost", mode, cmd.shape, first, groups, weights.shape[0], hold, every, start is not None, f32, pads))

    def _head(self, mode, cmd, first, hold, every, pads):
        """the command side of a rollout; returns (ticks, count, evaluations)"""
        assert cmd.ndim == 3
        self._commands(mode, cmd, first, pads[0])
        steps = cmd.shape[0] * hold
        self._rates(steps, hold, every, cmd.shape[0])
        assert min(pads) >= 0
        return steps, cmd.shape[1], steps // every

    @staticmethod
    def _evaluation(groups, targets, weights, E, count, start):
        """targets, weights and the start vector of a costed call; groups == 0 takes no targets and no weights"""
        w = gather_width(groups)
        assert 0 <= groups <= 255 and (start is None or start.shape == (count,))
        if groups:
            assert targets.shape == (E, count, w) and weights.shape in ((E, w), (1, w))
        else:
            assert targets is None and weights is None

    @staticmethod
    def _collide(crash, rebounce, crash_cost=0.0):
        assert isinstance(crash, bool) and np.isfinite(rebounce) and np.isfinite(crash_cost)

    def rollout_ticks(self, mode, cmd, first, groups, hold, every, crash, rebounce, crashed, f32, pads, measure=False):
        steps, count, E = self._head(mode, cmd, first, hold, every, pads)
        self._collide(crash, rebounce)
        assert 0 <= groups <= 255 and crashed in ("bool", "uint8", None)
        self.calls.append(("rollout_ticks", mode, cmd.shape, first, groups, hold, every, crash, rebounce, crashed, f32, pads))

    def rollout_tick_cost(self, mode, cmd, first, groups, targets, weights, crash_cost, hold, every, crash, rebounce, start, f32, pads, measure=False):
        steps, count, E = self._head(mode, cmd, first, hold, every, pads)
        self._collide(crash, rebounce, crash_cost)
        self._evaluation(groups, targets, weights, E, count, start)
        self.calls.append(("rollout_tick_cost", mode, cmd.shape, first, groups, None if weights is None else weights.shape[0], crash_cost, hold, every,
                           crash, rebounce, start is not None, f32, pads))

    def _feedback(self, name, tick, mode, cmd, first, fb_groups, gains, refs, cost_groups, targets, weights, hold, every, start, want_out, f32, pads):
        steps, count, E = self._head(mode, cmd, first, hold, every, pads)
        B, wo = cmd.shape[0], gather_width(fb_groups)
        wc = cmd.shape[2] if mode == O.ACTUATOR_CMD else WIDTH[mode]
        assert mode != 0, "a feedback rollout needs a mode with a payload: tensors.py refuses INPUT_UNKNOWN"
        assert 1 <= fb_groups <= 255 and cmd.shape[2] == wc
        assert gains.ndim in (3, 4) and gains.shape[0] in (1, B) and gains.shape[1:3] == (wc, wo) and (gains.ndim == 3 or gains.shape[3] == count)
        assert refs.ndim == 3 and refs.shape[0] in (1, B) and refs.shape[1] in (1, count) and refs.shape[2] == wo
        assert np.isfinite(gains).all() and np.isfinite(refs).all()
        self._evaluation(cost_groups, targets, weights, E, count, start)
        if cost_groups:
            assert want_out
        elif tick is None:
            assert not want_out and start is None, "cost_groups == 0 is a run without a cost"
        else:
            self._collide(*tick)
            assert want_out or start is None, "accumulate needs the vector it adds to"
        self.calls.append((name, mode, cmd.shape, first, fb_groups, gains.shape, refs.shape, cost_groups, hold, every, tick, start is not None, want_out,
                           f32, pads))

    def rollout_feedback(self, *a):
        self._feedback("rollout_feedback", None, *a)

    def rollout_tick_feedback(self, tick, *a, measure=False):
        self._feedback("rollout_tick_feedback", tick, *a)

    def proximity_cost(self, k, radius, kind, weight, eps, first, count, start, found):
        self._range(first, count)
        assert 1 <= k <= 32 and np.isfinite(radius) and radius > 0 and kind in (0, 1, 2) and np.isfinite(weight) and np.isfinite(eps) and eps >= 0
        assert (start is None or start.shape == (count,)) and isinstance(found, bool)
        self.calls.append(("proximity_cost", k, radius, kind, weight, eps, first, count, start is not None, found))

    def set_worlds(self, worlds, first):
        assert worlds.dtype == np.int32 and worlds.ndim == 1
        self._range(first, len(worlds))
        self.calls.append(("set_worlds", first, len(worlds)))

    # ---- the scene calls: include/mrs_swarm.h, "static obstacles", "range scans", "range scans that see other UAVs" ----

    def set_obstacles(self, ob, host):
        assert ob.dtype == OBSTACLE and ob.ndim == 1 and len(ob) <= OBST_MAX
        assert np.isin(ob["kind"], (0, 1, 2)).all() and not (ob["flags"] & ~np.uint32(ALL_WORLDS)).any() and not ob["reserved"].any()
        assert np.isfinite(ob["c"]).all()
        used = np.stack([np.ones(len(ob), bool), ob["kind"] == 1, ob["kind"] != 0], axis=1)
        pillar = np.zeros((len(ob), 3), bool)
        pillar[:, 2] = (ob["kind"] == CYLINDER) & (ob["h"][:, 2] == np.inf)
        assert not (used & ~pillar & ~(np.isfinite(ob["h"]) & (ob["h"] >= 0))).any(), "sizes: finite and >= 0 (a cylinder's half-height may be +inf)"
        self.calls.append(("set_obstacles", len(ob), host))

    def set_beams(self, beams, host):
        assert beams.ndim == 2 and beams.shape[1] == 3 and 1 <= len(beams) <= MAX_BEAMS, "the pattern is never cleared"
        assert np.isfinite(beams).all() and (np.abs((beams * beams).sum(axis=1) - 1.0) <= 1e-9).all()
        self.calls.append(("set_scan_beams", len(beams), host))

    def _query(self, k, radius, first, count):
        self._range(first, count)
        assert 1 <= k <= 32 and np.isfinite(radius) and radius > 0

    def nearest_obstacles(self, k, radius, fields, first, count, f32, pads):
        self._query(k, radius, first, count)
        assert 0 <= fields <= 7 and min(pads) >= 0, "unknown field bits, or a stride below k * the width of the fields / below k"
        outputs = (fields != 0, True, True)  # rows, index, counts: tensors.py always passes the last two
        assert any(outputs)
        self.calls.append(("nearest_obstacles", k, radius, fields, first, count, f32, pads))

    def obstacle_cost(self, k, radius, kind, weight, first, count, start, found):
        self._query(k, radius, first, count)
        assert kind in (0, 2) and np.isfinite(weight) and (start is None or start.shape == (count,)) and isinstance(found, bool)
        self.calls.append(("obstacle_cost", k, radius, kind, weight, first, count, start is not None, found))

    def range_scan(self, see_uavs, max_range, flags, first, count, f32, nb, pads, hits, uavs=False):
        self._range(first, count)
        assert np.isfinite(max_range) and max_range > 0 and not flags & ~(BODY_FRAME | GROUND) and 1 <= nb <= MAX_BEAMS
        assert min(pads) >= 0, "a stride below n_beams"
        assert isinstance(hits, bool) and isinstance(uavs, bool) and (see_uavs or not uavs)  # (the ranges are the output that is always there)
        self.calls.append(("range_scan_uavs" if see_uavs else "range_scan", max_range, flags, first, count, f32, nb, pads, hits, uavs))

    def obstacle_contacts(self, margin, crash, first, count, outs, fill, start, hit_cost):
        """include/mrs_swarm.h, "obstacle contacts": the range; a finite margin >= 0; a finite hit_cost when a cost vector is given; no
        output and no mark is refused ("nothing to do")"""
        self._range(first, count)
        assert isinstance(crash, bool) and isinstance(fill, bool) and np.isfinite(margin) and margin >= 0
        assert set(outs) <= set(CONTACT_OUTPUTS) and len(set(outs)) == len(outs)
        assert start is None or (start.shape == (count,) and np.isfinite(hit_cost))
        assert crash or outs or start is not None, "nothing to do"
        self.calls.append(("obstacle_contacts", margin, crash, first, count, tuple(outs), fill, start is not None, hit_cost))

    def scene_state(self):
        return None

    def grid_builds(self):
        return None

    def async_issue(self, kind, first, count):
        self._range(first, count)
        self.open[kind].append(self.next_ticket)
        assert len(self.open[kind]) <= 2, "more than two tickets of one kind"
        self.calls.append(("async_issue", kind, first, count))
        self.next_ticket += 1
        return self.next_ticket - 1

    def async_wait(self, kind, ticket):
        assert self.open[kind] and self.open[kind][0] == ticket, "tickets are waited for in the order they were issued"
        self.open[kind].pop(0)
        self.calls.append(("async_wait", kind, ticket))

    def finish(self):
        return np.zeros(7, dtype=np.int64)


PAD_VALUE = 7.25  # what the slack columns of every padded tensor hold before and after a call


class Device:
    """the device-resident calls through mrs_multirotor_simulator_amd.tensors: numpy in, numpy out; rows live in tensors with `pad`
    slack columns, so that every stride is larger than its width, and the slack must come back untouched.  side=True: every tensor is
    written, used and read under a torch stream of its own, so that the library's fences are what orders the data."""
    real = True

    def __init__(self, p, side):
        import torch
        from mrs_multirotor_simulator_amd import tensors as T
        self.p, self.T, self.torch = p, T, torch
        self.dev = torch.device("cuda", p.g.device())
        self.stream = torch.cuda.Stream(self.dev) if side else None
        self.totals = np.zeros(7, dtype=np.int64)  # fused_stats (4), download_stats (2), split_stats[0]
        self.tick_rollout_stats = np.zeros(2, dtype=np.int64)  # stalls and replayed launches inside the measured tick-rollout calls

    def ctx(self):
        return self.torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def _dtype(self, f32):
        return self.torch.float32 if f32 else self.torch.float64

    def _up(self, a, pad, f32):
        """`a` in the leading columns of a tensor with `pad` slack columns: (the whole tensor, the view that holds a)"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        big = self.torch.full(a.shape[:-1] + (a.shape[-1] + pad,), PAD_VALUE, dtype=self._dtype(f32), device=self.dev)
        view = big[..., :a.shape[-1]]
        if a.size:
            view.copy_(self.torch.from_numpy(a).to(self._dtype(f32)))
        return big, view

    def _empty(self, shape, pad, f32):
        big = self.torch.full(tuple(shape[:-1]) + (shape[-1] + pad,), PAD_VALUE, dtype=self._dtype(f32), device=self.dev)
        return big, big[..., :shape[-1]]

    @staticmethod
    def _down(big, width, what):
        host = big.cpu().numpy()
        assert (host[..., width:] == PAD_VALUE).all(), f"{what}: the slack columns were written"
        return host[..., :width]

    def set_input(self, mode, rows, first, f32, pad):
        with self.ctx():
            _, view = self._up(rows, pad, f32)
            self.T.set_input(self.p.g, mode, view, first)

    def apply_force(self, rows, first, f32, pad):
        with self.ctx():
            _, view = self._up(rows, pad, f32)
            self.T.apply_force(self.p.g, view, first)

    def gather(self, groups, first, count, f32, pad):
        w = gather_width(groups)
        with self.ctx():
            big, view = self._empty((count, w), pad, f32)
            self.T.gather(self.p.g, groups, first, count, out=view)
            return self._down(big, w, "gather")

    def crashed(self, first, count):
        with self.ctx():
            return self.T.crashed(self.p.g, first, count).cpu().numpy()

    def reset(self, mask, pos, heading, takeoff, first, f32, u8):
        torch = self.torch
        with self.ctx():
            m = torch.tensor(mask, device=self.dev)
            hd = None if heading is None else torch.tensor(heading, dtype=self._dtype(f32), device=self.dev)
            self.T.reset(self.p.g, m.to(torch.uint8) if u8 else m, torch.tensor(pos, dtype=self._dtype(f32), device=self.dev), hd, takeoff=takeoff,
                         first=first)

    def save_load(self, first, count, index):
        with self.ctx():
            rec = self.T.save(self.p.g, first, count)
            idx = None if index is None else self.torch.tensor(index, dtype=self.torch.int32, device=self.dev)
            return self.T.load(self.p.g, rec, first, index=idx).cpu().numpy()

    def harvest(self):
        g = self.p.g
        self.totals += np.array([*g.fused_stats(), *g.download_stats(), g.split_stats()[0]], dtype=np.int64)

    def clone_swap(self):
        self.harvest()  # (the counters stay with the handle)
        new = self.p.g.clone()
        self.p.g.close()
        self.p.g = new

    def nearest(self, k, radius, fields, first, count, f32, worlds=None):
        with self.ctx():
            rows, idx, cnt = self.T.nearest(self.p.g, k, radius, fields, first, count, dtype=self._dtype(f32))
            s = self.p.g.get_states()  # right after the call: the state it read
            compare_with_numpy(self.T, rows, idx, cnt, s["x"], s["v"], s["R"].reshape(self.p.n, 3, 3), k, radius, fields, self._dtype(f32), first, count,
                               label=("nearest", k, radius, fields, first, count), worlds=worlds)

    def rollout(self, mode, cmd, first, groups, hold, every, forces, fhold, f32, pads):
        steps, count, w = cmd.shape[0] * hold, cmd.shape[1], gather_width(groups)
        with self.ctx():
            _, c = self._up(cmd, pads[0], f32)
            f = None if forces is None else self._up(forces, pads[2], f32)[1]
            big, out = self._empty((steps // every, count, w), pads[1], f32) if groups else (None, None)
            self.T.rollout(self.p.g, mode, c, DT, groups, first=first, out=out, hold=hold, obs_every=every, forces=f, force_hold=fhold)
            return self._down(big, w, "rollout") if groups else None

    def rollout_cost(self, mode, cmd, first, groups, targets, weights, hold, every, start, f32, pads):
        torch = self.torch
        with self.ctx():
            _, c = self._up(cmd, pads[0], f32)
            _, tg = self._up(targets, pads[1], f32)
            _, wt = self._up(weights, pads[2], f32)
            out = None if start is None else torch.tensor(start, dtype=torch.float64, device=self.dev)
            got = self.T.rollout_cost(self.p.g, mode, c, DT, groups, tg, wt, first=first, hold=hold, cost_every=every, out=out, accumulate=start is not None)
            return got.cpu().numpy()

    def _measured(self, measure, call):
        """`call()`, and with `measure` the stalls and replayed launches it took: fused_stats() before and after.  Both reads enter like
        state calls and evaluate a pending collision tick, so the generator asks for them only where it expects none before the call and
        needs none behind it."""
        if not measure:
            return call()
        before = self.p.g.fused_stats()
        got = call()
        after = self.p.g.fused_stats()
        self.tick_rollout_stats += [after[1] - before[1], after[2] - before[2]]
        return got

    def rollout_ticks(self, mode, cmd, first, groups, hold, every, crash, rebounce, crashed, f32, pads, measure=False):
        torch = self.torch
        steps, count, w = cmd.shape[0] * hold, cmd.shape[1], gather_width(groups)
        E = steps // every
        with self.ctx():
            _, c = self._up(cmd, pads[0], f32)
            big, out = self._empty((E, count, w), pads[1], f32) if groups else (None, None)
            cr = False
            if crashed is not None:  # (3: a byte the call must overwrite with 0 or 1)
                cr = torch.zeros((E, count), dtype=torch.bool, device=self.dev) if crashed == "bool" else torch.full((E, count), 3, dtype=torch.uint8,
                                                                                                                     device=self.dev)
            self._measured(measure, lambda: self.T.rollout_ticks(self.p.g, mode, c, DT, crash, rebounce, groups, first=first, out=out, hold=hold,
                                                                 obs_every=every, crashed=cr))
            return (self._down(big, w, "rollout_ticks") if groups else None), (None if crashed is None else cr.cpu().numpy())

    def _evaluation(self, groups, targets, weights, start, want_out, count, f32, pads):
        """(targets, weights, out) of a costed call as tensors: padded rows; `out` holds `start`, or PAD_VALUE where the call overwrites it"""
        torch = self.torch
        tg = wt = out = None
        if groups:
            tg, wt = self._up(targets, pads[1], f32)[1], self._up(weights, pads[2], f32)[1]
        if start is not None:
            out = torch.tensor(start, dtype=torch.float64, device=self.dev)
        elif want_out:
            out = torch.full((count,), PAD_VALUE, dtype=torch.float64, device=self.dev)
        return tg, wt, out

    def rollout_tick_cost(self, mode, cmd, first, groups, targets, weights, crash_cost, hold, every, crash, rebounce, start, f32, pads, measure=False):
        with self.ctx():
            _, c = self._up(cmd, pads[0], f32)
            tg, wt, out = self._evaluation(groups, targets, weights, start, True, cmd.shape[1], f32, pads)
            got = self._measured(measure, lambda: self.T.rollout_tick_cost(self.p.g, mode, c, DT, crash, rebounce, groups, tg, wt, crash_cost=crash_cost,
                                                                           first=first, hold=hold, cost_every=every, out=out,
                                                                           accumulate=start is not None))
            return got.cpu().numpy()

    def _feedback(self, tick, mode, cmd, first, fb_groups, gains, refs, cost_groups, targets, weights, hold, every, start, want_out, f32, pads, measure):
        torch, count = self.torch, cmd.shape[1]
        with self.ctx():
            _, c = self._up(cmd, pads[0], f32)
            gn = torch.tensor(np.ascontiguousarray(gains), dtype=self._dtype(f32), device=self.dev)  # (dense, UAV-minor when per UAV)
            rf = self._up(refs, pads[3] if refs.shape[1] == count and count > 1 else 0, f32)[1]        # (shared setpoint rows are dense)
            tg, wt, out = self._evaluation(cost_groups, targets, weights, start, want_out, count, f32, pads)
            kw = dict(cost_groups=cost_groups, targets=tg, weights=wt, first=first, hold=hold, cost_every=every, out=out, accumulate=start is not None)
            if tick is None:
                got = self.T.rollout_feedback(self.p.g, mode, c, DT, fb_groups, gn, rf, **kw)
            else:
                crash, rebounce, crash_cost = tick
                got = self._measured(measure, lambda: self.T.rollout_tick_feedback(self.p.g, mode, c, DT, crash, rebounce, fb_groups, gn, rf,
                                                                                   crash_cost=crash_cost, **kw))
            assert (got is None) == (out is None and not cost_groups), "a run without a cost returns None, a costed one its vector"
            return None if got is None else got.cpu().numpy()

    def rollout_feedback(self, *a):
        return self._feedback(None, *a, False)

    def rollout_tick_feedback(self, tick, *a, measure=False):
        return self._feedback(tick, *a, measure)

    def proximity_cost(self, k, radius, kind, weight, eps, first, count, start, found):
        torch = self.torch
        with self.ctx():
            out = None if start is None else torch.tensor(start, dtype=torch.float64, device=self.dev)
            cost, fnd = self.T.proximity_cost(self.p.g, radius, k=k, kind=kind, weight=weight, eps=eps, first=first, count=count, out=out,
                                              accumulate=start is not None, found=found)
            return cost.cpu().numpy(), None if fnd is None else fnd.cpu().numpy()

    def set_worlds(self, worlds, first):
        with self.ctx():
            self.T.set_worlds(self.p.g, self.torch.tensor(worlds, dtype=self.torch.int32, device=self.dev), first)

    # ---- the scene calls: padded int32 rows hold PAD_INT where float rows hold PAD_VALUE ----

    def _ints(self, shape, pad):
        big = self.torch.full(tuple(shape[:-1]) + (shape[-1] + pad,), PAD_INT, dtype=self.torch.int32, device=self.dev)
        return big, big[..., :shape[-1]]

    @staticmethod
    def _down_ints(big, width, what):
        host = big.cpu().numpy()
        assert (host[..., width:] == PAD_INT).all(), f"{what}: the slack columns were written"
        return host[..., :width]

    def set_obstacles(self, ob, host):
        torch = self.torch
        with self.ctx():
            if host:
                self.p.g.set_obstacles(ob)
            else:  # (the set travels through the host: tensors of the device and arrays both serve)
                self.T.set_obstacles(self.p.g, ob["kind"], torch.tensor(ob["c"], dtype=torch.float64, device=self.dev),
                                     torch.tensor(ob["h"], dtype=torch.float64, device=self.dev), worlds=ob["world"],
                                     all_worlds=(ob["flags"] & ALL_WORLDS) != 0)

    def set_beams(self, beams, host):
        with self.ctx():
            if host:
                self.p.g.set_scan_beams(beams)
            else:
                self.T.set_scan_beams(self.p.g, self.torch.tensor(beams, dtype=self.torch.float64, device=self.dev))

    def nearest_obstacles(self, k, radius, fields, first, count, f32, pads):
        torch = self.torch
        w = k * sum(ON_WIDTHS[b] for b in range(3) if fields >> b & 1)
        with self.ctx():
            big, out = self._empty((count, w), pads[0], f32) if fields else (None, None)
            ibig, index = self._ints((count, k), pads[1])
            counts = torch.full((count,), PAD_INT, dtype=torch.int32, device=self.dev)
            rows, _, _ = self.T.nearest_obstacles(self.p.g, k, radius, fields, first, count, out=out, index=index, counts=counts)
            assert (rows is None) == (fields == 0)
            return (self._down(big, w, "nearest_obstacles") if fields else None), self._down_ints(ibig, k, "nearest_obstacles: index"), counts.cpu().numpy()

    def obstacle_cost(self, k, radius, kind, weight, first, count, start, found):
        torch = self.torch
        with self.ctx():
            out = None if start is None else torch.tensor(start, dtype=torch.float64, device=self.dev)
            fnd = torch.full((count,), PAD_INT, dtype=torch.int32, device=self.dev) if found else False
            cost, fnd = self.T.obstacle_cost(self.p.g, radius, k=k, kind=kind, weight=weight, first=first, count=count, out=out,
                                             accumulate=start is not None, found=fnd)
            return cost.cpu().numpy(), None if fnd is None else fnd.cpu().numpy()

    def range_scan(self, see_uavs, max_range, flags, first, count, f32, nb, pads, hits, uavs=False):
        name = "range_scan_uavs" if see_uavs else "range_scan"
        body, ground = bool(flags & BODY_FRAME), bool(flags & GROUND)
        with self.ctx():
            big, out = self._empty((count, nb), pads[0], f32)
            hbig, hview = self._ints((count, nb), pads[1]) if hits else (None, None)
            ubig, uview = self._ints((count, nb), pads[2]) if uavs else (None, None)
            if see_uavs:
                got = self.T.range_scan_uavs(self.p.g, max_range, body, ground, first, count, out=out, hits=hview, uavs=uview)
            else:
                got = self.T.range_scan(self.p.g, max_range, body, ground, first, count, out=out, hits=hview) + (None,)
            assert (got[1] is None) == (not hits) and (got[2] is None) == (not uavs), f"{name}: an output that was not asked for"
            return (self._down(big, nb, name), self._down_ints(hbig, nb, name + ": hit") if hits else None,
                    self._down_ints(ubig, nb, name + ": uav") if uavs else None)

    def obstacle_contacts(self, margin, crash, first, count, outs, fill, start, hit_cost):
        """the outputs named in `outs` (fill: vectors holding CONTACT_SENTINEL that the call must overwrite and hand back; else True: new
        vectors) and, with `start`, the cost vector after the call: {name: numpy}"""
        torch = self.torch
        dtypes = {"hit": torch.uint8, "index": torch.int32, "sd": torch.float64, "counts": torch.int32}
        with self.ctx():
            kw = {name: torch.full((count,), CONTACT_SENTINEL[name], dtype=dtypes[name], device=self.dev) if fill else True for name in outs}
            cost = None if start is None else torch.tensor(start, dtype=torch.float64, device=self.dev)
            got = self.T.obstacle_contacts(self.p.g, margin, crash, first, count, cost=cost, hit_cost=hit_cost, **kw)
            res = {}
            for name, t in zip(CONTACT_OUTPUTS, got):
                assert (t is None) == (name not in outs), f"obstacle_contacts: {name}: an output that was not asked for, or none that was"
                if t is not None:
                    assert not fill or t is kw[name], f"obstacle_contacts: {name}: not the vector that was given"
                    assert t.shape == (count,) and t.dtype == dtypes[name]
                    res[name] = t.cpu().numpy()
            if cost is not None:
                res["cost"] = cost.cpu().numpy()
            return res

    def scene_state(self):
        """(the obstacle set, the beam pattern) as the product returns them: both getters take the lock only"""
        return self.p.g.get_obstacles(), self.p.g.get_scan_beams()

    def grid_builds(self):
        return self.p.g.obstacle_stats()["grid_builds"]  # (mrs_swarm_obstacle_stats takes the lock only: a pending tick stays pending)

    def async_issue(self, kind, first, count):
        return self.p.g.get_outputs_async(first, count) if kind == "outputs" else self.p.g.get_poses_async(first, count)

    def async_wait(self, kind, ticket):
        return (self.p.g.outputs_wait(ticket) if kind == "outputs" else self.p.g.poses_wait(ticket)).copy()

    def finish(self):
        self.harvest()
        return self.totals


# (seed, FAST arithmetic, fleet, the long rollout, model-only phases): odd seeds run their tensor calls under a torch stream of their own
SEEDS = [(s, s % 3 == 2, "mixed" if (s // 2) % 2 else "x500", 16 <= s < 20, s >= 20) for s in range(28)]
RNG_BASE = 5000
# the largest step total of the 24 sequences of test_random_sequences_gpu.py (test_random_device_sequences.py counts both modules' totals)
STEP_CAP = 76
# child-process variants of the GPU module: (environment, (seed, ...) one per fleet, host call 12 in runs of at least four launches)
VARIANTS = {"split": ({"MRS_SPLIT_MIN_BLOCKS": "1"}, (4, 7), True),
            "pointer": ({"MRS_NO_BUFFER_ADDRESSING": "1"}, (1, 2), False),
            "split+pointer": ({"MRS_SPLIT_MIN_BLOCKS": "1", "MRS_NO_BUFFER_ADDRESSING": "1"}, (8, 3), True)}


def seed_rtol(fast):
    return 1e-7 if fast else helpers.RTOL_LITERAL  # the tolerances of test_random_sequences_gpu.py, as they are


# the seeds of the extended surface, with the flags of SEEDS by the same rules and two more: (seed, FAST, fleet, the long rollout — here a
# tick rollout —, model-only phases, collision worlds).  The numbers are those of a run of candidates that keep the two conditions of the
# module docstring and the limits of test_the_oracle_stays_usable (test_random_device_sequences.py asserts all of it).
EXT_SEED_NUMBERS = (100, 101, 102, 103, 104, 105, 107, 108, 109, 110, 112, 113, 114, 116, 117, 118, 119, 121, 130, 131)
EXT_LONG_SEED = 100


def ext_flags(s):
    return s, s % 3 == 2, "mixed" if (s // 2) % 2 else "x500", s == EXT_LONG_SEED, s % 5 == 4, s % 5 in (0, 2)


SEEDS_EXT = [ext_flags(s) for s in EXT_SEED_NUMBERS]
# two more seeds per child-process variant, one per fleet and one of them with worlds
VARIANTS_EXT = {"split": (108, 107), "pointer": (121, 102), "split+pointer": (105, 126)}

# the seeds of the scene surface, from 200 up, with the flags of ext_flags (none takes the long horizon); chosen like EXT_SEED_NUMBERS
SCENE_SEED_NUMBERS = (200, 201, 202, 203, 204, 205, 206, 222, 230, 242, 260, 280)
SEEDS_SCENE = [ext_flags(s) for s in SCENE_SEED_NUMBERS]
# one more seed per child-process variant
VARIANTS_SCENE = {"split": 317, "pointer": 221, "split+pointer": 310}


# what the 12 dry runs of SEEDS_SCENE add up to (scene_totals): test_random_device_sequences.py asserts these figures exactly, the GPU
# module about half of each, there counted from the restatement of the product's own state
SCENE_COUNTS = {"set_obstacles": 16, "nearest_obstacles": 16, "obstacle_cost": 17, "set_scan_beams": 18, "range_scan": 41, "range_scan_uavs": 21,
                "scene_behind_pending": 16,
                # scans that follow the call, no other scan in between; table-changing call, blind range_scan, scan that reads the table
                "scan_after_set_ground_z": 9, "scan_after_set_params": 8, "scan_after_reset": 7, "scan_after_clone": 8, "scan_after_set_worlds": 7,
                "scan_after_set_obstacles": 12, "stale_table_shapes": 10,
                # beams by what took them, beams of range 0, beams a UAV takes from an obstacle and beams an obstacle keeps from a UAV
                "hit_sphere": 448, "hit_box": 614, "hit_cylinder": 4862, "hit_uav": 2594, "hit_ground": 2725, "hit_none": 64699, "range_zero": 2398,
                "uav_takes_from_obstacle": 66, "obstacle_keeps_from_uav": 63,
                # query UAVs with more obstacles within the radius than slots, and with none; builds and hits of the two cache entries
                "found_over_k": 65, "found_none": 958, "query_grid_builds": 29, "query_cache_hits": 4, "scan_grid_builds": 53, "scan_cache_hits": 9}


def scene_totals(results):
    """the figures of SCENE_COUNTS over the results of run_sequence: calls per scene kind, scene calls behind a pending collision tick,
    and what the restatements and the cache model met"""
    results = list(results)
    total = {OP_NAMES[op]: sum(r["kinds"][op] for r in results) for op in SCENE_KINDS}
    total["scene_behind_pending"] = sum(r["scene_behind_pending"] for r in results)
    tally = sum((r["scene"] for r in results), Counter())
    total.update({name: int(tally[name]) for name in SCENE_TALLIES})
    return total


SCENE_TALLIES = ("scan_after_set_ground_z", "scan_after_set_params", "scan_after_reset", "scan_after_clone", "scan_after_set_worlds",
                 "scan_after_set_obstacles", "stale_table_shapes", "hit_sphere", "hit_box", "hit_cylinder", "hit_uav", "hit_ground", "hit_none",
                 "range_zero", "uav_takes_from_obstacle", "obstacle_keeps_from_uav", "found_over_k", "found_none", "query_grid_builds",
                 "query_cache_hits", "scan_grid_builds", "scan_cache_hits")


# the seeds of the contact surface, from 400 up (VARIANTS_SCENE took numbers above 300), with the flags of ext_flags; chosen like
# EXT_SEED_NUMBERS: candidates that keep the three honesty conditions, the limits of test_the_oracle_stays_usable and the conditions
# test_random_device_sequences.py states for them
CONTACT_SEED_NUMBERS = (415, 422, 428, 437, 446, 450, 470, 471, 472, 474, 484, 500)
SEEDS_CONTACT = [ext_flags(s) for s in CONTACT_SEED_NUMBERS]
# one more seed per child-process variant
VARIANTS_CONTACT = {"split": 565, "pointer": 411, "split+pointer": 545}

# what the 12 dry runs of SEEDS_CONTACT add up to (contact_totals): asserted exactly by test_random_device_sequences.py, at scene_floor
# by the GPU module, there counted from the restatement on the product's state
CONTACT_COUNTS = {"obstacle_contacts": 34, "contact_mark": 59, "contacts_behind_pending": 12, "marks_behind_pending": 13,
                  # marks among the followers of the stall recipe; marks while a pipelined download is open
                  "marks_behind_stall": 7, "marks_with_open_ticket": 25,
                  # UAVs of the ranges that touch, that touch more than one obstacle, that a mark crashed first, and of those the ones
                  # a later tick rollout showed in its first crash row; marking calls over an empty touching set
                  "uavs_touching": 302, "uavs_touching_several": 44, "uavs_newly_marked": 94, "marked_seen_in_crash_row": 53,
                  "marks_of_nobody": 27,
                  # contact calls that follow the call, no other contact call in between
                  "contact_after_set_ground_z": 8, "contact_after_set_params": 10, "contact_after_reset": 8, "contact_after_clone": 10,
                  "contact_after_set_worlds": 5, "contact_after_set_obstacles": 12,
                  # builds and hits of the third cache entry
                  "contact_grid_builds": 66, "contact_cache_hits": 27}
CONTACT_TALLIES = ("marks_behind_stall", "marks_with_open_ticket", "uavs_touching", "uavs_touching_several", "uavs_newly_marked",
                   "marked_seen_in_crash_row", "marks_of_nobody", "contact_after_set_ground_z", "contact_after_set_params",
                   "contact_after_reset", "contact_after_clone", "contact_after_set_worlds", "contact_after_set_obstacles",
                   "contact_grid_builds", "contact_cache_hits")


def contact_totals(results):
    """the figures of CONTACT_COUNTS over the results of run_sequence: calls per contact kind, those behind a pending collision tick by
    form, and what the restatement and the cache model met"""
    results = list(results)
    total = {OP_NAMES[op]: sum(r["kinds"][op] for r in results) for op in CONTACT_KINDS}
    total["contacts_behind_pending"] = sum(r["contacts_behind_pending"] for r in results)
    total["marks_behind_pending"] = sum(r["marks_behind_pending"] for r in results)
    tally = sum((r["scene"] for r in results), Counter())
    total.update({name: int(tally[name]) for name in CONTACT_TALLIES})
    return total


def surface_of(seed):
    """the surface a seed number belongs to"""
    return "base" if seed < EXT_SEED_NUMBERS[0] else "ext" if seed < 200 else "scene" if seed < 400 else "contact"


def draw_obstacles(rng):
    """an obstacle set of the scene surface: M of OBSTACLE_COUNTS records, all three kinds, every other cylinder a pillar without ends,
    centres in [-2, 11]^3 (the fleet lives in [0, 9]^3 + (0, 0, 0.5)), sizes 0.15 .. 1.0 m; from five obstacles on the last one sits about
    1e3 m away, so that the grid's outlier clamp is walked; by threes, obstacles are in world 0, carry one of the labels UAVs carry, or
    are ALL_WORLDS with a junk label"""
    M = pick(rng, OBSTACLE_COUNTS)
    idx = np.arange(M)
    ob = np.zeros(M, OBSTACLE)
    ob["kind"] = (idx + int(rng.integers(0, 3))) % 3
    ob["c"] = rng.uniform(-2.0, 11.0, (M, 3))
    ob["h"] = rng.uniform(0.15, 1.0, (M, 3))
    ob["h"][np.flatnonzero(ob["kind"] == CYLINDER)[::2], 2] = np.inf
    if M >= 5:
        ob["c"][M - 1] = rng.uniform(0.9e3, 1.1e3, 3) * rng.choice([-1.0, 1.0], 3)
    group = (idx // 3 + int(rng.integers(0, 3))) % 3
    carried = rng.choice(np.array((0, 1, 2) + WORLD_LABELS, dtype=np.int32), M)
    junk = rng.integers(-2 ** 31, 2 ** 31, M).astype(np.int32)
    ob["world"] = np.where(group == 1, carried, np.where(group == 2, junk, 0))
    ob["flags"] = np.where(group == 2, ALL_WORLDS, 0)
    return ob


def draw_beams(rng):
    """a beam pattern of the scene surface: mixed_beams(nb) with nb of BEAM_COUNTS, or a ring of eight with the straight-down beam"""
    which = int(rng.integers(0, len(BEAM_COUNTS) + 1))
    if which < len(BEAM_COUNTS):
        return mixed_beams(BEAM_COUNTS[which])
    from mrs_multirotor_simulator_amd.tensors import scan_ring
    return np.ascontiguousarray(np.concatenate([scan_ring(8), [[0.0, 0.0, -1.0]]]))


def first_difference(got, want):
    """where two arrays of one shape first differ in their bits, as text"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    raw = np.dtype(f"u{got.dtype.itemsize}")
    bad = np.argwhere(np.ascontiguousarray(got).view(raw) != np.ascontiguousarray(want).view(raw))
    at = tuple(int(v) for v in bad[0])
    return f"{len(bad)} of {got.size} values differ, the first at {at}: got {got[at]!r}, the restatement gives {want[at]!r}"


# ---- the generator -----------------------------------------------------------------------------------------------------------------

def divisors(steps, extra=()):
    return [d for d in (1, 2, 3, 4, 5, 6) if steps % d == 0] + [e for e in extra if e > 6]


def pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def f32_round(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def run_sequence(p, dev, mrs, rng, seed, fast, fleet, rtol, cap, split=False, long_rollout=False, model=False, surface="base", worlds=False):
    """one random sequence on the Pair `p`, whose product side is reached through `dev` as well.
    surface: "base" draws from the first N_OPS kinds, as ever; "ext" from EXT_KINDS as well (SET_WORLDS only with `worlds`), forces any of
    ROLLOUTS_EXT where "base" forces one of ROLLOUTS, lets the FAST_UAVS recipe force a cost-carrying tick rollout in place of its run of
    ticks half of the time and a proximity cost follow a pending tick, takes the long horizon through a tick rollout, and counts
    contact_violations at every collision pass of the oracle; "scene" is "ext" plus SCENE_KINDS (see the module docstring): its result
    also holds scene_behind_pending and, under "scene", the Counter of what the restatements and the cache model met (SCENE_TALLIES);
    "contact" is "scene" plus CONTACT_KINDS: its result also holds contacts_behind_pending, marks_behind_pending,
    obstacle_contact_violations summed over the marking calls, crashed_at_end, and CONTACT_TALLIES in the same Counter.
    worlds: the whole swarm is labelled i % 3 before the first call.
    split: host call 12 steps in runs of five to seven launches, so that the two-stream form of step_n is taken.
    long_rollout: a shorter sequence whose first rollout takes LONG_HORIZON steps.
    model: every fifth call gives the whole swarm actuator commands, through the host call, the device call or a one-step rollout in
    turn, so that the launches that follow use the model-only kernels until a call puts some UAVs under the controller cascade again;
    half of the time that call is made a rollout.
    Returns a dict: steps, the Counter of op kinds, the op log, quaternions compared up to sign, rollouts that followed a pending
    collision tick, tickets waited for, the worst cost bound relative to its cost, and the product's counters (Device.finish); for
    "ext" also the rollouts of the new kinds and the proximity costs behind a pending tick, the stalls and replayed launches inside the
    measured tick rollouts, contact_violations summed over the collision passes, and the UAVs near a quaternion branch boundary at a
    block start of a feedback on the quaternion."""
    n, n_iter = p.n, N_ITER_LONG if long_rollout else N_ITER
    contact = surface == "contact"
    scene = surface == "scene" or contact  # (the contact surface draws everything the scene surface draws)
    ext = surface == "ext" or scene        # (... and the scene surface everything the extended one draws)
    assert surface in ("base", "ext", "scene", "contact") and (ext or not worlds)
    n_ops, rollouts, drawn = N_OPS, ROLLOUTS, ()
    if ext:
        drawn = EXT_KINDS[:len(EXT_KINDS) - (0 if worlds else 1)] + (SCENE_KINDS if scene else ())  # (SET_WORLDS is the last of EXT_KINDS)
        drawn += CONTACT_KINDS if contact else ()
        n_ops, rollouts = N_OPS + len(drawn), ROLLOUTS_EXT
    kinds, oplog = Counter(), []
    tally = Counter()  # what the scene calls met, counted from the restatements
    res = dict(steps=0, kinds=kinds, log=oplog, quat_sign_cases=0, rollouts_behind_pending=0, worst_cost_ratio=0.0, tickets_waited=0,
               ext_rollouts_behind_pending=0, proximity_behind_pending=0, contact_violations=0, feedback_near_quat_branch=0, world_sets=[0, 0],
               measured_tick_rollouts=0, scene_behind_pending=0, scene=tally, contacts_behind_pending=0, marks_behind_pending=0,
               obstacle_contact_violations=0)
    pos = build_fleet(p, rng, n, fleet, seed)
    p.both("set_input", 0, n, O.POSITION_CMD, payload(rng, 10, n, pos))
    if worlds:
        p.both("set_worlds", (np.arange(n) % 3).astype(np.int32), 0)
    if scene:  # what the oracle does not have: the generator's own copies are part of the reference
        ob, beams = draw_obstacles(rng), draw_beams(rng)
        dev.set_obstacles(ob, True)
        dev.set_beams(beams, True)
        sets = [1, 1]                            # set_obstacles and set_scan_beams calls so far: the host call and the tensor call in turn
        cache = {"query": None, "scan": None}    # the model of obstacle_set.h: what each entry is current for (None: dropped)
        builds = 0                               # ... and grid_builds of the handle
        since_scan, stale = set(), 0             # SCAN_MARKS since the last scan; 1: the device table is stale, 2: ... and a blind scan ran
    if contact:
        cache["contact"] = None  # the third entry, current for fl(rmax + margin)
        # rmax: the largest arm_length + prop_radius of the airframe table, which never forgets an entry (host_api.hip: intern_type only
        # appends; mrs_swarm_clone_resized copies keys and tparams whole).  Index 0 is the default parameter set; every other entry is
        # a set some UAV held, and a call gives a UAV at most one new set, so the running maximum over the oracle's parameters after
        # every call is the table's maximum.  Never read back from the product.
        dflt = O.default_params()
        rmax = max(float(np.float64(dflt.arm_length) + np.float64(dflt.prop_radius)), float(airframes_of(p.o)[1].max()))
        since_contact = set()                    # SCAN_MARKS since the last contact call
        marked = set()                           # UAVs a CONTACT_MARK newly marked and no tick rollout's crash row has shown yet
        contact_calls, cover = 0, None                # calls so far; the UAV the range of a forced tick rollout is to cover
    if ext:  # every collision pass of the oracle, whichever call makes it
        passes = p.o.handle_collisions

        def watched(enabled, crash, rebounce):
            if enabled or crash:
                res["contact_violations"] += contact_violations(p.o, rtol)
            passes(enabled, crash, rebounce)
        p.o.handle_collisions = watched
    tickets = {"outputs": [], "poses": []}  # per kind, oldest first: (ticket, iteration it is due, the oracle's outputs of its range)
    pending, forced, long_left, ticked, stepped, model_due = False, [], long_rollout, False, False, False
    stall_at = -1  # the call at which the FAST_UAVS recipe forces a tick rollout

    def labels():
        return p.o.get_worlds() if worlds else None

    def cost_inputs(want, groups, f32):
        """targets within a few units (of each group's scale) of the rows, and weights, a row per evaluation or one for all"""
        E, w = want.shape[0], want.shape[2]
        off = rng.uniform(0.5, 3.0, want.shape) * rng.choice([-1.0, 1.0], want.shape) * group_floors(groups)
        targets = np.where(np.isfinite(want), want, 0.0) + off
        weights = rng.uniform(0.1, 2.0, (E if rng.integers(0, 2) else 1, w))
        return (f32_round(targets), f32_round(weights)) if f32 else (targets, weights)

    def cost_check(got, cost, bound, start, what):
        """a cost vector of the product against its restatement on the oracle's rows, within the first-order bound of the rows' tolerance"""
        own = cost - (0.0 if start is None else start)  # the cost of this call
        ok = np.isfinite(cost)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(own[ok] > 0, bound[ok] / own[ok], bound[ok])  # (a cost of 0 counts against the absolute bound)
        res["worst_cost_ratio"] = max(res["worst_cost_ratio"], float(ratio.max(initial=0.0)))
        if got is not None:
            assert np.array_equal(np.isfinite(got), ok), f"{what}: non-finite costs differ"
            err = np.abs(got[ok] - cost[ok])
            i = int(np.argmax(err - bound[ok])) if ok.any() else 0
            assert (err <= bound[ok]).all(), (f"{what}: cost of UAV {first + int(np.flatnonzero(ok)[i])} is off by {err[i]:.3e}, the bound is "
                                             f"{bound[ok][i]:.3e} (cost {cost[ok][i]:.6e})")

    def wait_oldest(kind, what):
        ticket, _, want = tickets[kind].pop(0)
        got = dev.async_wait(kind, ticket)
        res["tickets_waited"] += 1
        if got is not None:
            compare_outputs(got, want, fast, rtol, f"{what}: {kind} ticket {ticket}")

    def rows_check(got, want, R, groups, f32, what):
        if got is not None:
            res["quat_sign_cases"] += compare_rows(got, want, R, groups, rtol, f32, what)

    def touch(entry, key):
        """the rule of obstacle_set.h for a cache entry: current for `key`, or built anew"""
        nonlocal builds
        if cache[entry] == key:
            tally[entry + "_cache_hits"] += 1
        else:
            cache[entry], builds = key, builds + 1
            tally[entry + "_grid_builds"] += 1

    def scene_inputs():
        """what a scene call reads, fetched right before it under the call's stream context: the FP64 positions and attitudes of the whole
        swarm as the product holds them (a gather keeps a pending tick pending; the stub: the oracle's), and the oracle's labels"""
        rows = dev.gather(OBS_POS | OBS_R, 0, n, False, 0)
        if rows is None:
            rows = ref_rows(p.o, 0, n, OBS_POS | OBS_R)[0]
        return rows[:, :3], rows[:, 3:].reshape(n, 3, 3), labels()

    def airframes():
        """(ground_z, arm_length + prop_radius) per UAV, from the oracle's parameters as contact_violations takes them"""
        return airframes_of(p.o)

    def exact(got, want, label):
        assert np.array_equal(got, want), f"{label}: {first_difference(np.asarray(got, np.int64), np.asarray(want, np.int64))}"

    def bits(got, want, label):
        assert same_typed_bits(got, want), f"{label}: {first_difference(got, want)}"

    for it in range(n_iter):
        what = f"seed {seed}, call {it}"
        for kind in tickets:
            while tickets[kind] and tickets[kind][0][1] <= it:
                wait_oldest(kind, what)
        room = cap - res["steps"] - 2 * sum(1 for j in range(it, n_iter) if j % 5 == 4)  # (the two steps before every compare are kept free)
        model_due = model_due or (model and it % 5 == 0)
        was_forced, measure = bool(forced), False
        op = forced.pop(0) if forced else int(rng.integers(0, n_ops))
        if op >= N_OPS and not was_forced:
            op = drawn[op - N_OPS]  # (33 and 34 are the two kinds that are never drawn)
        blind = table = False
        if op in (SCAN_BLIND, SCAN_TABLE):  # the two scans of the stale-table shape
            blind, table = op == SCAN_BLIND, op == SCAN_TABLE
            op = RANGE_SCAN if blind or rng.integers(0, 2) else RANGE_SCAN_UAVS
        behind_stall = op == MARK_BEHIND_STALL  # the mark among the followers of the stall recipe
        if behind_stall:
            op = CONTACT_MARK
        first, count = rng_range(rng, n)
        show = False
        if contact and cover is not None:  # a tick rollout forced behind a mark: its range covers a UAV that was marked, its crash row
            if was_forced and op in (ROLL_TICK, ROLL_TICK_COST):  # is asked for and its crash cost charged
                lo, hi = min(first, cover), max(first + count, cover + 1)
                first, count, show = lo, hi - lo, True
            cover = None
        if model_due and not was_forced:  # (calls that belong together stay together)
            forced, op, first, count, model_due = [op], MODEL_ALL, 0, n, False  # (the call drawn for this turn comes next)
        x = p.o.get_state(first, count)["x"]
        # the step budget: the long rollout comes first, seven steps stay free for the first run of ticks behind fast UAVs, and a rollout
        # takes at most half of what is left then, so that stepping calls stay possible until the end of the sequence
        free = room - (LONG_HORIZON if long_left else 0 if ticked else 7)
        if split and not stepped and op != 12:
            free -= 14  # (... and, where the two-stream form of step_n is what the sequence is run for, fourteen for its first step run)
        need = {12: 14 if split else 10, 14: 7}
        stall = ext and it == stall_at
        if (op in need and free < need[op]) or (op == TICK_LONG and room < 7) or (op in ROLLOUTS and room < (LONG_HORIZON if long_left else 1)):
            op = GATHER  # no room left for the steps of this call
        elif ext and ((op in TICK_ROLLOUTS and room < (LONG_HORIZON if long_left else 7 if stall else 1))
                      or (op == ROLL_FEEDBACK and room < 1) or (long_left and (op == TICK_LONG or op in rollouts and op not in TICK_ROLLOUTS))):
            op = GATHER  # ... and the long horizon is kept for a tick rollout
        kinds[op] += 1
        oplog.append((it, OP_NAMES[op], first, count))
        if op == 12 and split:  # at least four launches behind the one that may carry a pending collision tick: the two-stream form is taken
            k, sub = int(rng.integers(5, 8)), int(rng.integers(1, 3))
            p.o.step_n(DT, k * sub)
            p.g.step_n(DT, k * sub, sub)
            res["steps"] += k * sub
            stepped = True
        elif op < 18:
            res["steps"] += host_op(p, mrs, O, rng, op, first, count, x, fast, rtol, what)
        elif op == MODEL_ALL:
            how = (it // 5) % 3 if room >= 1 else (it // 5) % 2
            pl = payload(rng, O.ACTUATOR_CMD, n, x)
            p.o.set_input(0, n, O.ACTUATOR_CMD, pl)
            if how == 0:
                p.g.set_input(0, n, O.ACTUATOR_CMD, pl)
            elif how == 1:
                dev.set_input(O.ACTUATOR_CMD, pl, 0, False, 0)
            else:
                p.o.step(DT)
                dev.rollout(O.ACTUATOR_CMD, pl[None], 0, 0, 1, 1, None, None, False, (0, 0, 0))
                res["steps"] += 1
            if rng.integers(0, 2):
                forced.insert(0, pick(rng, rollouts))
        elif op == TICK_LONG:
            k = int(rng.integers(4, 8))
            for _ in range(k):
                p.o.step(DT)
                p.o.handle_collisions(True, False, 60.0)
            p.g.tick_n(DT, k, True, False, 60.0)
            res["steps"] += k
            ticked = True
        elif op == DEV_SET_INPUT:
            mode, f32, pad = int(rng.integers(0, 11)), bool(rng.integers(0, 2)), int(rng.integers(0, 4))
            if mode == 0:
                cnt = min(count, 5)
                p.o.set_input(first, cnt, 0, None)
                dev.set_input(0, np.zeros((cnt, 1)), first, f32, pad)
            else:
                pl = payload(rng, mode, count, x)
                pl = f32_round(pl) if f32 else pl
                p.o.set_input(first, count, mode, pl)
                dev.set_input(mode, pl, first, f32, 0 if mode == O.ACTUATOR_CMD else pad)
        elif op == DEV_FORCE:
            f32, pad = bool(rng.integers(0, 2)), int(rng.integers(0, 4))
            f = rng.normal(0, 3, (count, 3))
            f = f32_round(f) if f32 else f
            p.o.apply_force(first, count, f)
            dev.apply_force(f, first, f32, pad)
        elif op == GATHER:
            groups, f32, pad = int(rng.integers(1, 256)), bool(rng.integers(0, 2)), int(rng.integers(0, 4))
            want, R = ref_rows(p.o, first, count, groups)
            rows_check(dev.gather(groups, first, count, f32, pad), want, R, groups, f32, f"{what}: gather {groups:#x}")
        elif op == CRASHED:
            got = dev.crashed(first, count)
            if got is not None:
                assert np.array_equal(got, p.o.has_crashed(first, count).astype(bool)), f"{what}: crash flags of {first}+{count}"
        elif op == RESET:
            mask = rng.random(count) < 0.3
            mask[int(rng.integers(0, count))] = True
            f32, heading, takeoff, u8 = (bool(v) for v in rng.integers(0, 2, 4))
            newpos, hd = rng.uniform(0, 9, (count, 3)) + [0, 0, 0.5], rng.uniform(-3, 3, count)
            if f32:
                newpos, hd = f32_round(newpos), f32_round(hd)
            for i in np.flatnonzero(mask):  # (runs of one UAV: every UAV is constructed with the parameters it has now)
                po = p.o.get_params(first + int(i))
                po.takeoff_patch_enabled = int(takeoff)  # the flag of the call replaces the UAV's own
                p.o.construct(first + int(i), 1, po, newpos[i:i + 1], hd[i:i + 1] if heading else None)
            dev.reset(mask, newpos, hd if heading else None, takeoff, first, f32, u8)
            if contact:  # (a reset UAV flies again)
                marked.difference_update(first + int(i) for i in np.flatnonzero(mask))
            # the oracle's construct forgets what the product's reset keeps: both sides are told all of it anew
            for lo, hi in _runs(mask):
                a, c = first + int(lo), int(hi - lo)
                p.both("set_mixer_params", a, c, desaturation=bool(rng.integers(0, 2)))
                for which in ("set_rate_params", "set_attitude_params", "set_velocity_params", "set_position_params"):
                    p.both(which, a, c, kp=float(rng.uniform(1.0, 5.0)))
                for kind in range(4):
                    p.both("set_feedforward", a, c, kind, np.concatenate([rng.uniform(-0.5, 0.5, (c, 3)), rng.uniform(-0.2, 0.2, (c, 1))], axis=1))
                p.both("set_hold", a, c, bool(rng.integers(0, 4) == 0))
                mode = int(rng.integers(1, 11))
                p.both("set_input", a, c, mode, payload(rng, mode, c, newpos[lo:hi]))
        elif op == SNAPSHOT:
            index = None
            if rng.integers(0, 2):
                index = np.where(rng.random(count) < 0.3, -1, np.arange(count)).astype(np.int32)
            status = dev.save_load(first, count, index)
            if status is not None:
                want = np.zeros(count, dtype=np.uint8) if index is None else (index < 0).astype(np.uint8)  # SNAP_LOADED 0, SNAP_SKIPPED 1
                assert np.array_equal(status, want), f"{what}: status bytes of the load"
        elif op == CLONE:
            for kind in tickets:  # (a ticket belongs to the handle that issued it)
                while tickets[kind]:
                    wait_oldest(kind, what)
            dev.clone_swap()
            if scene:  # the clone owns a set of its own: no grid built yet, every entry empty (obstacles.hip: obstacles_copy adopts the set);
                cache.update(dict.fromkeys(cache))  # it inherits the airframe table whole (mrs_swarm_clone_resized), so rmax stays
                builds = 0
        elif op == NEAREST:
            k, radius, fields, f32 = int(rng.integers(1, 9)), float(rng.uniform(0.5, 4.0)), int(rng.integers(0, 32)), bool(rng.integers(0, 2))
            dev.nearest(k, radius, fields, first, count, f32, worlds=labels())
        elif op in ROLLOUTS:
            mode, f32 = int(rng.integers(0, 11)), bool(rng.integers(0, 2))
            if long_left:
                steps, long_left = LONG_HORIZON, False
            else:
                steps = pick(rng, [h for h in HORIZONS if h <= max(1, free // 2)])
            hold = every = 1
            if op != ROLL_PLAIN:
                hold, every = pick(rng, divisors(steps)), pick(rng, divisors(steps, (steps,)))
            fhold = pick(rng, divisors(steps, (steps,))) if op == ROLL_FORCE else None
            groups = int(rng.integers(1, 256))
            if op != ROLL_COST and rng.integers(0, 5) == 0:
                groups = 0  # no observation rows at all
            pads = tuple(int(v) for v in rng.integers(0, 4, 3))
            if mode == O.ACTUATOR_CMD:
                pads = (0,) + pads[1:]  # actuator rows are dense
            if count == 1:
                pads = (0, 0, 0)  # (tensors.py takes the width of a lone row for its stride: row blocks of one padded row are not dense)
            blocks = steps // hold
            cmd = np.zeros((blocks, count, 1)) if mode == 0 else np.stack([payload(rng, mode, count, x) for _ in range(blocks)])
            forces = rng.normal(0, 3, (steps // fhold, count, 3)) if op == ROLL_FORCE else None
            if f32:
                cmd, forces = f32_round(cmd), None if forces is None else f32_round(forces)
            res["rollouts_behind_pending"] += int(pending)
            if pending and not forced and rng.integers(0, 2):
                forced.append(13)  # the rollout settles the pending tick: the next tick must not be evaluated from what that one left behind
            # the oracle's side: the loop of the header comment, literally
            want, Rs = [], []
            for t in range(steps):
                if t % hold == 0:
                    p.o.set_input(first, count, mode, cmd[t // hold] if mode else None)
                if forces is not None and t % fhold == 0:
                    p.o.apply_force(first, count, forces[t // fhold])
                p.o.step(DT)
                if groups and (t + 1) % every == 0:
                    rows, R = ref_rows(p.o, first, count, groups)
                    want.append(rows)
                    Rs.append(R)
            res["steps"] += steps
            oplog[-1] += (mode, steps, hold, every, fhold, groups, f32)
            if op != ROLL_COST:
                got = dev.rollout(mode, cmd, first, groups, hold, every, forces, fhold, f32, pads)
                if groups:
                    rows_check(got, np.array(want), np.array(Rs), groups, f32, f"{what}: {OP_NAMES[op]} of {steps} steps, mode {mode}")
            else:
                want = np.array(want)
                targets, weights = cost_inputs(want, groups, f32)
                start = rng.uniform(0.0, 5.0, count) if rng.integers(0, 3) == 0 else None
                cost = restate(want, targets, weights, start)
                bound = cost_bound(want, targets, weights, groups, rtol)
                got = dev.rollout_cost(mode, cmd, first, groups, targets, weights, hold, every, start, f32, pads)
                cost_check(got, cost, bound, start, what)
        elif op in ROLLOUTS_EXT:  # the four entry points of the extended surface
            tick, fb = op != ROLL_FEEDBACK, op in (ROLL_FEEDBACK, ROLL_TICK_FEEDBACK)
            mode, f32 = int(rng.integers(1 if fb else 0, 11)), bool(rng.integers(0, 2))  # (a feedback needs a mode with a payload)
            if long_left:
                steps, long_left = LONG_HORIZON, False
            elif stall:
                steps = pick(rng, [h for h in STALL_HORIZONS if h <= max(STALL_HORIZONS[0], free // 2)])
            else:
                steps = pick(rng, [h for h in HORIZONS if h <= max(1, free // 2)])
            ticked = ticked or stall
            hold, every = pick(rng, divisors(steps)), pick(rng, divisors(steps, (steps,)))
            blocks = steps // hold
            crash, rebounce, crash_cost = bool(rng.integers(0, 4) == 0), pick(rng, (60.0, 100.0)), pick(rng, (0.0, 2.5))
            crashed = pick(rng, ("bool", "uint8", None))
            if show:  # (the contact surface: the marked UAV must show in the crash rows, or in the cost at crash_cost a level)
                crashed, crash_cost = crashed or "uint8", crash_cost or 2.5
            # what is evaluated: observation rows (ROLL_TICK), or a cost in one of three forms: 0 a term over `groups`; 1 no cost at all
            # (ROLL_FEEDBACK, ROLL_TICK_FEEDBACK: no `out`); 2 the crash cost alone (`groups` 0: ROLL_TICK_COST; ROLL_TICK_FEEDBACK with `out`)
            groups = int(rng.integers(1, 256))
            form = 0
            if op == ROLL_TICK_COST:
                form = 2 if rng.integers(0, 5) == 0 else 0
            elif fb:
                form = int(rng.integers(0, 3 if tick else 2))
            if form or (op == ROLL_TICK and rng.integers(0, 5) == 0):
                groups = 0
            pads = tuple(int(v) for v in rng.integers(0, 4, 4))  # commands, rows or targets, weights, setpoints
            if mode == O.ACTUATOR_CMD:
                pads = (0,) + pads[1:]
            if count == 1:
                pads = (0, 0, 0, 0)
            cmd = np.zeros((blocks, count, 1)) if mode == 0 else np.stack([payload(rng, mode, count, x) for _ in range(blocks)])
            cmd = f32_round(cmd) if f32 else cmd
            if fb:
                fb_groups, per_uav, wc = int(rng.integers(1, 256)), bool(rng.integers(0, 2)), cmd.shape[2]
                wo = gather_width(fb_groups)
                scale = np.full(wo, 1e-3)  # small enough that the closed loop stays finite (test_rollout_feedback_gpu.draw)
                if fb_groups >> 7 & 1:
                    scale[-O.MAX_MOTORS:] = 1e-7  # (the rpm columns are thousands)
                Bg, Br = (blocks if rng.integers(0, 2) else 1), (blocks if rng.integers(0, 2) else 1)
                gains = rng.normal(0.0, 1.0, (Bg, wc, wo, count) if per_uav else (Bg, wc, wo)) * (scale[:, None] if per_uav else scale)
                refs = rng.normal(0.0, 2.0, (Br, 1 if rng.integers(0, 2) else count, wo))
                if f32:
                    gains, refs = f32_round(gains), f32_round(refs)
            measure = tick and not pending and (stall or rng.integers(0, 2) == 0)  # (Device._measured)
            res["measured_tick_rollouts"] += int(measure)
            res["rollouts_behind_pending"] += int(pending)
            res["ext_rollouts_behind_pending"] += int(pending)
            if pending and not forced and rng.integers(0, 2):
                forced.append(13)
            # the oracle's side: the loops of the header comments, literally
            want, Rs, crs = [], [], []
            for t in range(steps):
                if t % hold == 0:
                    if fb:  # the command of the block: nominal + G (ref - obs), from the rows before the step
                        obs, R = ref_rows(p.o, first, count, fb_groups)
                        if fb_groups >> QUAT_BIT & 1:
                            res["feedback_near_quat_branch"] += int(near_quat_branch(R).sum())
                        p.o.set_input(first, count, mode, restate_feedback(obs, cmd, gains, refs, t // hold))
                    else:
                        p.o.set_input(first, count, mode, cmd[t // hold] if mode else None)
                p.o.step(DT)
                if (t + 1) % every == 0:  # between the tick's step and its collision pass
                    if groups:
                        rows, R = ref_rows(p.o, first, count, groups)
                        want.append(rows)
                        Rs.append(R)
                    crs.append(p.o.has_crashed(first, count).astype(bool))
                if tick:
                    p.o.handle_collisions(True, crash, rebounce)
            res["steps"] += steps
            oplog[-1] += (mode, steps, hold, every, None, groups, f32)
            want, crs = (np.array(want) if groups else None), np.array(crs)
            label = f"{what}: {OP_NAMES[op]} of {steps} steps, mode {mode}"
            if op == ROLL_TICK:
                got = dev.rollout_ticks(mode, cmd, first, groups, hold, every, crash, rebounce, crashed, f32, pads[:3], measure=measure)
                if got is not None:
                    if groups:
                        rows_check(got[0], want, np.array(Rs), groups, f32, label)
                    assert got[1] is None or np.array_equal(got[1].astype(bool), crs), f"{label}: crash rows"
                    assert (got[0] is None) == (groups == 0) and (got[1] is None) == (crashed is None)
            else:
                targets = weights = start = None
                if groups:
                    targets, weights = cost_inputs(want, groups, f32)
                want_out = form != 1
                if want_out and rng.integers(0, 3) == 0:
                    start = rng.uniform(0.0, 5.0, count)
                if form == 1:
                    cost = None
                elif tick:
                    cost = restate_ticks(want, crs, targets, weights, crash_cost, start)
                else:
                    cost = restate(want, targets, weights, start)
                bound = cost_bound(want, targets, weights, groups, rtol) if groups else np.zeros(count)  # (the crash cost alone: exact)
                if op == ROLL_TICK_COST:
                    got = dev.rollout_tick_cost(mode, cmd, first, groups, targets, weights, crash_cost, hold, every, crash, rebounce, start, f32, pads[:3],
                                                measure=measure)
                elif op == ROLL_FEEDBACK:
                    got = dev.rollout_feedback(mode, cmd, first, fb_groups, gains, refs, groups, targets, weights, hold, every, start, want_out, f32, pads)
                else:
                    got = dev.rollout_tick_feedback((crash, rebounce, crash_cost), mode, cmd, first, fb_groups, gains, refs, groups, targets, weights,
                                                    hold, every, start, want_out, f32, pads, measure=measure)
                if cost is not None:
                    cost_check(got, cost, bound, start, label)
                else:
                    assert got is None, f"{label}: a run without a cost returned one"
            if contact and tick and marked and (crashed is not None if op == ROLL_TICK else cost is not None and crash_cost != 0.0):
                # UAVs a contact mark crashed, in the first crash row of a rollout that hands the rows out or charges for them
                seen = {u for u in marked if first <= u < first + count and crs[0][u - first]}
                tally["marked_seen_in_crash_row"] += len(seen)
                marked.difference_update(seen)
        elif op == PROXIMITY:
            k, radius, kind = int(rng.integers(1, 33)), float(rng.uniform(0.5, 4.0)), int(rng.integers(0, 3))
            weight, eps, found = float(rng.uniform(0.1, 2.0)), pick(rng, (0.0, 0.01)), bool(rng.integers(0, 2))
            start = rng.uniform(0.0, 5.0, count) if rng.integers(0, 2) else None
            res["proximity_behind_pending"] += int(pending)
            oplog[-1] += (k, kind)
            # the reference reads what the call reads: the product's FP64 positions (a gather keeps a pending tick pending) and the labels
            # (the oracle's: the product's own getter enters like a state call; the two are compared at every compare)
            xs = dev.gather(OBS_POS, 0, n, False, 0)
            got = dev.proximity_cost(k, radius, kind, weight, eps, first, count, start, found)
            if got is not None:
                term, nfound = proximity_ref(xs, first, count, k, radius, kind, weight, eps, worlds=labels())
                assert same_bits(got[0], add_bits(start, term)), f"{what}: proximity cost, kind {kind}, k {k}, radius {radius}"
                assert (got[1] is None) == (not found) and (got[1] is None or np.array_equal(got[1], nfound)), f"{what}: proximity cost: found"
        elif op == SET_WORLDS:
            whole = rng.integers(0, 6) == 0
            if whole:
                first, count = 0, n
            w = np.full(count, pick(rng, WORLD_LABELS), dtype=np.int32) if whole else rng.choice(np.array(WORLD_LABELS, dtype=np.int32), count)
            how = sum(res["world_sets"]) % 2  # the host call on both sides, or the device call on the product's, in turn
            res["world_sets"][how] += 1
            if how == 0:
                p.both("set_worlds", w, first)
            else:
                p.o.set_worlds(w, first)
                dev.set_worlds(w, first)
        elif op == SET_OBSTACLES:
            ob = draw_obstacles(rng)
            dev.set_obstacles(ob, sets[0] % 2 == 0)
            sets[0] += 1
            cache.update(dict.fromkeys(cache))  # every entry served the old set; the setter itself builds nothing
            oplog[-1] += (len(ob),)
        elif op == SET_BEAMS:
            beams = draw_beams(rng)
            dev.set_beams(beams, sets[1] % 2 == 0)
            sets[1] += 1
            oplog[-1] += (len(beams),)
        elif op in (NEAREST_OBSTACLES, OBSTACLE_COST):
            # k: the largest one time in six, a small one (more obstacles within the radius than slots) two times, else any
            k = (32, 0, 0, 33, 33, 33)[int(rng.integers(0, 6))]
            k = k if k == 32 else int(rng.integers(1, 5)) if k == 0 else int(rng.integers(1, 33))
            radius = pick(rng, PALETTE)
            fields, f32, pads = int(rng.integers(0, 8)), bool(rng.integers(0, 2)), tuple(int(v) for v in rng.integers(0, 4, 2))
            kind, weight, found = pick(rng, (0, 2)), float(rng.uniform(0.1, 2.0)), bool(rng.integers(0, 2))  # PROX_HINGE2, PROX_COUNT
            start = rng.uniform(0.0, 5.0, count) if rng.integers(0, 2) else None
            oplog[-1] += (k, radius)
            sl = slice(first, first + count)
            xs, Rs, lab = scene_inputs()
            ref = restate_obstacles(xs, Rs, lab, ob, k, radius)
            tally["found_over_k"] += int((ref["found"][sl] > k).sum())
            tally["found_none"] += int((ref["found"][sl] == 0).sum())
            touch("query", radius)
            if op == NEAREST_OBSTACLES:
                label = f"{what}: nearest_obstacles of {first}+{count}, k {k}, radius {radius}, fields {fields}, {'FP32' if f32 else 'FP64'}"
                got = dev.nearest_obstacles(k, radius, fields, first, count, f32, pads)
                if got is not None:
                    exact(got[2], ref["count"][sl], label + ": counts")
                    exact(got[1], ref["index"][sl], label + ": index")
                    if fields:
                        bits(got[0], restate_rows({key: v[sl] for key, v in ref.items()}, fields, np.float32 if f32 else np.float64), label + ": rows")
            else:
                label = f"{what}: obstacle_cost of {first}+{count}, k {k}, radius {radius}, kind {kind}"
                got = dev.obstacle_cost(k, radius, kind, weight, first, count, start, found)
                if got is not None:
                    bits(got[0], obstacle_add_bits(start, restate_cost(ref, k, radius, kind, weight)[sl]), label + ": cost")
                    assert (got[1] is None) == (not found), label
                    if found:
                        exact(got[1], ref["found"][sl], label + ": found")
        elif op in SCANS:
            see = op == RANGE_SCAN_UAVS
            max_range, pads = pick(rng, PALETTE), tuple(int(v) for v in rng.integers(0, 4, 3))
            body, ground, f32, hits, uavs = (bool(v) for v in rng.integers(0, 2, 5))
            ground = (ground or (table and not see)) and not blind  # (the stale-table shape: a scan that reads no table, then one that does)
            uavs = uavs and see
            flags = (BODY_FRAME if body else 0) | (GROUND if ground else 0)
            oplog[-1] += (max_range, flags, len(beams))
            sl = slice(first, first + count)
            xs, Rs, lab = scene_inputs()
            gz, rad = airframes()
            base = restate_scan(xs, Rs, lab, ob, beams, max_range, body)
            if see:
                want = restate_scan_uavs(xs, Rs, lab, rad, ob, beams, max_range, body, ground_z=gz if ground else None, base=base)
                alone = restate_scan_uavs(xs, Rs, lab, rad, NO_OBSTACLES, beams, max_range, body)  # (what the UAVs alone would take)
                tally["uav_takes_from_obstacle"] += int(((want[1][sl] == HIT_UAV) & (base[1][sl] >= 0)).sum())
                tally["obstacle_keeps_from_uav"] += int(((want[1][sl] >= 0) & (alone[1][sl] == HIT_UAV)).sum())
            else:
                want = (restate_scan(xs, Rs, lab, ob, beams, max_range, body, ground_z=gz, base=base) if ground else base) + (None,)
            h = want[1][sl]
            for kind, name in enumerate(("hit_sphere", "hit_box", "hit_cylinder")):
                tally[name] += int((ob["kind"][h[h >= 0]] == kind).sum())
            for value, name in ((HIT_UAV, "hit_uav"), (HIT_GROUND, "hit_ground"), (HIT_NONE, "hit_none")):
                tally[name] += int((h == value).sum())
            tally["range_zero"] += int((want[0][sl] == 0.0).sum())
            for mark in since_scan:
                tally["scan_after_" + mark] += 1
            since_scan.clear()
            touch("scan", max_range)
            label = (f"{what}: {OP_NAMES[op]} of {first}+{count}, {len(beams)} beams, max_range {max_range}, flags {flags}, "
                     f"{'FP32' if f32 else 'FP64'}")
            got = dev.range_scan(see, max_range, flags, first, count, f32, len(beams), pads, hits, uavs)
            if got is not None:
                bits(got[0], want[0][sl].astype(np.float32 if f32 else np.float64), label + ": ranges")
                if hits:
                    exact(got[1], want[1][sl], label + ": hit")
                if uavs:
                    exact(got[2], want[2][sl], label + ": uav")
        elif op in CONTACT_KINDS:
            mark = op == CONTACT_MARK
            margin = pick(rng, MARK_MARGINS if mark else MARGINS)
            outs = tuple(name for name, on in zip(CONTACT_OUTPUTS, rng.integers(0, 2, 4)) if on)
            start = rng.uniform(0.0, 5.0, count) if rng.integers(0, 2) else None
            hit_cost = float(rng.uniform(0.5, 5.0))
            if mark and rng.integers(0, 4) == 0:
                outs, start = (), None  # the mark alone, one time in four
            elif not mark and not outs and start is None:
                outs = (pick(rng, CONTACT_OUTPUTS),)  # ("nothing to do" is refused: the read-only form asks for something)
            fill, contact_calls = contact_calls % 2 == 0, contact_calls + 1  # vectors to fill and True in turn
            oplog[-1] += (margin, outs, start is not None)
            res["marks_behind_pending" if mark else "contacts_behind_pending"] += int(pending)
            sl = slice(first, first + count)
            rad = airframes()[1]
            # What the kernel reads: the positions behind the launches queued so far.  A gather before the call sees them (it drains
            # like the read-only form; and the marking form's settle() evaluates the pending tick through collide_now, which reads
            # positions and writes forces and flag words, never a position: tick_single.hip).  Behind the stall recipe the gather comes
            # after the call instead, so that the mark itself is what has to replay the stall: the mark writes flag words only, so
            # the positions it read are still there.
            if not behind_stall:
                xs, _, lab = scene_inputs()
            touch("contact", float(np.float64(rmax) + np.float64(margin)))
            label = f"{what}: {OP_NAMES[op]} of {first}+{count}, margin {margin}, outputs {outs}, {'vectors to fill' if fill else 'new vectors'}"
            got = dev.obstacle_contacts(margin, mark, first, count, outs, fill, start, hit_cost)
            if behind_stall:
                xs, _, lab = scene_inputs()
            ref = restate_contacts(xs, lab, ob, rad, margin)
            hit = ref["hit"][sl] != 0
            tally["uavs_touching"] += int(hit.sum())
            tally["uavs_touching_several"] += int((ref["count"][sl] > 1).sum())
            for name in since_contact:
                tally["contact_after_" + name] += 1
            since_contact.clear()
            if got is not None:
                assert sorted(got) == sorted(outs + (("cost",) if start is not None else ())), label
                for name in outs:
                    if name == "sd":
                        bits(got["sd"], ref["sd"][sl], label + ": sd")
                    else:
                        exact(got[name], ref["count" if name == "counts" else name][sl], f"{label}: {name}")
                if start is not None:  # (bit for bit: the elements of UAVs that touch nothing keep theirs)
                    bits(got["cost"], cost_after(start, {"hit": ref["hit"][sl]}, hit_cost), label + ": cost")
            if mark:
                # the oracle has no obstacles: the touching set of the restatement on its own positions is crashed as Swarm.crash() does
                res["obstacle_contact_violations"] += obstacle_contact_violations(p.o, ob, rad, margin, first, count, rtol)
                own = restate_contacts(p.o.get_state()["x"], lab, ob, rad, margin)["hit"][sl] != 0 if dev.real else hit
                assert np.array_equal(hit, own), (
                    f"{label}: the product's positions touch UAVs {first + np.flatnonzero(hit & ~own)} that the oracle's do not, and not "
                    f"{first + np.flatnonzero(own & ~hit)} that the oracle's do, although no pair of the range is within 2 sqrt(3) delta of "
                    f"its threshold (obstacle_contact_violations is {res['obstacle_contact_violations']} so far)")
                new = own & ~p.o.has_crashed(first, count).astype(bool)
                for lo, hi in _runs(own):
                    p.o.crash(first + int(lo), int(hi - lo))
                tally["uavs_newly_marked"] += int(new.sum())
                tally["marks_of_nobody"] += int(not own.any())
                tally["marks_behind_stall"] += int(behind_stall)
                tally["marks_with_open_ticket"] += int(any(tickets.values()))
                marked.update(first + int(i) for i in np.flatnonzero(new))
                if new.any() and not forced and rng.integers(0, 2):  # the crash row and the level crash cost of the next tick rollout
                    forced.append(pick(rng, (ROLL_TICK, ROLL_TICK_COST)))
                    cover = first + int(pick(rng, np.flatnonzero(new)))
        elif op in (ASYNC_OUTPUTS, ASYNC_POSES):
            kind = "outputs" if op == ASYNC_OUTPUTS else "poses"
            if len(tickets[kind]) == 2:
                wait_oldest(kind, what)
            want = p.o.get_outputs(first, count).copy()
            ticket, due = dev.async_issue(kind, first, count), it + int(rng.integers(1, 7))
            if contact and not forced and rng.integers(0, 2):  # a mark while the ticket is open: its payload stays the state at issue
                forced.append(CONTACT_MARK)
                due = max(due, it + 2)
            tickets[kind].append((ticket, due, want))
        elif op == FAST_UAVS:  # the stall recipe: a handful of UAVs fast enough to leave their skin within two steps
            cnt = min(count, 6)
            st = p.o.get_state(first, cnt)
            st["v"][:] = [0.0, 170.0, 0.0]
            p.both("set_state", first, cnt, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
            # ... then a run of ticks that stalls, and two of the calls that must replay it and leave its last tick pending
            # (the extended surface, half of the time: a cost-carrying tick rollout of at least four ticks stalls instead — a replayed launch
            # adds to the caller's cost vector once)
            ticks = TICK_LONG
            if ext and rng.integers(0, 2):
                ticks, stall_at = pick(rng, STALL_ROLLOUTS), it + 1
            forced += [ticks] + [pick(rng, STALL_FOLLOWERS) for _ in range(2)]
            # (the contact surface, half of the time behind a run of ticks: one of the two is a marking contact call, which has to replay
            # the stall before it marks, and whose marks no replayed launch may lose)
            if contact and ticks == TICK_LONG and rng.integers(0, 2):
                forced[-1 - int(rng.integers(0, 2))] = MARK_BEHIND_STALL
        if op == 14 and not forced and rng.integers(0, 3) == 0:
            forced.append(pick(rng, rollouts))  # a rollout right behind the pending tick of a run
        if scene and op in SCENE_KINDS + CONTACT_KINDS:
            res["scene_behind_pending"] += int(pending and op in SCENE_KINDS)
            got = dev.grid_builds()
            assert got is None or got == builds, (f"{what}: {OP_NAMES[op]}: grid_builds is {got}, the cache rule of obstacle_set.h gives {builds} "
                                                  f"(entries current for {cache})")
        if ext and op in (13, 14, ROLL_TICK) and not measure and not forced and rng.integers(0, 2):
            # a call that promises to leave the pending tick alone, right behind one
            forced.append(pick(rng, SCENE_KINDS) if scene and rng.integers(0, 2) else PROXIMITY)
            if contact and rng.integers(0, 2):  # either contact form: the read-only one keeps the tick pending, the mark evaluates it
                forced[-1] = pick(rng, CONTACT_KINDS)
        if contact:
            rmax = max(rmax, float(airframes()[1].max()))  # (what the call has interned is in the table for good)
            if op in SCAN_MARKS:
                since_contact.add(SCAN_MARKS[op])
        if scene:
            if op in SCAN_MARKS:
                since_scan.add(SCAN_MARKS[op])
            # the stale-table shape: a call that re-interns airframe types, a range_scan that reads no table, a scan that reads it, and
            # between them nothing that uploads the table (every stepping call does)
            if op in TABLE_CALLS:
                stale = 1
            elif op == RANGE_SCAN and not ground:
                stale = 2 if stale else 0
            elif op in SCANS:
                tally["stale_table_shapes"] += int(stale == 2)
                stale = 0
            elif op not in NO_TABLE_UPLOAD:
                stale = 0
            if (op in TABLE_CALLS or op in SCAN_MARKS) and not forced and it % 5 <= 2:
                if rng.integers(0, 2):
                    forced += [SCAN_BLIND, SCAN_TABLE] if op in TABLE_CALLS else [pick(rng, SCANS)]  # (the compare's steps do not come between)
                elif contact:  # the other half: a contact call, which reads the table, the set, the labels and its own cache entry
                    forced.append(pick(rng, CONTACT_KINDS))
        if op in (13, 14, TICK_LONG) or (op in TICK_ROLLOUTS and not measure):
            pending = True
        elif op not in KEEP_PENDING and not (op == MODEL_ALL and how < 2):
            pending = False
        if it % 5 == 4:
            p.step(DT, 2)
            res["steps"] += 2
            pending = False
            if scene:
                stale = 0
            if dev.real:
                check(p, rtol, f"{what} ({it + 1} calls)")
                if ext:
                    assert np.array_equal(p.g.get_worlds(), p.o.get_worlds()), f"{what} ({it + 1} calls): world labels"
                if scene:
                    got_ob, got_beams = dev.scene_state()
                    assert got_ob.tobytes() == ob.tobytes(), f"{what} ({it + 1} calls): get_obstacles() is not the set that was given"
                    assert got_beams.tobytes() == beams.tobytes(), f"{what} ({it + 1} calls): get_scan_beams() is not the pattern that was given"
    for kind in tickets:
        while tickets[kind]:
            wait_oldest(kind, f"seed {seed}, end")
    assert res["steps"] <= cap, (res["steps"], cap)
    assert not long_left, "the long rollout did not happen"
    if ext:
        del p.o.handle_collisions  # (the watched one)
    res["stats"] = dev.finish()
    res["crashed_at_end"] = int(p.o.has_crashed().astype(bool).sum())
    res["stalls_in_tick_rollouts"], res["replayed_in_tick_rollouts"] = (int(v) for v in dev.tick_rollout_stats)
    return res
