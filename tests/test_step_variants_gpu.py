"""Every step-kernel entry point of step_device.inc, in both arithmetic flavours, against the CPU oracle in all 11 input modes.

Two launchers choose among 24 kernels (each built LITERAL and FAST): mrs_launch_step by swarm size (three-wave and non-temporal
forms), state size (buffer or 64-bit pointer addressing), cascade or model-only, and mixed-airframe blocks; mrs_launch_step_coll
(fused collision ticks) the same, and for a shard of a sharded swarm the part of a split tick it runs.  The choices a process makes
once (MRS_THREE_WAVES, MRS_NT_ACCESSES, MRS_NO_BUFFER_ADDRESSING) are forced in child processes, started one at a time; the
per-swarm ones (MRS_SHARD_SPLIT*) in this process.  The oracle runs once, in this process.

  * single GPU: one swarm of 2583 UAVs (ragged tail): x500, f550 and naki in uniform blocks, a region of mixed-airframe blocks, all
    11 modes in runs of 5-7 UAVs plus a few single-mode blocks, feed-forwards, inverted attitudes in ACCELERATION_HDG_CMD (NaN
    throttle), non-finite velocities (rollback; FAST repeats the wave), UAVs resting on the ground plane; and an all-ACTUATOR_CMD
    copy of it (model-only kernels).  Forms: step_n with one substep, step_n with fused substeps, tick_n with collisions in both
    crash modes.  LITERAL must be bit-identical across the kernel variants and within RTOL_LITERAL of the oracle; FAST within
    RTOL_FAST after one step and RTOL_NORTH_STAR after the run.
  * sharded: virtual shards over the loopback group (world 2 and 3, slabs), a moving swarm with fast UAVs (stalls, replays and
    searches), every mode: split ticks, serial ticks, mixed-airframe blocks (the launcher refuses the split form), model-only
    ticks, and the pointer-addressed kernels in a child process.

STEP_KERNELS maps every entry point to the test (and form) that forces it; test_step_kernel_table.py keeps the table complete."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
from helpers import RTOL_FAST, RTOL_LITERAL, RTOL_NORTH_STAR
from oracle import oracle_swarm as O
from test_export_sets_gpu import VirtualShards, moving_swarm, runs, set_inputs
from test_parity_gpu import payload_for

pytestmark = pytest.mark.gpu
DT = 0.001
REBOUNCE = 100.0
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)

# which test forces each entry point ("test[form]"; LITERAL / FAST noted where the launcher's choice differs between them); a case of
# another module is written "module::test[case]" - the three-wave kernels are also run at the sizes at which the launcher takes them
# by itself (step_regimes.py), as the launches of a run on two streams with the IMU stores switched off, and against fused runs
W3_IMU_CASE = "test_run_imu_elision_gpu::test_run_equals_single_steps_in_the_two_wave_and_three_wave_regimes"
STEP_KERNELS = {
    "mrs_uav_step": ("test_single_gpu_variant[pointer]",),
    "mrs_uav_step_buf": ("test_single_gpu_variant[default]  (LITERAL)", "test_single_gpu_variant[nt_off]  (FAST)",
                         W3_IMU_CASE + "[position-57601-fast]"),
    "mrs_uav_step_buf_w3": ("test_single_gpu_variant[three_waves]", W3_IMU_CASE + "[position-131073-fast]"),
    "mrs_uav_step_multi": ("test_single_gpu_variant[pointer]",),
    "mrs_uav_step_multi_buf": ("test_single_gpu_variant[default]",),
    "mrs_uav_model_step": ("test_single_gpu_variant[pointer]",),
    "mrs_uav_model_step_buf": ("test_single_gpu_variant[default]  (LITERAL)", "test_single_gpu_variant[nt_off]  (FAST)",
                               W3_IMU_CASE + "[model-131072-fast]"),
    "mrs_uav_model_step_buf_w3": ("test_single_gpu_variant[three_waves]", W3_IMU_CASE + "[model-131073-fast]",
                                  "test_run_fusion_gpu::test_fused_runs_equal_single_steps[131073-fast]",
                                  "test_step_regimes_gpu::test_three_wave_single_steps_equal_the_fused_run[fast]"),
    "mrs_uav_model_step_buf_nt": ("test_single_gpu_variant[nt_on]  (LITERAL)", "test_single_gpu_variant[default]  (FAST)"),
    "mrs_uav_step_buf_nt": ("test_single_gpu_variant[nt_on]  (LITERAL)", "test_single_gpu_variant[default]  (FAST)"),
    "mrs_uav_model_step_multi": ("test_single_gpu_variant[pointer]",),
    "mrs_uav_model_step_multi_buf": ("test_single_gpu_variant[default]",),
    "mrs_uav_step_coll_buf": ("test_single_gpu_variant[default]",),
    "mrs_uav_model_step_coll_buf": ("test_single_gpu_variant[default]",),
    "mrs_uav_step_coll": ("test_single_gpu_variant[pointer]",),
    "mrs_uav_step_mixed_coll": ("test_single_gpu_variant[default]",),
    "mrs_uav_step_xcoll_buf": ("test_sharded_matrix[serial]", "test_sharded_matrix[mixed]", "test_sharded_matrix[split]"),
    "mrs_uav_model_step_xcoll_buf": ("test_sharded_matrix[model]",),
    "mrs_uav_step_xcoll": ("test_sharded_pointer_kernels[pointer]",),
    "mrs_uav_step_mixed_xcoll": ("test_sharded_matrix[mixed]",),
    "mrs_uav_step_coll_bnd_buf": ("test_sharded_matrix[split]",),
    "mrs_uav_step_coll_buf_nt": ("test_sharded_matrix[split]",),
    "mrs_uav_step_mixed": ("test_single_gpu_variant[default]",),
    "mrs_uav_step_mixed_multi": ("test_single_gpu_variant[default]",),
}

# process-wide launcher switches of the single-GPU children (the default child is the LITERAL bit-identity reference)
SINGLE_FORMS = {
    "default": {},
    "three_waves": {"MRS_THREE_WAVES": "1"},
    "nt_off": {"MRS_NT_ACCESSES": "0"},
    "nt_on": {"MRS_NT_ACCESSES": "1"},
    "pointer": {"MRS_NO_BUFFER_ADDRESSING": "1"},
}
SHARDED_FORMS = ("split", "serial", "mixed", "model")
POINTER_FORMS = ("pointer",)
SWITCHES = ("MRS_THREE_WAVES", "MRS_NT_ACCESSES", "MRS_NO_BUFFER_ADDRESSING", "MRS_FORCE_MULTI", "MRS_SHARD_SPLIT",
            "MRS_SHARD_SPLIT_MIN_BLOCKS", "MRS_SHARD_SPLIT_MAX_FRACTION", "MRS_NO_BOUNDARY_KERNEL", "MRS_INTERIOR_NT", "MRS_RUN_FUSION")
ARITHS = {"literal": 0, "fast": 1}  # mrs_multirotor_simulator_amd.ARITH_*
AIRFRAMES3 = ("x500", "f550", "naki")
N_MOTORS = {"x500": 4, "f550": 6, "naki": 8}
FIELDS = ("x", "v", "v_prev", "R", "omega", "motor_rpm", "imu", "pid", "f")
DIAG_KEYS = tuple(sorted(k for k, _ in O.Diag._fields_))
CONTROLLER_SETTERS = ("set_mixer_params", "set_rate_params", "set_attitude_params", "set_velocity_params", "set_position_params")
CHILD_TIMEOUT = 300

N_SINGLE = 64 * 40 + 23
STEPS, SUB, TICKS = 24, 5, 20
N_SHARD = 3001
SHARD_TICKS = ((45, False), (1, True), (34, False))  # 80 ticks, one of them in crash mode

_dead = []     # the first child process that died by a signal or timed out: nothing more is started on the GPU
_cache = {}    # oracle runs and child results, computed once per module


def _alive():
    if _dead:
        pytest.fail(f"an earlier child process of this module died ({_dead[0]}): no further GPU process is started")


def run_child(kind, form, env_extra, tmp_dir, module="test_step_variants_gpu"):
    """child_main(kind, form) of `module` (a test module with an entry point of that name) in a fresh process under the given launcher
    switches; its results as {key: array}.  One rule for every module that starts children through here: after a child that died
    by a signal or timed out, nothing more is started on the GPU."""
    _alive()
    out = os.path.join(str(tmp_dir), f"{kind}_{form}.npz")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra)
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {TESTS!r}]; import {module} as T; "
            f"T.child_main({kind!r}, {form!r}, {out!r})")
    try:
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _dead.append(f"{kind}[{form}] timed out after {CHILD_TIMEOUT} s")
        pytest.fail(_dead[0])
    if p.returncode < 0:
        _dead.append(f"{kind}[{form}] ended by signal {-p.returncode}")
        pytest.fail(f"{_dead[0]}\n{p.stderr[-3000:]}")
    assert p.returncode == 0, p.stderr[-3000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def snapshot(sw):
    s = sw.get_state()
    s["imu"], s["pid"], s["f"] = sw.get_imu(), sw.get_pid(), sw.get_external_force()
    s["crashed"] = np.asarray(sw.has_crashed())
    d = sw.get_diag()
    s["diag"] = np.array([d[k] for k in DIAG_KEYS], dtype=np.int64)
    return s


def check_against_oracle(got, ref, rtol, what, frtol=None):
    for k in FIELDS:
        helpers.assert_close(got[k], ref[k], frtol if (k == "f" and frtol is not None) else rtol, f"{what}: {k}")
    helpers.assert_close_per_uav(got, ref, rtol, what)
    assert np.array_equal(got["crashed"], ref["crashed"]), f"{what}: crash flags"
    assert np.array_equal(got["diag"], ref["diag"]), f"{what}: diag counters {got['diag']} vs the oracle's {ref['diag']}"


# ---- single-GPU scenario ----------------------------------------------------------------------------------------------------
def single_scenario(actuator_only):
    """per-UAV airframes, start state, feed-forwards, modes and payload rows; the same in every process (seeded)"""
    rng = np.random.default_rng(2583)
    n = N_SINGLE
    af = np.empty(n, dtype=object)
    af[0:960], af[960:1600], af[1600:2240] = "x500", "f550", "naki"  # uniform blocks 0-34
    for k, a in enumerate(range(2240, n, 37)):                       # blocks 35-40: airframe runs end inside blocks
        af[a:a + 37] = AIRFRAMES3[k % 3]
    nm = np.array([N_MOTORS[a] for a in af])
    st = helpers.random_state(rng, n, 8, box=13.0, zlo=0.5, zhi=26.0, tilted=True)  # ~600 pairs within collision range
    st["motor_rpm"][np.arange(8)[None, :] >= nm[:, None]] = 0.0
    mode = np.empty(n + 11 * 7, dtype=np.int64)
    i = 0
    while i < n:  # runs of 5-7 UAVs through all 11 modes: most waves mix most modes
        for m in rng.permutation(11):
            k = int(rng.integers(5, 8))
            mode[i:i + k] = m
            i += k
    mode = mode[:n]
    for blk, m in ((2, O.INPUT_UNKNOWN), (5, O.POSITION_CMD), (7, O.ACTUATOR_CMD), (18, O.ATTITUDE_CMD), (28, O.VELOCITY_HDG_CMD),
                   (31, O.TILT_HDG_RATE_CMD)):
        mode[64 * blk:64 * blk + 64] = m
    ground = np.r_[300:340, 1650:1660, 2500:2510]
    st["x"][ground, 2] = 0.0
    st["v"][ground], st["omega"][ground], st["R"][ground] = 0.0, 0.0, np.eye(3)
    inverted = np.r_[100:104, 2300:2303]
    st["R"][inverted] = np.diag([1.0, -1.0, -1.0])
    st["v"][200, 0], st["v"][1700, 1], st["v"][2400] = np.nan, np.inf, np.nan
    if actuator_only:
        mode[:] = O.ACTUATOR_CMD
    else:
        mode[ground], mode[inverted] = O.ACTUATOR_CMD, O.ACCELERATION_HDG_CMD
    rows, ff = [None] * n, []
    for a, c, (m, name) in runs(list(zip(mode.tolist(), af.tolist()))):
        p = payload_for(O, m, rng, c, N_MOTORS[name], {"x": st["x"][a:a + c]})
        for q in range(c):
            rows[a + q] = None if p is None else p[q]
        if m >= O.VELOCITY_HDG_RATE_CMD and rng.random() < 0.5:
            kinds = (0, 1, 2, 3) if m == O.POSITION_CMD else (2, 3)
            for kind in rng.choice(kinds, int(rng.integers(1, len(kinds) + 1)), replace=False):
                ff.append((a, c, int(kind), rng.uniform(-1, 1, (c, 4))))
    for i in ground:
        rows[i] = np.full(nm[i], 0.1)  # far below hover: they stay on the ground
    if not actuator_only:
        for i in inverted:
            rows[i] = np.array([0.0, 0.0, 0.0, 0.3])  # upside down: the thrust projection goes negative, throttle NaN
    return dict(af=af, st=st, mode=mode, rows=rows, ff=ff)


def build_single(sw, sc, params_of):
    for a, c, name in runs(sc["af"].tolist()):
        sw.construct(a, c, params_of(name))
        for setter in CONTROLLER_SETTERS:  # UavSystemRos init order: controller params after construction
            getattr(sw, setter)(a, c)
    st = sc["st"]
    sw.set_state(0, N_SINGLE, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    for a, c, kind, pay in sc["ff"]:
        sw.set_feedforward(a, c, kind, pay)
    set_inputs(sw, sc["mode"], sc["rows"])


def oracle_params(name):
    return helpers.oracle_params(name, ground_enabled=True, ground_z=0.0)


def single_forms(make):
    """the snapshots every form leaves: step_n(1 substep), step_n(SUB fused substeps), tick_n with collisions in both crash modes"""
    out = {}
    g = make()
    g.step_n(DT, 1)
    out["step1"] = snapshot(g)
    g.step_n(DT, STEPS - 1)
    out["stepN"] = snapshot(g)
    g = make()
    g.step_n(DT, STEPS, SUB)  # launches of 5, 5, 5, 5 and 4 substeps
    out["multiN"] = snapshot(g)
    for crash in (False, True):
        g = make()
        g.tick_n(DT, 1, True, crash, REBOUNCE)
        out[f"tick1_{int(crash)}"] = snapshot(g)
        g.tick_n(DT, TICKS - 1, True, crash, REBOUNCE)
        out[f"tickN_{int(crash)}"] = snapshot(g)
        out[f"tickN_{int(crash)}"]["fused"] = np.array(g.fused_stats()[0])
    return out


def oracle_single(scen):
    key = ("oracle_single", scen)
    if key not in _cache:
        sc = single_scenario(scen == "model")

        def make():
            o = O.OracleSwarm(N_SINGLE)
            build_single(o, sc, oracle_params)
            return o

        out = {}
        o = make()
        o.step(DT)
        out["step1"] = snapshot(o)
        o.step_n(DT, STEPS - 1, 8)
        out["stepN"] = out["multiN"] = snapshot(o)
        for crash in (False, True):
            o = make()
            for t in range(TICKS):
                o.step(DT)
                o.handle_collisions(True, crash, REBOUNCE)
                if t == 0:
                    out[f"tick1_{int(crash)}"] = snapshot(o)
            out[f"tickN_{int(crash)}"] = snapshot(o)
        _cache[key] = out
    return _cache[key]


# ---- sharded scenario -------------------------------------------------------------------------------------------------------
SHARD_WORLD = {"split": 2, "serial": 3, "mixed": 2, "model": 3, "pointer": 2}
SHARD_KIND = {"split": "cascade", "serial": "cascade", "mixed": "mixed", "model": "model", "pointer": "cascade"}


def sharded_scenario(M, world, kind):
    """kind 'cascade': uniform 64-UAV airframe blocks in every shard, every mode; 'mixed': blocks 1-3 of every shard hold airframe
    runs of 23 UAVs (and most of the fast UAVs); 'model': every UAV ACTUATOR_CMD.  Airframes and modes follow the shards' (slab)
    order, so set_input and construct calls cover runs; per-UAV data is kept by public index."""
    from mrs_multirotor_simulator_amd.sharded import shard_range
    rng = np.random.default_rng(6000 + 10 * world + ("cascade", "mixed", "model").index(kind))
    pos, st, _ = moving_swarm(rng, N_SHARD, speed=5.0)
    order = M.slab_partition(pos, world)
    af = np.empty(N_SHARD, dtype=object)
    in_mixed = np.zeros(N_SHARD, dtype=bool)
    mode_sorted = np.empty(N_SHARD + 11 * 7, dtype=np.int64)
    i = 0
    while i < N_SHARD:
        for m in rng.permutation(11):
            k = int(rng.integers(5, 8))
            mode_sorted[i:i + k] = m
            i += k
    for r in range(world):
        lo, hi = shard_range(N_SHARD, world, r)
        k = np.arange(hi - lo)
        a = (k // 64) % 3
        if kind == "mixed":
            sel = (k >= 64) & (k < 256)
            a[sel] = (k[sel] // 23) % 3
            in_mixed[order[lo:hi][sel]] = True
        af[order[lo:hi]] = np.array(AIRFRAMES3, dtype=object)[a]
    mode = np.empty(N_SHARD, dtype=np.int64)
    mode[order] = O.ACTUATOR_CMD if kind == "model" else mode_sorted[:N_SHARD]
    # fast UAVs: their skin is used up within a dozen ticks (announced stalls, replays, searches); in the mixed form mostly in mixed blocks
    pool = np.flatnonzero(in_mixed) if kind == "mixed" else np.arange(N_SHARD)
    hot = np.concatenate([rng.choice(pool, 30, replace=False), rng.choice(N_SHARD, 10, replace=False)])
    st["v"][hot] = rng.normal(0, 1, (len(hot), 3)) * [12.0, 12.0, 4.0]
    rows = [None] * N_SHARD
    for a, c, (m, name) in runs(list(zip(mode[order].tolist(), af[order].tolist()))):
        sl = order[a:a + c]
        p = payload_for(O, m, rng, c, N_MOTORS[name], {"x": st["x"][sl]})
        for q in range(c):
            rows[sl[q]] = None if p is None else p[q]
    return dict(pos=pos, st=st, order=order, af=af, mode=mode, rows=rows, in_mixed=in_mixed)


def virtual_shards(M, form, arith):
    sc = sharded_scenario(M, SHARD_WORLD[form], SHARD_KIND[form])
    pp = {name: helpers.to_product_params(M, oracle_params(name)) for name in AIRFRAMES3}
    return sc, VirtualShards(M, SHARD_WORLD[form], sc["order"], [pp[a] for a in sc["af"]], sc["pos"], np.zeros(N_SHARD), sc["st"],
                             sc["mode"], sc["rows"], ARITHS[arith], M.EXCHANGE_EXPORT_SETS)


def shard_snapshot(vs):
    a = vs.gather()
    d = [g.get_diag() for g, _ in vs.shards]
    a["diag"] = np.array([sum(x[k] for x in d) for k in DIAG_KEYS], dtype=np.int64)
    return a


def run_sharded(vs):
    snaps = []
    for n, crash in SHARD_TICKS:
        vs.tick_n(n, True, crash, REBOUNCE)
        snaps.append(shard_snapshot(vs))
    return snaps


def oracle_sharded(M, form):
    key = ("oracle_sharded", SHARD_WORLD[form], SHARD_KIND[form])
    if key not in _cache:
        sc = sharded_scenario(M, SHARD_WORLD[form], SHARD_KIND[form])
        st = sc["st"]
        o = O.OracleSwarm(N_SHARD)
        for a, c, name in runs(sc["af"].tolist()):
            o.construct(a, c, oracle_params(name), sc["pos"][a:a + c], np.zeros(c))
        o.set_state(0, N_SHARD, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
        set_inputs(o, sc["mode"], sc["rows"])
        snaps = []
        for n, crash in SHARD_TICKS:
            for _ in range(n):
                o.step_n(DT, 1, 8)
                o.handle_collisions(True, crash, REBOUNCE)
            snaps.append(snapshot(o))
        assert snaps[-1]["crashed"].sum() > 0 and (np.abs(snaps[-1]["f"]).sum(axis=1) > 0).sum() > 30
        _cache[key] = snaps
    return _cache[key]


def check_sharded(snaps, ref, arith, what):
    done = 0
    for (n, _), a, b in zip(SHARD_TICKS, snaps, ref):
        done += n
        if arith == "literal":
            check_against_oracle(a, b, RTOL_LITERAL, f"{what}, after {done} ticks", frtol=1e-11)
        else:
            check_against_oracle(a, b, RTOL_NORTH_STAR, f"{what}, after {done} ticks")


# ---- children ---------------------------------------------------------------------------------------------------------------
def child_main(kind, form, out_path):
    import mrs_multirotor_simulator_amd as M
    M.load_library()
    res = {}
    if kind == "single":
        for arith, ar in ARITHS.items():
            for scen in ("cascade", "model"):
                sc = single_scenario(scen == "model")

                def make():
                    g = M.Swarm(N_SINGLE, arith=ar)
                    build_single(g, sc, lambda name: helpers.to_product_params(M, oracle_params(name)))
                    return g

                for snap, d in single_forms(make).items():
                    for k, v in d.items():
                        res[f"{arith}__{scen}__{snap}__{k}"] = v
    else:
        for arith in ARITHS:
            _, vs = virtual_shards(M, form, arith)
            snaps = run_sharded(vs)
            info, split = vs.info(), [g.split_stats()[0] for g, _ in vs.shards]
            vs.close()
            for t, d in enumerate(snaps):
                for k, v in d.items():
                    res[f"{arith}__{t}__{k}"] = v
            res[f"{arith}__searches"] = np.array([ci["searches"] for ci in info])
            res[f"{arith}__split"] = np.array(split)
    np.savez(out_path, **res)


def single_child(form, tmp_path_factory):
    key = ("single", form)
    if key not in _cache:
        _cache[key] = run_child("single", form, SINGLE_FORMS[form], tmp_path_factory.mktemp("variants"))
    return _cache[key]


def unpack(res, arith, scen, snap):
    pre = f"{arith}__{scen}__{snap}__"
    return {k[len(pre):]: v for k, v in res.items() if k.startswith(pre)}


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(SINGLE_FORMS))
def test_single_gpu_variant(mrs, oracle, tmp_path_factory, form):
    """one child process per launcher setting; each runs every form on the mixed-mode swarm and its all-actuator copy, in both
    flavours.  LITERAL: bit-identical to the default setting and within RTOL_LITERAL of the oracle; FAST: RTOL_FAST after one step,
    RTOL_NORTH_STAR after the run; PID columns, IMU, forces, crash flags and diag counters included."""
    _alive()
    res = single_child(form, tmp_path_factory)
    base = single_child("default", tmp_path_factory) if form != "default" else res
    for scen in ("cascade", "model"):
        ref = oracle_single(scen)
        assert ref["stepN"]["diag"][DIAG_KEYS.index("nan_rollback")] > 0
        assert ref["tickN_1"]["crashed"].sum() > 0 and (np.abs(ref["tickN_0"]["f"]).sum(axis=1) > 0).sum() > 100
        for snap in ref:
            what = f"{form}, {scen}, {snap}"
            lit, fast = unpack(res, "literal", scen, snap), unpack(res, "fast", scen, snap)
            if snap.startswith("tickN"):
                assert lit.pop("fused") > 0 and fast.pop("fused") > 0, f"{what}: no fused step + collision launch ran"
            check_against_oracle(lit, ref[snap], RTOL_LITERAL, f"LITERAL {what}")
            if form != "default":
                b = unpack(base, "literal", scen, snap)
                for k in lit:
                    assert np.array_equal(lit[k], b[k], equal_nan=True), f"LITERAL {what}: {k} differs from the default kernels"
            one = snap in ("step1", "tick1_0", "tick1_1")
            check_against_oracle(fast, ref[snap], RTOL_FAST if one else RTOL_NORTH_STAR, f"FAST {what}")


@pytest.mark.parametrize("arith", list(ARITHS))
@pytest.mark.parametrize("form", SHARDED_FORMS)
def test_sharded_matrix(mrs, oracle, monkeypatch, form, arith):
    """virtual shards in every mode: split ticks (boundary + interior kernels), serial ticks, mixed-airframe blocks inside the shards
    (the launcher refuses the split form; the mixed kernel decides stalls and warnings without a lead lane), model-only ticks"""
    _alive()
    M = mrs
    monkeypatch.setenv("MRS_SHARD_SPLIT_MIN_BLOCKS", "1")  # (read when a swarm is created: small shards take the split form too)
    monkeypatch.setenv("MRS_SHARD_SPLIT_MAX_FRACTION", "0.95")
    if form == "serial":
        monkeypatch.setenv("MRS_SHARD_SPLIT", "0")
    sc, vs = virtual_shards(M, form, arith)
    snaps = run_sharded(vs)
    info, split = vs.info(), [g.split_stats()[0] for g, _ in vs.shards]
    vs.close()
    check_sharded(snaps, oracle_sharded(M, form), arith, f"{arith} {form}")
    assert max(ci["searches"] for ci in info) >= 2, info
    if form in ("split", "model"):
        assert sum(split) > 20, split
    else:
        assert sum(split) == 0, split
    if form == "mixed":
        from mrs_multirotor_simulator_amd.sharded import shard_range
        for r in range(SHARD_WORLD[form]):
            lo, hi = shard_range(N_SHARD, SHARD_WORLD[form], r)
            blocks = [set(sc["af"][sc["order"][b:min(b + 64, hi)]]) for b in range(lo, hi, 64)]
            assert sum(len(s) > 1 for s in blocks) >= 3, f"rank {r}: no mixed-airframe blocks"


@pytest.mark.parametrize("form", POINTER_FORMS)
def test_sharded_pointer_kernels(mrs, oracle, tmp_path_factory, form):
    """MRS_NO_BUFFER_ADDRESSING=1 in a child process: the 64-bit pointer-addressed shard kernel on the cascade scenario"""
    _alive()
    ref = oracle_sharded(mrs, form)
    res = run_child("sharded", form, {"MRS_NO_BUFFER_ADDRESSING": "1", "MRS_SHARD_SPLIT": "0"}, tmp_path_factory.mktemp("variants"))
    for arith in ARITHS:
        snaps = []
        for t in range(len(SHARD_TICKS)):
            pre = f"{arith}__{t}__"
            snaps.append({k[len(pre):]: v for k, v in res.items() if k.startswith(pre)})
        check_sharded(snaps, ref, arith, f"{arith} {form}")
        assert res[f"{arith}__searches"].max() >= 2 and res[f"{arith}__split"].sum() == 0


if __name__ == "__main__":
    child_main(*sys.argv[1:4])
