"""The kernel pair a plain FAST run takes above 2048 blocks, at the smallest shape that can still go wrong.

Above 2048 blocks (step_regimes.py: the "w3" regime) a FAST step() is a launch of the three-wave mrs_uav_model_step_buf_w3 while a
fused step_n() is launches of the two-wave mrs_uav_model_step_buf_fuseD: two instantiations with different register budgets
(launch bounds (64, 3) and SU = 1 against (64, MRS_WAVES_PER_SIMD) and SU = MRS_SU).  The size-regime cases of
test_run_fusion_gpu.py ([131072-*], [131073-*]) show that the launcher really takes that pair; this module holds the pair itself
together on 191 UAVs (three blocks, a ragged tail) by forcing the kernels through the launcher's process-wide switches, in child
processes started one at a time through test_step_variants_gpu.run_child (and under its rule: after a child that died, nothing more
is started on the GPU):

  child A  MRS_THREE_WAVES=1                     K x step()   -> *_buf_w3 launches (forcing three waves also switches fusion off)
  child B  MRS_NT_ACCESSES=0                     step_n(K)    -> *_buf_fuseD launches and a *_buf remainder
  child C  MRS_NT_ACCESSES=0, MRS_RUN_FUSION=0   step_n(K)    -> *_buf launches

from identical seeded inputs, K = 1, 2, 3, 4, 5, 9, 19, both flavours, with UAVs on hold, under the take-off patch, above the ground
plane, with a split v_prev, under an external force and crashed.  B == C is the promise of run fusion in this process layout; A
against B is the production pairing, and a failure of the size-regime cases that shows here too lies in the kernels, not in the
launcher.

Which case holds which FAST regime of step_regimes.regime() (LITERAL is "buf" at every size).  F: run fusion against single steps,
test_run_fusion_gpu.py::test_fused_runs_equal_single_steps; I: IMU elision against single steps, test_run_imu_elision_gpu.py, where
"regimes" is test_run_equals_single_steps_in_the_two_wave_and_three_wave_regimes:
  nt      F [37-fast] .. [66000-fast]         I model-only: test_run_equals_single_steps_on_a_two_stream_swarm[None-fast] (66 000);
                                                cascade: test_run_equals_single_steps_position_cascade[2048-fast]
  buf     F [122000-fast], [131072-fast]      I model-only: regimes[model-131072-fast]; cascade: regimes[position-57601-fast],
                                                test_run_equals_single_steps_position_cascade[66000-fast]
  w3      F [131073-fast], and this module    I model-only: regimes[model-131073-fast]; cascade: regimes[position-131073-fast]
  hbm_nt  no bit-identity case, and that is decided: from 3.4 M UAVs (1.8 M with the cascade) the launchers pair the same two kernels
          as in the small-swarm nt regime (one rule for both launchers, step_kernel_choice), which the cases of the first row hold
          bit for bit, and test_bench_launch_gpu.py runs 4 M model-only and 2 M cascade UAVs in the run form against the oracle.  A
          case here would cost swarms of 3.4 M UAVs in every run of the suite for a kernel pair that is already held."""
import numpy as np
import pytest

import step_regimes as R
import test_step_variants_gpu as V
from helpers import random_state
from test_run_fusion_gpu import D, launches, same, view

pytestmark = pytest.mark.gpu
DT = 0.001
N = 191  # three blocks, the last one with 63 lanes
KS = (1, 2, 3, D, D + 1, 2 * D + 1, 4 * D + 3)
ARITHS = {"literal": 0, "fast": 1}  # mrs_multirotor_simulator_amd.ARITH_*
FORMS = {
    "w3_steps": {"MRS_THREE_WAVES": "1"},
    "fused_run": {"MRS_NT_ACCESSES": "0"},
    "unfused_run": {"MRS_NT_ACCESSES": "0", "MRS_RUN_FUSION": "0"},
}
# the groups of the scenario (hold crosses the border of blocks 0 and 1, ground and free UAVs share the ragged tail block)
PATCH, HOLD, SPLIT, FORCED, CRASHED, GROUND = slice(0, 30), slice(40, 80), slice(85, 115), slice(120, 150), slice(155, 170), slice(172, 184)
FLAGS_OF = range(0, 36, 5)
Z_ABOVE = 1.5e-3  # with v_z = -1 m/s and dt = 1 ms: above the clamp height after one step, below it after two

_cache = {}


def scenario():
    """the same in every process (seeded): start state, commands, the replaced velocities and the forces"""
    rng = np.random.default_rng(191)
    st = random_state(rng, N, 4)
    act = rng.uniform(0.35, 0.60, (N, 4))
    spawn = st["x"].copy()
    for sl in (PATCH, GROUND):  # idle motors, sinking: the patch group from 1.5 mm above its spawn height, the ground group above z = 0
        st["v"][sl] = [0.0, 0.0, -1.0]
        st["omega"][sl] = 0.0
        st["motor_rpm"][sl] = 0.0
        act[sl] = 0.0
    st["x"][PATCH, 2] += Z_ABOVE
    st["x"][GROUND, 2] = Z_ABOVE
    return dict(st=st, act=act, spawn=spawn, v_new=rng.normal(0, 2, (SPLIT.stop - SPLIT.start, 3)),
                force=rng.normal(0, 3, (FORCED.stop - FORCED.start, 3)))


def build(M, ar, sc):
    """one swarm in the scenario's start state"""
    def params(patch):
        return M.model_params("x500", ground_enabled=True, ground_z=0.0, takeoff_patch_enabled=patch)

    g = M.Swarm(N, arith=ar)
    g.construct(0, N, params(True), sc["spawn"], np.zeros(N))
    cnt = GROUND.stop - GROUND.start  # no take-off patch here, so that the ground plane is what clamps them
    g.construct(GROUND.start, cnt, params(False), sc["spawn"][GROUND], np.zeros(cnt))
    st = sc["st"]
    g.set_state(0, N, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    g.set_input(0, N, M.ACTUATOR_CMD, sc["act"])
    g.set_state(SPLIT.start, SPLIT.stop - SPLIT.start, None, sc["v_new"], None, None, None)  # v replaced, v_prev kept
    g.set_hold(HOLD.start, HOLD.stop - HOLD.start, True)
    g.apply_force(FORCED.start, FORCED.stop - FORCED.start, sc["force"])
    g.crash(CRASHED.start, CRASHED.stop - CRASHED.start)
    return g


def child_main(kind, form, out_path):
    """every K of KS from the start state, in both flavours, in the form the process's switches force"""
    import mrs_multirotor_simulator_amd as M
    M.load_library()
    sc, res = scenario(), {}
    for arith, ar in ARITHS.items():
        for k in KS:
            g = build(M, ar, sc)
            g.set_profiling(1)
            if k == KS[0]:
                for f, a in view(g, FLAGS_OF).items():
                    res[f"{arith}__start__{f}"] = a
            if form == "w3_steps":
                n_launches = 0
                for _ in range(k):
                    g.step(DT)
                    n_launches += g.last_step_kernel_ms()[1]
            else:
                g.step_n(DT, k)
                n_launches = g.last_step_kernel_ms()[1]
            for f, a in view(g, FLAGS_OF).items():
                res[f"{arith}__{k}__{f}"] = a
            d = g.get_diag()
            res[f"{arith}__{k}__diag"] = np.array([d[key] for key in V.DIAG_KEYS], dtype=np.int64)
            res[f"{arith}__{k}__launches"] = np.array(n_launches)
    np.savez(out_path, **res)


def child(form, tmp_path_factory):
    if form not in _cache:
        _cache[form] = V.run_child("pair", form, FORMS[form], tmp_path_factory.mktemp("regimes"), module="test_step_regimes_gpu")
    return _cache[form]


def unpack(res, arith, k):
    pre = f"{arith}__{k}__"
    return {f[len(pre):]: a for f, a in res.items() if f.startswith(pre)}


def ulps(x, y):
    """distance of two float64 arrays in units in the last place, element by element (exact: Python integers)"""
    def ordered(a):
        i = np.ascontiguousarray(a, dtype=np.float64).view(np.int64).ravel().astype(object)
        return np.array([-(int(v) & 0x7FFFFFFFFFFFFFFF) if v < 0 else int(v) for v in i], dtype=object)
    return np.abs(ordered(x) - ordered(y))


def difference_table(a, b, what):
    """prints, for every field, the number of differing elements and the largest difference in ulps; the fields that differ"""
    bad = []
    for f in a:
        if same(a[f], b[f]):
            continue
        bad.append(f)
        if a[f].dtype == np.float64:
            u = ulps(a[f], b[f])
            print(f"{what}: {f}: {int((u > 0).sum())} of {u.size} elements differ, largest difference {int(u.max())} ulp")
        else:
            print(f"{what}: {f}: {int((np.asarray(a[f]) != np.asarray(b[f])).sum())} of {np.asarray(a[f]).size} elements differ")
    if not bad:
        print(f"{what}: every field bit-identical")
    return bad


@pytest.mark.parametrize("arith", list(ARITHS))
def test_fused_run_equals_unfused_run_in_child_processes(mrs, tmp_path_factory, arith):
    """B == C: the promise of run fusion (fused two-wave launches against the two-wave single-step kernel), in this process layout;
    and the launches were the ones this module is about"""
    V._alive()
    b, c, a = child("fused_run", tmp_path_factory), child("unfused_run", tmp_path_factory), child("w3_steps", tmp_path_factory)
    for k in KS:
        vb, vc = unpack(b, arith, k), unpack(c, arith, k)
        assert int(vb.pop("launches")) == launches(k) and int(vc.pop("launches")) == k and int(unpack(a, arith, k)["launches"]) == k, k
        bad = difference_table(vb, vc, f"fused run vs MRS_RUN_FUSION=0, K={k}, {arith}")
        assert not bad, f"K={k}, {arith}: {bad} differ between the fused run and the run with one launch per step"


@pytest.mark.parametrize("arith", list(ARITHS))
def test_three_wave_single_steps_equal_the_fused_run(mrs, tmp_path_factory, arith):
    """A against B: K three-wave single steps against the fused two-wave run, the pairing of step() and step_n() above 2048 blocks.
    Bit for bit in both flavours; the table of differences is printed for every K before anything is asserted."""
    V._alive()
    a, b = child("w3_steps", tmp_path_factory), child("fused_run", tmp_path_factory)
    start = unpack(a, arith, "start")
    assert not difference_table(start, unpack(b, arith, "start"), f"start state, {arith}")
    failed = {}
    for k in KS:
        va, vb = unpack(a, arith, k), unpack(b, arith, k)
        va.pop("launches"), vb.pop("launches")
        bad = difference_table(va, vb, f"three-wave single steps vs fused run, K={k}, {arith}")
        if bad:
            failed[k] = bad
        # the scenario did what it is there for, in both children
        for v in (va, vb):
            for f in ("x", "v", "R", "omega", "motor_rpm", "imu"):
                assert same(v[f][HOLD], start[f][HOLD]), f"K={k}: a UAV on hold must keep {f}"
            assert np.all(v["crashed"][CRASHED] == 1) and v["crashed"].sum() == CRASHED.stop - CRASHED.start
            assert np.abs(v["fext"][FORCED]).min() > 0
            assert same(v["v"][SPLIT], v["v_prev"][SPLIT]) and not same(start["v"][SPLIT], start["v_prev"][SPLIT])
            if k == 1:  # still falling after one step ...
                assert np.all(v["v"][GROUND][:, 2] < 0) and np.all(v["x"][GROUND][:, 2] > 0) and np.all(v["v"][PATCH][:, 2] < 0)
            else:       # ... at rest from the second on: clamped inside a fused launch
                assert np.all(v["v"][GROUND] == 0) and np.all(v["x"][GROUND][:, 2] == 0) and np.all(v["v"][PATCH] == 0)
            moving = np.r_[SPLIT, FORCED, 184:N]
            assert np.all(np.isfinite(v["imu"])) and (v["imu"][moving] != start["imu"][moving]).any(axis=1).all()
    assert not failed, f"{arith}: three-wave single steps and the fused run differ, K -> fields: {failed}"


def test_the_forced_pair_is_the_one_the_launcher_takes():
    """what ties this module to the sizes: in the w3 regime single steps are three-wave launches and the run still fuses (two-wave)"""
    assert R.regime(R.N_W3_FIRST, True, False) == "w3" and R.fuses(R.N_W3_FIRST, True, False) and not R.fused_nt(R.N_W3_FIRST, True)
    assert R.regime(N, True, False) == "nt" and R.blocks(N) == 3 and N % 64 == 63
