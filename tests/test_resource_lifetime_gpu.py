"""Every GPU resource the library takes is given back: device buffers, pinned blocks, events and streams are held by the owners of
csrc/hip_owned.h, whose live counters (swarm.debug_live_resources) must stand above their baseline while swarms live and return to it
EXACTLY once everything is closed — after every lazily created resource of a swarm has been created, after buffers have regrown, for
sharded swarms closed with and without comm_destroy, for a peer window that never became a communicator, and for clones.

Shards of a communicator are equal-count (sizes differ by at most one), so the sharded case runs 259 UAVs as 130 + 129: two full
blocks and a tail on both ranks."""
import gc

import numpy as np
import pytest
import torch

import helpers
from test_export_sets_gpu import VirtualShards, moving_swarm

pytestmark = pytest.mark.gpu
DT = 0.001
N = 130  # two full 64-UAV blocks and a tail of two lanes


def live(M):
    return np.array(M.swarm.debug_live_resources())


def baseline(M):
    gc.collect()
    return live(M)


def make_swarm(M, arith, n=N, seed=5):
    """n x500 UAVs on a 3 m grid, every tenth one 0.5 m from its predecessor (within collision range), under actuator commands"""
    rng = np.random.default_rng(seed)
    st = helpers.random_state(rng, n, 4, tilted=True)
    pos = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3)[:n] * 3.0 + [0, 0, 30.0]
    pos[10::10] = pos[9::10][:len(pos[10::10])] + [0.5, 0.0, 0.0]
    st["x"], st["v"] = pos, rng.normal(0, 1.0, (n, 3))
    s = M.Swarm(n, arith=arith)
    s.construct(0, n, M.model_params("x500"), pos, np.zeros(n))
    s.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    s.set_input(0, n, M.ACTUATOR_CMD, rng.uniform(0.4, 0.55, (n, 4)))
    return s


@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
def test_every_lazily_created_resource_is_given_back(mrs, arith):
    from mrs_multirotor_simulator_amd import tensors as T
    M = mrs
    base = baseline(M)
    s = make_swarm(M, getattr(M, "ARITH_" + arith))
    s.step_n(DT, 4)  # second stream
    s.step_range(3, 70, DT)  # block list of a partial step
    s.tick_n(DT, 6, True, False, 100.0)  # tables, lists, fused buffers, pinned control words
    assert s.collision_stats()[1] >= 1 and np.abs(s.get_external_force()).sum() > 0
    for get, start, wait in ((s.get_outputs, s.get_outputs_async, s.outputs_wait), (s.get_poses, s.get_poses_async, s.poses_wait)):
        want = get()
        for _ in range(2):  # both slots of the kind, the copy stream
            t = [start(), start()]
            for k in t:
                assert wait(k).tobytes() == want.tobytes()
    assert len(s.get_states()) == N
    for _ in range(2):  # both staging blocks, the upload stream
        rows = s.input_staging(N, 4)
        rows[:] = 0.5
        s.commit_input(0, N, M.ACTUATOR_CMD, 4)
    s.set_profiling(2)  # the event vector
    s.step_n(DT, 3)
    assert s.last_step_kernel_ms()[1] >= 1
    s.set_profiling(0)
    obs = T.gather(s, T.OBS_POS | T.OBS_VEL)  # fence events
    rows, index, counts = T.nearest(s, 4, 5.0)  # scratch of the neighbour observations
    torch.cuda.synchronize()
    assert obs.shape == (N, 6) and int(counts.sum()) > 0
    assert s.pack_positions()[1] > 0
    assert s.debug_component(4, 0, N, np.zeros((N, 3))).shape == (N, 3)
    s.synchronize()
    mid = live(M)
    print("live resources (device, pinned, events, streams):", base, "->", mid)
    assert (mid > base).all(), (base, mid)
    assert mid[3] - base[3] == 4 and mid[1] - base[1] >= 2 + 4 + 1 + 2 + 1  # streams: step x 2, copy x 2; pinned: stages, slots, states, rows, words
    s.close()
    assert (live(M) == base).all(), (base, live(M))


def regrow_results(M, s, small_first):
    """the large calls of the regrowth case on swarm s, each preceded by its small form when small_first; the device / pinned buffer
    counts must not move over a regrow"""
    from mrs_multirotor_simulator_amd import tensors as T
    out = {}

    def regrow(name, small, large):
        if small_first:
            small()
            before = live(M)[:2]
        out[name] = large()
        if small_first:
            assert (live(M)[:2] == before).all(), (name, before, live(M)[:2])

    regrow("outputs", lambda: s.get_outputs(0, 10), lambda: s.get_outputs(0, N).tobytes())
    regrow("states", lambda: s.get_states(0, 1), lambda: s.get_states(0, N).tobytes())

    def nearest(k):
        rows, index, counts = T.nearest(s, k, 5.0)
        torch.cuda.synchronize()
        return rows.cpu().numpy().tobytes(), index.cpu().numpy().tobytes(), counts.cpu().numpy().tobytes()

    regrow("nearest", lambda: nearest(1), lambda: nearest(8))

    def stage(count, stride, mode, row):
        # (two calls: both staging blocks take the shape)
        for _ in range(2):
            rows = s.input_staging(count, stride)
            rows[:] = row
        s.commit_input(0, count, mode, stride)

    attitude = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5]  # orientation (identity) + throttle
    regrow("staging", lambda: stage(10, 4, M.ACTUATOR_CMD, 0.45), lambda: stage(N, 10, M.ATTITUDE_CMD, attitude))
    s.step_n(DT, 3)
    out["after"] = s.get_states().tobytes()
    return out


def test_regrown_buffers_replace_the_old_ones(mrs):
    M = mrs
    base = baseline(M)
    fresh = make_swarm(M, M.ARITH_LITERAL)
    want = regrow_results(M, fresh, small_first=False)
    fresh.close()
    assert (live(M) == base).all()
    s = make_swarm(M, M.ARITH_LITERAL)
    # the small staging rows of the regrown swarm command 10 UAVs before the large ones command all: the fresh swarm gets the same
    got = regrow_results(M, s, small_first=True)
    assert (live(M) > base).all()
    for k in ("outputs", "states", "nearest"):
        assert got[k] == want[k], k
    # (after the staged commands the two swarms differ in the 10 UAVs' earlier actuator command, which the attitude command replaced
    #  before any step ran: the states after the steps are equal too)
    assert got["after"] == want["after"]
    s.close()
    assert (live(M) == base).all(), (base, live(M))


@pytest.mark.parametrize("comm_destroy_first", [True, False])
def test_sharded_swarms_give_everything_back(mrs, comm_destroy_first):
    M = mrs
    base = baseline(M)
    n_total = 259  # 130 + 129
    rng = np.random.default_rng(11)
    pos, st, cmd = moving_swarm(rng, n_total)
    vs = VirtualShards(M, 2, M.slab_partition(pos, 2), M.model_params("x500"), pos, np.zeros(n_total), st, M.ACTUATOR_CMD, cmd, M.ARITH_LITERAL,
                       M.EXCHANGE_EXPORT_SETS)
    assert [g.n for g, _ in vs.shards] == [130, 129]
    vs.tick_n(40, True, False, 100.0)
    for ci in vs.info():
        assert ci["ticks"] == 40 and 1 <= ci["searches"] < 40, ci  # at least one search and one export tick
    assert (live(M) > base).all(), (base, live(M))
    if comm_destroy_first:
        vs.close()  # comm_destroy on every rank
    for g, _ in vs.shards:
        g.close()
    vs.group.close()
    assert (live(M) == base).all(), (base, live(M))


def test_peer_window_that_never_becomes_a_communicator(mrs):
    M = mrs
    base = baseline(M)
    s = make_swarm(M, M.ARITH_LITERAL)
    before = live(M)
    s.peer_window_create(2, 0, 2 * N, want_handle=False)
    held = live(M)
    assert held[0] == before[0] + 2 and held[1] == before[1] + 1, (before, held)  # window, ticket words; the pinned error word
    with pytest.raises(M.MrsError, match="already has a peer window"):
        s.peer_window_create(2, 0, 2 * N, want_handle=False)
    assert (live(M) == held).all()
    s.comm_destroy()
    assert (live(M) == before).all(), (before, live(M))
    s.close()
    assert (live(M) == base).all(), (base, live(M))


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])
def test_clones_own_their_resources(mrs, order):
    M = mrs
    base = baseline(M)
    s = make_swarm(M, M.ARITH_LITERAL)
    s.tick_n(DT, 3, True, False, 100.0)
    swarms = [s, s.clone(), s.clone_resized(200)]
    for c in swarms[1:]:
        c.step_n(DT, 2)
        assert c.get_states(0, N).tobytes() == swarms[1].get_states(0, N).tobytes()
    assert (live(M) > base).all()
    for k in order:
        swarms[k].get_states()  # (the others are alive and usable whichever went first)
        swarms[k].close()
    assert (live(M) == base).all(), (base, live(M))
