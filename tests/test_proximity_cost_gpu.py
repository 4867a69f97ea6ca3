"""The proximity cost on the GPU (mrs_swarm_proximity_cost_device, tensors.proximity_cost): every result is compared on bits with the
numpy restatement of test_proximity_cost.py — three radii x three k x three kinds on 3000 UAVs in both lane orders, ties, coincident and
non-finite UAVs, accumulation onto existing bits, collision worlds, calls between the pieces of a cost tick rollout (which leave the
simulation bit-identical to a run without them, the pending collision tick included), refusals that change nothing, the caller's stream
fence, and the C++ facade (tests/cpp/proximity_cost_test.cpp)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle_swarm as O
from test_device_io_gpu import build_cpp, torch_dev
from test_nearest_gpu import spread_swarm
from test_proximity_cost import (COUNT, HINGE2, INVERSE, add_bits, lattice_set, neighbours_in_worlds, proximity_ref, proximity_terms,
                                 same_bits)
from test_rollout_gpu import DT, REBOUNCE
from test_rollout_tick_cost_gpu import make_targets
from test_rollout_tick_gpu import N_PAIR, assert_same_swarm, pair_state, pair_swarm

pytestmark = pytest.mark.gpu
KINDS = (HINGE2, INVERSE, COUNT)
SENTINEL = -123.456


def run(T, g, radius, k, kind, weight, eps, first=0, count=None, start=None, pad=3):
    """one tensors.proximity_cost call into the middle of sentinel-padded buffers: (cost [count], found [count]) as numpy; start: the
    bits the cost vector holds before an accumulating call (None: accumulate=False over NaN bits)"""
    import torch
    count = g.n - first if count is None else count
    dev = torch_dev(g)
    cbuf = torch.full((count + 2 * pad,), SENTINEL, dtype=torch.float64, device=dev)
    fbuf = torch.full((count + 2 * pad,), -9, dtype=torch.int32, device=dev)
    cbuf[pad:pad + count] = float("nan") if start is None else torch.tensor(start, dtype=torch.float64, device=dev)
    out, found = T.proximity_cost(g, radius, k, kind, weight, eps, first, count, out=cbuf[pad:pad + count], accumulate=start is not None,
                                  found=fbuf[pad:pad + count])
    assert out.data_ptr() == cbuf[pad:].data_ptr() and found.data_ptr() == fbuf[pad:].data_ptr()
    hc, hf = cbuf.cpu().numpy(), fbuf.cpu().numpy()
    assert (hc[:pad] == SENTINEL).all() and (hc[pad + count:] == SENTINEL).all(), "cost elements outside [0, count) were touched"
    assert (hf[:pad] == -9).all() and (hf[pad + count:] == -9).all(), "found elements outside [0, count) were touched"
    return hc[pad:pad + count], hf[pad:pad + count]


def check(T, g, x, radius, k, kind, weight, eps, first=0, count=None, worlds=None, label=""):
    """both accumulate states of one call against the restatement on the positions x; returns (term, found) of the restatement"""
    count = g.n - first if count is None else count
    term, found = proximity_ref(x, first, count, k, radius, kind, weight, eps, worlds)
    got, gf = run(T, g, radius, k, kind, weight, eps, first, count)
    assert np.array_equal(gf, found), (label, "found")
    assert same_bits(got, add_bits(None, term)), (label, "accumulate=0", np.flatnonzero(got != add_bits(None, term))[:5])
    start = np.linspace(-3.0, 5.0, count)
    start[::7] = -0.0
    got, gf = run(T, g, radius, k, kind, weight, eps, first, count, start=start)
    assert np.array_equal(gf, found) and same_bits(got, add_bits(start, term)), (label, "accumulate=1")
    return term, found


def test_exact_against_numpy(mrs):
    from mrs_multirotor_simulator_amd import tensors as T
    g, x, _, _ = spread_swarm(mrs)
    n = g.n
    lists = {radius: neighbours_in_worlds(x, 0, n, radius) for radius in (0.5, 2.5, 8.0)}  # one search per radius, shared below
    f = {radius: lists[radius][1] for radius in lists}
    assert (f[0.5] == 0).mean() > 0.9
    assert (f[2.5] >= 1).mean() > 0.9 and (f[2.5] > 8).mean() < 0.02
    assert (f[8.0] > 8).all() and (f[8.0] >= 32).mean() > 0.95
    idx, found, dd = lists[8.0]
    nearest_first = proximity_terms(dd, found, 32, 8.0, HINGE2, 1.0, 0.0)
    by_index = np.argsort(np.where(idx[:, :32] >= 0, idx[:, :32], 2 ** 40), axis=1, kind="stable")
    ascending = proximity_terms(dd, found, 32, 8.0, HINGE2, 1.0, 0.0, order=by_index)
    assert (nearest_first.view(np.int64) != ascending.view(np.int64)).mean() > 0.5  # a wrong summation order cannot pass
    assert np.allclose(nearest_first, ascending, rtol=1e-12)
    for radius in (0.5, 2.5, 8.0):
        _, found, dd = lists[radius]
        for k in (1, 8, 32):
            for kind in KINDS:
                weight, eps = (1.0, 0.0) if kind != INVERSE else (0.7, 0.05)
                term = proximity_terms(dd, found, k, radius, kind, weight, eps)
                for first, count in ((0, n), (100, 500)):  # sorted lane order / index order
                    sl = slice(first, first + count)
                    got, gf = run(T, g, radius, k, kind, weight, eps, first, count)
                    assert np.array_equal(gf, found[sl]), (radius, k, kind, first)
                    assert same_bits(got, add_bits(None, term[sl])), (radius, k, kind, first)
                    start = np.cos(np.arange(count))
                    got, gf = run(T, g, radius, k, kind, weight, eps, first, count, start=start)
                    assert np.array_equal(gf, found[sl]) and same_bits(got, add_bits(start, term[sl])), (radius, k, kind, first, "accumulate")
    # defaults, and without found
    _, found, dd = lists[2.5]
    out, nofound = T.proximity_cost(g, 2.5)
    assert nofound is None and out.shape == (n,)
    assert same_bits(out.cpu().numpy(), add_bits(None, proximity_terms(dd, found, 8, 2.5, HINGE2, 1.0, 0.0)))
    out, fnd = T.proximity_cost(g, 2.5, found=True)
    assert np.array_equal(fnd.cpu().numpy(), lists[2.5][1])


def test_ties_coincident_and_non_finite(mrs):
    from mrs_multirotor_simulator_amd import tensors as T
    x = lattice_set()
    n = len(x)
    g = mrs.Swarm(n)
    g.construct(0, n, mrs.model_params("x500"), np.nan_to_num(x))
    g.set_state(0, n, x, None, None, None, None)
    xs = g.get_states()["x"]
    assert np.isnan(xs[n - 3, 0])
    for radius in (2.0, 2.0000001, 2.9, 3.5):
        for k in (4, 8, 32):
            for kind, weight, eps in ((HINGE2, 1.0, 0.0), (INVERSE, 1.0, 0.0), (INVERSE, -2.0, 1e-3), (COUNT, 0.3, 0.0), (COUNT, -0.0, 0.0)):
                term, found = check(T, g, xs, radius, k, kind, weight, eps, label=(radius, k, kind, eps))
                assert found[n - 3] == 0 and same_bits(term[n - 3], 0.0)  # the NaN UAV adds +0.0
                if kind == INVERSE:
                    assert np.isposinf(term[216:221]).all() if eps == 0.0 else np.isfinite(term).all()
    got, found = run(T, g, 2.0, 4, HINGE2, 1.0, 0.0)
    with np.errstate(invalid="ignore"):
        far = np.sqrt(((xs[:216] - 0.25) ** 2).sum(axis=1)) > 2.5
    assert (found[:216][far] == 0).all() and same_bits(got[:216][far], np.zeros(far.sum()))  # strict <: nobody at exactly 2 m
    assert same_bits(got[216:221], np.full(5, 16.0))                                          # d2 = 0: g = radius, four times
    _, f2 = run(T, g, 2.0000001, 8, COUNT, 1.0, 0.0)
    c = 2 * 36 + 2 * 6 + 4  # an inner lattice point away from the coincident five: its six 2-m neighbours
    assert f2[c] == 6
    # nobody counts the NaN UAV: with it moved far away every other UAV's found stays what it was
    _, f_all = run(T, g, 3.5, 8, COUNT, 1.0, 0.0)
    assert np.array_equal(f_all, proximity_ref(np.where(np.isnan(xs), 1e9, xs), 0, n, 8, 3.5, COUNT, 1.0, 0.0)[1])
    # 40 UAVs, radius larger than the swarm: the 27 probes share buckets; everybody found once
    m = 40
    h = mrs.Swarm(m)
    h.construct(0, m, mrs.model_params("x500"), np.random.default_rng(2).uniform(-3, 3, (m, 3)))
    hx = h.get_states()["x"]
    for radius in (20.0, 1e6):
        for kind in KINDS:
            _, found = check(T, h, hx, radius, 32, kind, 1.0, 0.5, label=radius)
            assert (found == m - 1).all()


def test_accumulate(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, x, _, _ = spread_swarm(mrs, n=600, side=12.0, seed=9)
    n = g.n
    term, found = proximity_ref(x, 0, n, 8, 1.0, HINGE2, 2.0, 0.0)
    alone = np.flatnonzero(found == 0)
    assert len(alone) > 10 and (found > 0).sum() > 10
    start = np.random.default_rng(4).normal(0, 100.0, n)
    start[alone[:5]] = -0.0
    got, _ = run(T, g, 1.0, 8, HINGE2, 2.0, 0.0, start=start)
    assert same_bits(got, add_bits(start, term))
    assert same_bits(got[alone[:5]], np.zeros(5))  # -0.0 + (+0.0) = +0.0
    got, _ = run(T, g, 1.0, 8, HINGE2, 2.0, 0.0)  # accumulate=0 over NaN bits: the term
    assert same_bits(got, add_bits(None, term))
    # two accumulating calls: the stated double add
    t2, _ = proximity_ref(x, 0, n, 4, 2.0, INVERSE, 0.5, 0.1)
    out = torch.tensor(start, device=torch_dev(g))
    T.proximity_cost(g, 1.0, 8, T.PROX_HINGE2, 2.0, out=out, accumulate=True)
    T.proximity_cost(g, 2.0, 4, T.PROX_INVERSE, 0.5, 0.1, out=out, accumulate=True)
    assert same_bits(out.cpu().numpy(), add_bits(add_bits(start, term), t2))


def test_worlds(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    m, copies = 40, 4
    scene = np.random.default_rng(12).uniform(-3, 3, (m, 3))
    g = mrs.Swarm(m * copies)
    g.construct(0, m * copies, mrs.model_params("x500"), np.concatenate([scene] * copies))
    lone = mrs.Swarm(m)
    lone.construct(0, m, mrs.model_params("x500"), scene)
    x, lx = g.get_states()["x"], lone.get_states()["x"]
    for kind in KINDS:
        _, found = check(T, g, x, 2.5, 8, kind, 1.5, 0.25, label="before labels")
        assert (found >= 3).all()  # the coincident partners of the other copies
    labels = np.repeat(np.array([7, -1, 0, 2 ** 31 - 1], np.int32), m)
    T.set_worlds(g, torch.tensor(labels, device=torch_dev(g)))
    for kind in KINDS:
        for k in (2, 8):
            check(T, g, x, 2.5, k, kind, 1.5, 0.25, worlds=labels, label="labels")
            check(T, g, x, 2.5, k, kind, 1.5, 0.25, first=30, count=25, worlds=labels, label="labels, index order")
            want, wf = run(T, lone, 2.5, k, kind, 1.5, 0.25)
            got, gf = run(T, g, 2.5, k, kind, 1.5, 0.25)
            for c in range(copies):
                assert same_bits(got[c * m:(c + 1) * m], want) and np.array_equal(gf[c * m:(c + 1) * m], wf), (kind, k, c)
    assert wf.max() > 2  # (the scene has neighbourhoods)


@pytest.mark.parametrize("crash", [False, True], ids=["elastic", "crash"])
@pytest.mark.parametrize("arith", ["LITERAL", "FAST"])
def test_inside_a_horizon(mrs, arith, crash):
    """rollout_tick_cost over 24 + 24 ticks with accumulate, proximity_cost(accumulate) between the halves and after; a twin runs the same
    horizon without the proximity calls"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    ar = getattr(mrs, "ARITH_" + arith)
    a, b = pair_swarm(mrs, ar), pair_swarm(mrs, ar)
    dev = torch_dev(a)
    rng = np.random.default_rng(31)
    ticks, hold = 24, 4
    groups = T.OBS_POS | T.OBS_VEL
    pos, _ = pair_state()
    blocks = np.concatenate([pos, np.zeros((N_PAIR, 1))], axis=1)[None] + rng.normal(0, 0.01, (2 * ticks // hold, N_PAIR, 4))
    cmd = torch.tensor(blocks, device=dev)
    tg, wt = make_targets(rng, 2 * ticks // hold, N_PAIR, T.gather_width(groups), torch.float64, dev, False, False)
    costs = {id(a): torch.zeros(N_PAIR, dtype=torch.float64, device=dev), id(b): torch.zeros(N_PAIR, dtype=torch.float64, device=dev)}
    half = ticks // hold
    listed = 0
    for piece in range(2):
        sl = slice(piece * half, (piece + 1) * half)
        for g in (a, b):
            T.rollout_tick_cost(g, O.POSITION_CMD, cmd[sl], DT, crash, REBOUNCE, groups, tg[sl], wt[sl], 1000.0, hold=hold, out=costs[id(g)],
                                accumulate=True)
        xa = T.gather(a, T.OBS_POS, dtype=torch.float64).cpu().numpy()  # (the same calls and host waits in both runs)
        T.gather(b, T.OBS_POS, dtype=torch.float64).cpu()
        if piece == 0:  # (afterwards a's vector holds the proximity terms too)
            assert same_bits(costs[id(a)].cpu().numpy(), costs[id(b)].cpu().numpy())
        for kind, radius, k, weight, eps in ((HINGE2, 12.0, 4, 0.5, 0.0), (INVERSE, 3.0, 1, 2.0, 0.01)):
            before = costs[id(a)].cpu().numpy()
            term, found = proximity_ref(xa, 0, N_PAIR, k, radius, kind, weight, eps)
            _, gf = T.proximity_cost(a, radius, k, kind, weight, eps, out=costs[id(a)], accumulate=True, found=True)
            assert np.array_equal(gf.cpu().numpy(), found), (piece, kind)
            assert same_bits(costs[id(a)].cpu().numpy(), add_bits(before, term)), (piece, kind)
            listed += int(found.sum())
    assert listed > 2 * N_PAIR
    if crash:
        assert np.asarray(a.has_crashed()).any()
    assert_same_swarm(a, b, f"{arith} crash={crash}: with and without the proximity calls")
    for g in (a, b):
        g.tick_n(DT, 1, True, crash, REBOUNCE)  # evaluates the collision tick the horizon left pending
    assert_same_swarm(a, b, f"{arith} crash={crash}: one more tick on both")


def test_refused_calls_change_nothing(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, x, _, _ = spread_swarm(mrs, n=300, side=15.0, seed=4)
    dev = torch_dev(g)
    st = torch.cuda.current_stream(dev).cuda_stream
    cost = torch.full((300,), SENTINEL, dtype=torch.float64, device=dev)
    found = torch.full((300,), -9, dtype=torch.int32, device=dev)
    c, f = cost.data_ptr(), found.data_ptr()
    host_c, host_f = np.zeros(300), np.zeros(300, np.int32)
    hip = C.CDLL("libamdhip64.so")
    small_p, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(small_p), C.c_size_t(4096)) == 0
    assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), small_p) == 0 and size.value < 4100
    small = small_p.value
    nan, inf = float("nan"), float("inf")
    H, I = HINGE2, INVERSE
    bad = [
        ((200, 101, 8, 5.0, H, 1.0, 0.0, c, 0, f), "error 3:"),
        ((-1, 10, 8, 5.0, H, 1.0, 0.0, c, 0, f), "error 3:"),
        ((0, 300, 0, 5.0, H, 1.0, 0.0, c, 0, f), "error 1:.*k must be"),
        ((0, 300, 33, 5.0, H, 1.0, 0.0, c, 0, f), "error 1:.*k must be"),
        ((0, 300, 8, 0.0, H, 1.0, 0.0, c, 0, f), "error 1:.*radius"),
        ((0, 300, 8, -1.0, H, 1.0, 0.0, c, 0, f), "error 1:.*radius"),
        ((0, 300, 8, nan, H, 1.0, 0.0, c, 0, f), "error 1:.*radius"),
        ((0, 300, 8, inf, H, 1.0, 0.0, c, 0, f), "error 1:.*radius"),
        ((0, 300, 8, 5.0, 3, 1.0, 0.0, c, 0, f), "error 1:.*unknown proximity kind"),
        ((0, 300, 8, 5.0, -1, 1.0, 0.0, c, 0, f), "error 1:.*unknown proximity kind"),
        ((0, 300, 8, 5.0, I, 1.0, nan, c, 0, f), "error 1:.*eps"),
        ((0, 300, 8, 5.0, I, 1.0, inf, c, 0, f), "error 1:.*eps"),
        ((0, 300, 8, 5.0, I, 1.0, -1e-9, c, 0, f), "error 1:.*eps"),
        ((0, 300, 8, 5.0, H, 1.0, 0.0, 0, 0, f), "error 1:.*dev_cost: null pointer"),
        ((0, 0, 8, 5.0, H, 1.0, 0.0, 0, 0, f), "error 1:.*dev_cost: null pointer"),
        ((0, 300, 8, 5.0, H, 1.0, 0.0, host_c.ctypes.data, 0, f), "error 1:.*dev_cost"),
        ((0, 300, 8, 5.0, H, 1.0, 0.0, c, 1, host_f.ctypes.data), "error 1:.*dev_found"),
        ((0, 300, 8, 5.0, H, 1.0, 0.0, small + 4096 - 2392, 1, f), "error 1:.*dev_cost: the rows extend past"),
        ((0, 300, 8, 5.0, H, 1.0, 0.0, c, 1, small + 4096 - 1196), "error 1:.*dev_found: the rows extend past"),
    ]
    torch.cuda.synchronize(dev)
    for args, msg in bad:
        with pytest.raises(mrs.MrsError, match=msg):
            g.proximity_cost_device(*args, st)
    torch.cuda.synchronize(dev)
    assert hip.hipFree(C.c_void_p(small)) == 0
    assert (cost.cpu().numpy() == SENTINEL).all() and (found.cpu().numpy() == -9).all()  # nothing was launched
    # eps is ignored by the other kinds; count == 0 is MRS_OK
    g.proximity_cost_device(0, 0, 8, 5.0, H, 1.0, 0.0, c, 1, 0, st)
    g.proximity_cost_device(300, 0, 8, 5.0, H, 1.0, 0.0, c, 0, f, st)
    assert (cost.cpu().numpy() == SENTINEL).all() and (found.cpu().numpy() == -9).all()
    for kind in (H, COUNT):
        g.proximity_cost_device(0, 300, 8, 5.0, kind, 1.0, nan, c, 0, f, st)
        term, fnd = proximity_ref(x, 0, 300, 8, 5.0, kind, 1.0, 0.0)
        assert same_bits(cost.cpu().numpy(), add_bits(None, term)) and np.array_equal(found.cpu().numpy(), fnd)
    # a sharded swarm
    group = mrs.LoopbackGroup(2)
    shards = []
    for rk in range(2):
        s = mrs.Swarm(100)
        s.construct(0, 100, mrs.model_params("x500"), np.stack([np.arange(100) * 3.0 + 400 * rk, np.zeros(100), np.full(100, 5.0)], axis=1))
        s.comm_init_loopback(group, rk, 200)
        shards.append(s)
    cost.fill_(SENTINEL)
    for s in shards:
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.proximity_cost(s, 5.0, out=cost[:100], found=found[:100])
    assert (cost.cpu().numpy() == SENTINEL).all()
    for s in shards:
        s.close()
    group.close()


def test_caller_stream_is_fenced(mrs):
    """the cost vector is filled on a side stream kept busy by a long sleep, then proximity_cost is called with that stream current: the
    vector must hold fill + term (the kernel ran after the fill), and a copy queued behind the call on the side stream reads it"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, x, _, _ = spread_swarm(mrs, n=3000, side=40.0, seed=6)
    dev = torch_dev(g)
    term, found = proximity_ref(x, 0, g.n, 8, 5.0, HINGE2, 1.0, 0.0)
    out = torch.zeros(g.n, dtype=torch.float64, device=dev)
    fnd = torch.zeros(g.n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        out.fill_(2.5)
        fnd.fill_(-5)
        T.proximity_cost(g, 5.0, out=out, accumulate=True, found=fnd)
        copy = out * 1.0
        fcopy = fnd.clone()
    side.synchronize()
    assert same_bits(copy.cpu().numpy(), add_bits(np.full(g.n, 2.5), term)) and np.array_equal(fcopy.cpu().numpy(), found)


def test_cpp_facade_equals_python(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, k = 2000, 8
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "proximity.bin")
        out = subprocess.run([build_cpp("proximity_cost_test"), path], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok proximity_equals_brute_force", "ok written"):
            assert tag in out.stdout, out.stdout
        raw = open(path, "rb").read()
    ccost = np.frombuffer(raw[:8 * 4 * n], np.float64).reshape(4, n)
    cfound = np.frombuffer(raw[8 * 4 * n:], np.int32)
    i = np.arange(n)
    pos = np.stack([3.1 * (i % 20) + 0.01 * (i % 7), 2.9 * ((i // 20) % 20) - 0.02 * (i % 5), 3.3 * (i // 400) + 0.005 * (i % 11)], axis=1)
    g = mrs.Swarm(n)
    g.construct(0, n, mrs.model_params("x500"), pos)
    for row, kind in enumerate((T.PROX_HINGE2, T.PROX_INVERSE, T.PROX_COUNT)):
        mine, fnd = T.proximity_cost(g, 5.0, k, kind, 0.75, 0.125, found=True)
        assert same_bits(mine.cpu().numpy(), ccost[row]), kind
        assert np.array_equal(fnd.cpu().numpy(), cfound)
    both, _ = T.proximity_cost(g, 5.0, k, T.PROX_HINGE2, 0.75, 0.125)
    T.proximity_cost(g, 5.0, k, T.PROX_COUNT, 0.75, 0.125, out=both, accumulate=True)
    assert same_bits(both.cpu().numpy(), ccost[3])
    assert (cfound > k).any() and isinstance(both, torch.Tensor)
