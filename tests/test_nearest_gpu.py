"""Nearest-neighbour observations on the GPU (mrs_swarm_nearest_device, tensors.nearest): indices, counts and fields equal the numpy
restatement of test_nearest.py (world-frame fields bit for bit), ties go to the lower index, a small swarm whose 27 probes share buckets
lists nobody twice, sub-ranges leave padding and other rows alone, calls inside a collision run equal numpy on the gathered state and
leave the simulation bit-identical to a run without them, 100 000 UAVs equal the host reference, bad arguments are error codes, the
caller's stream is fenced, and the C++ facade (tests/cpp/nearest_test.cpp) agrees."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_device_io_gpu import build_cpp, mixed_swarm, torch_dev
from test_nearest import nearest_ref, nearest_rows

DT = 0.001


def check_against_numpy(T, g, x, v, R, k, radius, fields, dtype, first=0, count=None, label=""):
    """one tensors.nearest call against nearest_ref / nearest_rows on the state (x, v, R) it must have read"""
    count = g.n - first if count is None else count
    rows, idx, cnt = T.nearest(g, k, radius, fields, first, count, dtype=dtype)
    return compare_with_numpy(T, rows, idx, cnt, x, v, R, k, radius, fields, dtype, first, count, label)


def nearest_ref_in_worlds(x, worlds, first, count, k, radius):
    """nearest_ref among the UAVs that carry the query UAV's label: world by world, a swarm of its own that holds the UAVs of one label
    in ascending index order (include/mrs_swarm.h, "collision worlds"); indices are the whole swarm's"""
    x, worlds = np.asarray(x, np.float64), np.asarray(worlds)
    idx, cnt, dd = np.full((count, k), -1, np.int64), np.zeros(count, np.int64), np.zeros((count, k))
    for w in np.unique(worlds[first:first + count]):
        m = np.flatnonzero(worlds == w)
        i, c, d = nearest_ref(x[m], 0, len(m), k, radius)
        sel = (m >= first) & (m < first + count)
        rows = m[sel] - first
        idx[rows], cnt[rows], dd[rows] = np.where(i >= 0, m[np.maximum(i, 0)], -1)[sel], c[sel], d[sel]
    return idx, cnt, dd


def compare_with_numpy(T, rows, idx, cnt, x, v, R, k, radius, fields, dtype, first, count, label="", worlds=None):
    """the (rows, index, counts) of a tensors.nearest call against nearest_ref / nearest_rows on the state (x, v, R) it read; worlds: the
    collision-world labels of the whole swarm, where some were set"""
    import torch
    ridx, rcnt, rdd = nearest_ref(x, first, count, k, radius) if worlds is None else nearest_ref_in_worlds(x, worlds, first, count, k, radius)
    assert np.array_equal(cnt.cpu().numpy(), rcnt), label
    assert np.array_equal(idx.cpu().numpy(), ridx), label
    if not fields:
        assert rows is None
        return rcnt
    want = nearest_rows(x, v, R, first, ridx, rdd, fields)
    got = rows.cpu().numpy()
    body = np.concatenate([np.full(w, bool(b & (T.NN_REL_POS_BODY | T.NN_REL_VEL_BODY)))
                           for b, w in ((1, 3), (2, 3), (4, 3), (8, 3), (16, 1)) if fields & b])
    body = np.tile(body, k)
    if dtype == torch.float64:
        assert np.array_equal(got[:, ~body], want[:, ~body]), label
    else:
        assert np.array_equal(got[:, ~body], want[:, ~body].astype(np.float32)), label
    if body.any():
        mag = np.abs(want).max(axis=1, keepdims=True) + 1e-300
        rel = np.abs(got[:, body].astype(np.float64) - want[:, body]) / mag
        assert rel.max() <= (1e-12 if dtype == torch.float64 else 6e-8), (label, rel.max())
    empty = np.repeat(idx.cpu().numpy() < 0, len(body) // k, axis=1)
    assert (got[empty] == 0).all(), label
    return rcnt


def spread_swarm(mrs, n=3000, side=40.0, seed=5):
    """mixed airframes with random flight state (test_device_io_gpu.mixed_swarm), positions spread across the origin"""
    rng = np.random.default_rng(seed + 100)
    g, st, _ = mixed_swarm(mrs, n=n, seed=seed)
    x = rng.uniform(-side / 2, side / 2, (n, 3))
    g.set_state(0, n, x, None, None, None, None)
    s = g.get_states()
    return g, s["x"], s["v"], s["R"].reshape(n, 3, 3)


@pytest.mark.gpu
def test_exact_against_numpy(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, x, v, R = spread_swarm(mrs)
    seen = {}
    for radius in (0.5, 2.5, 8.0):  # most alone / a few / more than 32 for most
        for k in (1, 8, 32):
            for dtype in (torch.float64, torch.float32):
                cnt = check_against_numpy(T, g, x, v, R, k, radius, T.NN_ALL, dtype, label=(radius, k, dtype))
                seen[radius, k] = cnt
    assert (seen[0.5, 8] == 0).mean() > 0.9
    assert 0.2 < (seen[2.5, 8] > 0).mean() < 1.0 and np.median(seen[2.5, 8]) < 8
    assert (seen[8.0, 32] == 32).mean() > 0.5
    # other field sets and the default
    for fields in (T.NN_REL_POS | T.NN_DIST, T.NN_REL_VEL_BODY, T.NN_DIST | T.NN_REL_POS_BODY, 0):
        check_against_numpy(T, g, x, v, R, 8, 5.0, fields, torch.float64, label=fields)
    rows, idx, cnt = T.nearest(g, 4, 5.0)
    assert rows.dtype == torch.float32 and rows.shape == (g.n, 16) and idx.shape == (g.n, 4) and cnt.shape == (g.n,)


@pytest.mark.gpu
def test_ties_coincident_and_shared_buckets(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    # a 2-m lattice: equal distances, ordered by index; five coincident UAVs; a NaN and a far-away UAV
    n = 6 * 6 * 6 + 8
    lat = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3) * 2.0 - 5.0
    x = np.concatenate([lat, np.full((5, 3), 0.25), [[np.nan, 0, 0], [1e12, -3e11, 5.0], [-4.0, 7.0, 1.0]]])
    g = mrs.Swarm(n)
    g.construct(0, n, mrs.model_params("x500"), np.nan_to_num(x))
    g.set_state(0, n, x, None, None, None, None)
    s = g.get_states()
    xs, v, R = s["x"], s["v"], s["R"].reshape(n, 3, 3)
    assert np.isnan(xs[n - 3, 0])
    for k in (1, 6, 8, 32):
        for radius in (2.0, 2.0000001, 2.9, 3.5, 4.0):
            for dtype in (torch.float64, torch.float32):
                check_against_numpy(T, g, xs, v, R, k, radius, T.NN_ALL, dtype, label=(k, radius))
    _, idx, cnt = T.nearest(g, 8, 2.0000001, 0)
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    c = 2 * 36 + 2 * 6 + 2  # an inner lattice point: its six 2-m neighbours in ascending index
    assert cnt[c] == 6 and list(idx[c, :6]) == sorted([c - 36, c - 6, c - 1, c + 1, c + 6, c + 36])
    assert cnt[n - 3] == 0 and (idx[n - 3] == -1).all()            # the NaN UAV: an empty row, and nobody lists it
    assert not (idx == n - 3).any()
    assert list(idx[216, :4]) == [217, 218, 219, 220]              # the coincident UAVs, d2 = 0, by index
    # 40 UAVs, radius larger than the swarm: 128 buckets, the 27 probes share buckets; every other UAV listed once
    m = 40
    h = mrs.Swarm(m)
    rng = np.random.default_rng(2)
    h.construct(0, m, mrs.model_params("x500"), rng.uniform(-3, 3, (m, 3)))
    s = h.get_states()
    for radius in (20.0, 3.0, 1e6):
        cnt = check_against_numpy(T, h, s["x"], s["v"], s["R"].reshape(m, 3, 3), 32, radius, T.NN_ALL, torch.float64, label=radius)
        if radius > 10:
            assert (cnt == 32).all()
    _, idx, cnt = T.nearest(h, 32, 20.0, 0)
    for r in idx.cpu().numpy():
        assert len(set(r.tolist())) == 32


@pytest.mark.gpu
def test_sub_ranges_and_stride(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, x, v, R = spread_swarm(mrs, n=1000, side=25.0, seed=8)
    dev = torch_dev(g)
    k, w = 5, 13 * 5
    for dtype in (torch.float64, torch.float32):
        for first, count in ((1, 63), (65, 130), (0, 1), (999, 1), (937, 63)):
            buf = torch.full((count + 4, w + 7), 7.25, dtype=dtype, device=dev)
            ibuf = torch.full((count + 4, k + 3), -7, dtype=torch.int32, device=dev)
            cbuf = torch.full((count + 4,), -9, dtype=torch.int32, device=dev)
            rows, idx, cnt = T.nearest(g, k, 5.0, T.NN_ALL, first, count, out=buf[2:count + 2, 3:3 + w], index=ibuf[2:count + 2, 1:1 + k],
                                       counts=cbuf[2:count + 2])
            hb, hi, hc = buf.cpu().numpy(), ibuf.cpu().numpy(), cbuf.cpu().numpy()
            assert (hb[:2] == 7.25).all() and (hb[count + 2:] == 7.25).all() and (hb[:, :3] == 7.25).all() and (hb[:, 3 + w:] == 7.25).all()
            assert (hi[:2] == -7).all() and (hi[count + 2:] == -7).all() and (hi[:, :1] == -7).all() and (hi[:, 1 + k:] == -7).all()
            assert (hc[:2] == -9).all() and (hc[count + 2:] == -9).all()
            ridx, rcnt, rdd = nearest_ref(x, first, count, k, 5.0)
            assert np.array_equal(hi[2:count + 2, 1:1 + k], ridx) and np.array_equal(hc[2:count + 2], rcnt)
            want = nearest_rows(x, v, R, first, ridx, rdd, T.NN_REL_POS | T.NN_REL_VEL | T.NN_DIST)
            got = hb[2:count + 2, 3:3 + w].reshape(count, k, 13)[..., [0, 1, 2, 6, 7, 8, 12]].reshape(count, -1)
            assert np.array_equal(got, want.astype(hb.dtype)), (first, count)
    # index and counts alone, counts alone
    _, idx, cnt = T.nearest(g, 8, 5.0, 0, 10, 100)
    ridx, rcnt, _ = nearest_ref(x, 10, 100, 8, 5.0)
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(cnt.cpu().numpy(), rcnt)
    c = torch.zeros(100, dtype=torch.int32, device=dev)
    g.nearest_device(10, 100, 8, 5.0, 0, 0, T.DTYPE_F64, 0, 0, 0, c.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert np.array_equal(c.cpu().numpy(), rcnt)


def _sim_swarm(mrs, n, seed):
    import bench
    st, cmd = bench.make_inputs(n, "position+collisions", seed=seed, volume_per_uav=16.0)
    g = mrs.Swarm(n, arith=mrs.ARITH_FAST)
    g.construct(0, n, mrs.model_params("x500", ground_enabled=True, ground_z=0.0))
    g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    g.set_input(0, n, mrs.POSITION_CMD, cmd)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("crash", [False, True])
def test_inside_the_simulation(mrs, crash):
    """200 collision ticks with gather(POS|VEL|ROT) after every tick; run b also calls nearest there.  (a) each call equals numpy on the
    gathered state; (b) both runs end bit-identical, crash flags and collision statistics included"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n = 3000
    a, b = _sim_swarm(mrs, n, 21), _sim_swarm(mrs, n, 21)
    grp = T.OBS_POS | T.OBS_VEL | T.OBS_ROT
    listed = 0
    for t in range(200):
        for g in (a, b):
            g.tick_n(DT, 1, True, crash, 100.0)
        T.gather(a, grp, dtype=torch.float64).cpu()  # (the same calls and host waits in both runs)
        obs = T.gather(b, grp, dtype=torch.float64).cpu().numpy()
        x, v, R = obs[:, 0:3], obs[:, 3:6], obs[:, 6:15].reshape(n, 3, 3)
        k = (1, 8, 32)[t % 3]
        cnt = check_against_numpy(T, b, x, v, R, k, 3.0, T.NN_ALL, torch.float64 if t % 2 else torch.float32, label=t)
        listed += int(cnt.sum())
    assert listed > 0
    sa, sb = a.get_states(), b.get_states()
    for f in sa.dtype.names:
        assert np.array_equal(sa[f], sb[f]), f
    assert np.array_equal(a.has_crashed(), b.has_crashed())
    assert a.collision_stats() == b.collision_stats()
    assert np.array_equal(a.get_external_force(), b.get_external_force())
    if crash:
        assert a.has_crashed().any()


@pytest.mark.gpu
def test_scale_100k(mrs):
    import bench
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n = 100_000
    st, _ = bench.make_inputs(n, "position+collisions", seed=3)
    g = mrs.Swarm(n, arith=mrs.ARITH_FAST)
    g.construct(0, n, mrs.model_params("x500"))
    g.set_state(0, n, st["x"], st["v"], st["R"], st["omega"], st["motor_rpm"])
    s = g.get_states()
    fields = T.NN_REL_POS | T.NN_REL_VEL | T.NN_DIST
    cnt = check_against_numpy(T, g, s["x"], s["v"], s["R"].reshape(n, 3, 3), 8, 5.0, fields, torch.float32, label="100k")
    assert 5.0 < cnt.mean() < 8.0, cnt.mean()


@pytest.mark.gpu
def test_bad_arguments_are_error_codes(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, x, v, R = spread_swarm(mrs, n=300, side=15.0, seed=4)
    dev = torch_dev(g)
    st = torch.cuda.current_stream(dev).cuda_stream
    F64 = T.DTYPE_F64
    rows = torch.zeros((300, 13 * 8), dtype=torch.float64, device=dev)
    idx = torch.zeros((300, 8), dtype=torch.int32, device=dev)
    cnt = torch.zeros(300, dtype=torch.int32, device=dev)
    r, i, c = rows.data_ptr(), idx.data_ptr(), cnt.data_ptr()
    host = np.zeros((300, 13 * 8))
    host_i = np.zeros((300, 8), np.int32)
    # memory of the wrong size: one allocation of its own (a torch tensor may sit inside a larger cached block), 4 KiB against the
    # 250 KB the rows need; the runtime must report its extent, else the library could not refuse it
    hip = C.CDLL("libamdhip64.so")
    small_p, base, size = C.c_void_p(), C.c_void_p(), C.c_size_t()
    assert hip.hipMalloc(C.byref(small_p), C.c_size_t(4096)) == 0
    assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), small_p) == 0 and size.value < 300 * 104 * 8
    small = small_p.value
    bad = [
        ((200, 101, 8, 5.0, T.NN_ALL, r, F64, 104, i, 8, c), "error 3:"),
        ((-1, 10, 8, 5.0, T.NN_ALL, r, F64, 104, i, 8, c), "error 3:"),
        ((0, 300, 0, 5.0, T.NN_ALL, r, F64, 104, i, 8, c), "error 1:.*k must be"),
        ((0, 300, 33, 5.0, T.NN_ALL, r, F64, 33 * 13, i, 33, c), "error 1:.*k must be"),
        ((0, 300, 8, 0.0, T.NN_ALL, r, F64, 104, i, 8, c), "error 1:.*radius"),
        ((0, 300, 8, -1.0, T.NN_ALL, r, F64, 104, i, 8, c), "error 1:.*radius"),
        ((0, 300, 8, float("nan"), T.NN_ALL, r, F64, 104, i, 8, c), "error 1:.*radius"),
        ((0, 300, 8, float("inf"), T.NN_ALL, r, F64, 104, i, 8, c), "error 1:.*radius"),
        ((0, 300, 8, 5.0, 0x20, r, F64, 104, i, 8, c), "error 1:.*unknown neighbour field"),
        ((0, 300, 8, 5.0, T.NN_ALL, r, F64, 103, i, 8, c), "error 1:.*stride"),
        ((0, 300, 8, 5.0, T.NN_ALL, r, 2, 104, i, 8, c), "error 1:.*dtype"),
        ((0, 300, 8, 5.0, T.NN_ALL, r, F64, 104, i, 7, c), "error 1:.*index_stride"),
        ((0, 300, 8, 5.0, 0, 0, F64, 0, 0, 0, 0), "error 1:.*no output"),
        ((0, 300, 8, 5.0, T.NN_ALL, 0, F64, 104, i, 8, c), "error 1:.*null pointer"),
        ((0, 300, 8, 5.0, T.NN_ALL, host.ctypes.data, F64, 104, i, 8, c), "error 1:.*dev_rows"),
        ((0, 300, 8, 5.0, 0, 0, F64, 0, host_i.ctypes.data, 8, c), "error 1:.*dev_index"),
        ((0, 300, 8, 5.0, T.NN_ALL, small, F64, 104, i, 8, c), "error 1:.*dev_rows: the rows extend past"),
        ((0, 300, 8, 5.0, 0, 0, F64, 0, small, 8, c), "error 1:.*dev_index: the rows extend past"),
        ((0, 300, 8, 5.0, 0, 0, F64, 0, 0, 0, small + 4096 - 1196), "error 1:.*dev_count: the rows extend past"),
    ]
    rows.fill_(3.5)
    torch.cuda.synchronize(dev)
    for args, msg in bad:
        with pytest.raises(mrs.MrsError, match=msg):
            g.nearest_device(*args, st)
    torch.cuda.synchronize(dev)
    assert hip.hipFree(C.c_void_p(small)) == 0
    assert (rows.cpu().numpy() == 3.5).all()  # nothing was launched
    check_against_numpy(T, g, x, v, R, 8, 5.0, T.NN_ALL, torch.float64)
    # a sharded swarm
    group = mrs.LoopbackGroup(2)
    shards = []
    for rk in range(2):
        s = mrs.Swarm(100)
        s.construct(0, 100, mrs.model_params("x500"), np.stack([np.arange(100) * 3.0 + 400 * rk, np.zeros(100), np.full(100, 5.0)], axis=1))
        s.comm_init_loopback(group, rk, 200)
        shards.append(s)
    for s in shards:
        with pytest.raises(mrs.MrsError, match="error 1:.*sharded"):
            T.nearest(s, 4, 5.0)
    for s in shards:
        s.close()
    group.close()


@pytest.mark.gpu
def test_caller_stream_is_fenced(mrs):
    """the output rows are filled with a sentinel on a side stream kept busy by a long sleep, then nearest is called with that stream
    current: the rows must hold the result (the kernel ran after the fill), and a copy queued behind the call on the side stream reads it"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g, x, v, R = spread_swarm(mrs, n=3000, side=40.0, seed=6)
    dev = torch_dev(g)
    ridx, rcnt, rdd = nearest_ref(x, 0, g.n, 8, 5.0)
    want = nearest_rows(x, v, R, 0, ridx, rdd, T.NN_REL_POS | T.NN_DIST)
    out = torch.zeros((g.n, 32), dtype=torch.float64, device=dev)
    idx = torch.zeros((g.n, 8), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        out.fill_(-1.0)
        idx.fill_(-5)
        rows, _, _ = T.nearest(g, 8, 5.0, dtype=torch.float64, out=out, index=idx)
        copy = rows * 1.0
        icopy = idx.clone()
    side.synchronize()
    assert np.array_equal(copy.cpu().numpy(), want) and np.array_equal(icopy.cpu().numpy(), ridx)


@pytest.mark.gpu
def test_cpp_facade_equals_python(mrs):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    n, k = 2000, 8
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "nearest.bin")
        out = subprocess.run([build_cpp("nearest_test"), path], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        for tag in ("ok nearest_equals_brute_force", "ok written"):
            assert tag in out.stdout, out.stdout
        raw = open(path, "rb").read()
    cidx = np.frombuffer(raw[:4 * n * k], np.int32).reshape(n, k)
    crows = np.frombuffer(raw[4 * n * k:], np.float64).reshape(n, 13 * k)
    i = np.arange(n)
    pos = np.stack([3.1 * (i % 20) + 0.01 * (i % 7), 2.9 * ((i // 20) % 20) - 0.02 * (i % 5), 3.3 * (i // 400) + 0.005 * (i % 11)], axis=1)
    g = mrs.Swarm(n)
    g.construct(0, n, mrs.model_params("x500"), pos)
    rows, idx, _ = T.nearest(g, k, 5.0, T.NN_ALL, dtype=torch.float64)
    assert np.array_equal(idx.cpu().numpy(), cidx)
    assert np.array_equal(rows.cpu().numpy(), crows)
