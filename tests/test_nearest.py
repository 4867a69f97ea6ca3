"""CPU-side checks of the nearest-neighbour observations (include/mrs_swarm.h, "nearest-neighbour observations"): the symbols are
exported, the header's MRS_NN_* values are the Python ones, mrs_nearest_width returns the slot widths, tensors.nearest refuses bad
tensors before any library call, and the numpy reference the GPU tests use (nearest_ref / nearest_rows below) agrees with a plain
O(n^2) loop.  No pointer reaches the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import abi_header, fake_cuda, stand_in

NN_WIDTHS = {"REL_POS": 3, "REL_POS_BODY": 3, "REL_VEL": 3, "REL_VEL_BODY": 3, "DIST": 1}


# ---- the numpy reference (used by test_nearest_gpu.py) ----

def _d2(xq, xc):
    """d2 in the kernel's term order: dx = x_j - x_i, ((dx*dx) + dy*dy) + dz*dz, elementwise FP64 (numpy contracts nothing)"""
    d = xc - xq
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


@np.errstate(over="ignore")
def nearest_ref(x, first, count, k, radius):
    """(index [count, k] int64 with -1 in empty slots, counts [count], d2 [count, k] with 0 in empty slots): for each UAV i of
    [first, first + count) the first k of the UAVs j != i with d2 < radius * radius by ascending (d2, j).  A grid of cells larger than the
    radius picks the candidate pairs (any cell edge above the radius lists every pair within it); the predicate and the order are exact."""
    x = np.asarray(x, np.float64)
    n = len(x)
    rr = float(radius) * float(radius)
    idx = np.full((count, k), -1, np.int64)
    cnt = np.zeros(count, np.int64)
    dd = np.zeros((count, k))
    fin = np.flatnonzero(np.isfinite(x).all(axis=1))
    if count == 0 or len(fin) == 0:
        return idx, cnt, dd
    edge = float(radius) * 1.001
    cell = np.clip(np.floor(x[fin] / edge), -(2.0 ** 40), 2.0 ** 40).astype(np.int64)
    axes = [np.unique(cell[:, a]) for a in range(3)]  # cells keyed by their rank on each axis: (n + 1)^3 stays inside int64
    base = len(fin) + 1

    def key_of(c):
        r = [np.searchsorted(axes[a], c[:, a]) for a in range(3)]
        hit = np.ones(len(c), bool)
        for a in range(3):
            rc = np.minimum(r[a], len(axes[a]) - 1)
            hit &= axes[a][rc] == c[:, a]
        return np.where(hit, (r[0] * base + r[1]) * base + r[2], -1)

    key = key_of(cell)
    order = np.argsort(key, kind="stable")
    skey, sidx = key[order], fin[order]
    q = np.arange(first, first + count)
    qfin = np.isfinite(x[q]).all(axis=1)
    qi = q[qfin]
    pos_of = np.full(n, -1)
    pos_of[fin] = np.arange(len(fin))
    qcell = cell[pos_of[qi]]
    pairs_i, pairs_j = [], []
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):
                c = qcell + [ox, oy, oz]
                k2 = key_of(c)
                a = np.searchsorted(skey, k2, "left")
                b = np.searchsorted(skey, k2, "right")
                m = b - a
                pi = np.repeat(qi, m)
                start = np.repeat(a - np.concatenate([[0], np.cumsum(m)[:-1]]), m) + np.arange(m.sum())
                pairs_i.append(pi)
                pairs_j.append(sidx[start])
    pi, pj = np.concatenate(pairs_i), np.concatenate(pairs_j)
    d2 = _d2(x[pi], x[pj])
    keep = (d2 < rr) & (pj != pi)
    pi, pj, d2 = pi[keep], pj[keep], d2[keep]
    o = np.lexsort((pj, d2, pi))
    pi, pj, d2 = pi[o], pj[o], d2[o]
    row = pi - first
    begin = np.searchsorted(row, np.arange(count), "left")
    tot = np.searchsorted(row, np.arange(count), "right") - begin
    rank = np.arange(len(row)) - begin[row]
    sel = rank < k
    idx[row[sel], rank[sel]] = pj[sel]
    dd[row[sel], rank[sel]] = d2[sel]
    cnt[:] = np.minimum(tot, k)
    return idx, cnt, dd


def _body(R, d):
    """R^T d with R row-major [.., 3, 3]: ((R[0][c] d0 + R[1][c] d1) + R[2][c] d2), the R^T v of pose_math.h"""
    return np.stack([(R[..., 0, c] * d[..., 0] + R[..., 1, c] * d[..., 1]) + R[..., 2, c] * d[..., 2] for c in range(3)], axis=-1)


def nearest_rows(x, v, R, first, idx, dd, fields):
    """the FP64 rows [count, k * width] of the slots listed in idx (empty slots 0), the MRS_NN_* fields of `fields` in bit order"""
    count, k = idx.shape
    q = np.arange(first, first + count)
    valid = idx >= 0
    j = np.where(valid, idx, 0)
    parts = []
    d = x[j] - x[q][:, None, :]
    w = v[j] - v[q][:, None, :]
    Rq = np.broadcast_to(R[q][:, None], (count, k, 3, 3))
    if fields & 1:
        parts.append(d)
    if fields & 2:
        parts.append(_body(Rq, d))
    if fields & 4:
        parts.append(w)
    if fields & 8:
        parts.append(_body(Rq, w))
    if fields & 16:
        parts.append(np.sqrt(dd)[..., None])
    if not parts:
        return np.zeros((count, 0))
    slot = np.concatenate(parts, axis=2)
    slot[~valid] = 0.0
    return slot.reshape(count, -1)


@np.errstate(over="ignore")
def brute_force(x, first, count, k, radius):
    """the definition, one pair at a time"""
    rr = float(radius) * float(radius)
    out = []
    for i in range(first, first + count):
        if not np.isfinite(x[i]).all():
            out.append([])
            continue
        nb = []
        for j in range(len(x)):  # (-1e300 against a finite UAV: d2 overflows to inf, which no radius admits)
            if j == i or not np.isfinite(x[j]).all():
                continue
            dx, dy, dz = x[j][0] - x[i][0], x[j][1] - x[i][1], x[j][2] - x[i][2]
            d2 = ((dx * dx) + dy * dy) + dz * dz
            if d2 < rr:
                nb.append((d2, j))
        out.append(sorted(nb)[:k])
    return out


def header_enums():
    return {name: eval(expr.strip(), {}) for name, expr in re.findall(r"\b(MRS_NN_[A-Z0-9_]+)\s*=\s*([^,}\n]+)", abi_header())}


# ---- tests ----

def test_reference_equals_the_definition():
    rng = np.random.default_rng(11)
    n = 300
    x = rng.uniform(-12, 12, (n, 3))
    x[10:14] = x[9]                                          # coincident UAVs
    lat = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 2.0 - 40.0
    x[20:47] = lat                                           # a lattice: equal distances, ties by index
    x[50] = [np.nan, 0, 0]
    x[51] = [np.inf, 1, 1]
    x[52] = [-1e300, 5, 5]                                   # far away, finite
    for first, count, k, radius in ((0, n, 8, 3.0), (5, 100, 1, 2.0001), (0, n, 32, 6.5), (17, 40, 4, 2.5), (0, n, 3, 0.5), (49, 5, 8, 4.0)):
        idx, cnt, dd = nearest_ref(x, first, count, k, radius)
        want = brute_force(x, first, count, k, radius)
        for r in range(count):
            got = [(dd[r, m], int(idx[r, m])) for m in range(cnt[r])]
            assert got == want[r], (first, count, k, radius, r)
            assert (idx[r, cnt[r]:] == -1).all() and (dd[r, cnt[r]:] == 0).all()
    idx, cnt, _ = nearest_ref(x, 0, n, 32, 2.0001)
    assert list(idx[9, :4]) == [10, 11, 12, 13]              # d2 == 0 neighbours, by index
    assert list(idx[33, :7]) == [24, 30, 32, 34, 36, 42, -1]  # the lattice centre: six at 2 m, ascending index
    assert cnt[50] == cnt[51] == 0 and cnt[52] == 0


def test_nearest_rows_layout():
    rng = np.random.default_rng(3)
    x, v = rng.normal(size=(50, 3)) * 3, rng.normal(size=(50, 3))
    R = np.broadcast_to(np.eye(3), (50, 3, 3)).copy()
    idx, cnt, dd = nearest_ref(x, 0, 50, 4, 4.0)
    rows = nearest_rows(x, v, R, 0, idx, dd, 0x1F).reshape(50, 4, 13)
    r = int(np.argmax(cnt))
    j = idx[r, 0]
    assert np.array_equal(rows[r, 0, 0:3], x[j] - x[r]) and np.array_equal(rows[r, 0, 3:6], x[j] - x[r])
    assert np.array_equal(rows[r, 0, 6:9], v[j] - v[r]) and rows[r, 0, 12] == np.sqrt(dd[r, 0])
    assert (rows[idx < 0] == 0).all()


def test_new_symbols_are_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm
    L = C.CDLL(swarm.LIB_PATH)
    for name in ("mrs_nearest_width", "mrs_swarm_nearest_device"):
        assert hasattr(L, name), name
        assert name in swarm.ABI_SYMBOLS, name


def test_header_values_equal_the_python_ones(mrs):
    from mrs_multirotor_simulator_amd import tensors
    vals = header_enums()
    for b, f in enumerate(NN_WIDTHS):
        assert vals[f"MRS_NN_{f}"] == getattr(tensors, f"NN_{f}") == 1 << b, f
    assert vals["MRS_NN_ALL"] == tensors.NN_ALL == 0x1F
    assert vals["MRS_NN_MAX_K"] == tensors.NN_MAX_K == 32


def test_nearest_width(mrs):
    from mrs_multirotor_simulator_amd import swarm
    for b, (f, w) in enumerate(NN_WIDTHS.items()):
        assert swarm.nearest_width(1 << b, 1) == w, f
        assert swarm.nearest_width(1 << b, 7) == 7 * w, f
    for k in (1, 8, 32):
        assert swarm.nearest_width(swarm.NN_ALL, k) == 13 * k
    assert swarm.nearest_width(swarm.NN_REL_POS | swarm.NN_REL_VEL | swarm.NN_DIST, 8) == 56
    assert swarm.nearest_width(0, 5) == 0
    with pytest.raises(mrs.MrsError, match="unknown neighbour field"):
        swarm.nearest_width(0x20, 4)
    for k in (0, -1, 33):
        with pytest.raises(mrs.MrsError, match="k must be in"):
            swarm.nearest_width(swarm.NN_DIST, k)


_FakeSwarm = stand_in("nearest_device")


def test_tensors_nearest_refuses_bad_tensors(mrs, monkeypatch):
    """CPU tensors, and (dressed as cuda:0, as test_device_io does) wrong shapes and dtypes: ValueError before any library call"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = _FakeSwarm()
    with pytest.raises(ValueError, match="is on cpu"):
        T.nearest(g, 4, 5.0, out=torch.zeros(100, 16), index=torch.zeros((100, 4), dtype=torch.int32),
                  counts=torch.zeros(100, dtype=torch.int32))
    on = fake_cuda(monkeypatch)
    i32 = torch.int32
    rows, idx, cnt = on(torch.zeros(100, 16)), on(torch.zeros((100, 4), dtype=i32)), on(torch.zeros(100, dtype=i32))
    bad = [
        (dict(out=on(torch.zeros(100, 15))), r"expected a \[100, >= 16\] matrix"),
        (dict(out=on(torch.zeros(99, 16))), r"expected a \[100, >= 16\] matrix"),
        (dict(out=on(torch.zeros(100, 16, dtype=torch.int32))), "dtype must be torch.float32 or torch.float64"),
        (dict(out=on(torch.zeros(16, 100).t())), "rows are not contiguous"),
        (dict(index=on(torch.zeros((100, 3), dtype=i32))), r"expected a \[100, >= 4\] matrix"),
        (dict(index=on(torch.zeros((100, 4), dtype=torch.int64))), "expected torch.int32"),
        (dict(counts=on(torch.zeros(100, dtype=torch.int64))), "expected torch.int32"),
        (dict(counts=on(torch.zeros((100, 1), dtype=i32))), "expected a vector of 100 elements"),
        (dict(counts=on(torch.zeros(200, dtype=i32)[::2])), "vector is not contiguous"),
    ]
    for kw, msg in bad:
        args = dict(out=rows, index=idx, counts=cnt)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            T.nearest(g, 4, 5.0, **args)
    with pytest.raises(mrs.MrsError, match="k must be in"):
        T.nearest(g, 33, 5.0, out=rows, index=idx, counts=cnt)


def test_nearest_test_compiles(mrs):
    """tests/cpp/nearest_test.cpp builds against the facade and the HIP runtime (run on the GPU by test_nearest_gpu.py)"""
    from test_device_io_gpu import build_cpp
    assert os.path.exists(build_cpp("nearest_test"))
