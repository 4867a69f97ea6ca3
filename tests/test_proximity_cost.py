"""CPU-side checks of the proximity cost (include/mrs_swarm.h, "proximity cost"): the numpy restatement the GPU tests compare bits
against (proximity_ref below, built on test_nearest.nearest_ref) equals a pair-at-a-time definition in Python floats, the symbol is
exported and listed, the header prototype equals the ctypes argtypes, the header's MRS_PROX_* values are the Python ones,
tensors.proximity_cost refuses bad tensors before the library is reached, and tests/cpp/proximity_cost_test.cpp compiles.  No pointer
reaches the library."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest  # noqa: F401

from helpers import CTYPE, abi_header, abi_prototype, fake_cuda, stand_in
from test_nearest import nearest_ref

HINGE2, INVERSE, COUNT = 0, 1, 2
NAMES = ["s", "first", "count", "k", "radius", "kind", "weight", "eps", "dev_cost", "accumulate", "dev_found", "ext_stream"]
TYPES = dict(CTYPE, **{"double*": C.c_void_p, "int32_t*": C.c_void_p})


# ---- the numpy restatement (used by test_proximity_cost_gpu.py) ----

def all_neighbours(x, first, count, radius):
    """(index [count, K], found [count], d2 [count, K]) of nearest_ref with a K no row fills: every neighbour, so `found` is uncapped"""
    kk = 64
    while True:
        idx, cnt, dd = nearest_ref(x, first, count, kk, radius)
        if count == 0 or cnt.max() < kk:
            return idx, cnt, dd
        kk *= 4


def neighbours_in_worlds(x, first, count, radius, worlds=None):
    """all_neighbours among the UAVs that carry the query UAV's label: world by world, a swarm of its own that holds the UAVs of one
    label in ascending index order (the statement of include/mrs_swarm.h, "collision worlds")"""
    x = np.asarray(x, np.float64)
    if worlds is None:
        return all_neighbours(x, first, count, radius)
    worlds = np.asarray(worlds)
    parts = {}
    for w in np.unique(worlds[first:first + count]):
        members = np.flatnonzero(worlds == w)
        idx, cnt, dd = all_neighbours(x[members], 0, len(members), radius)
        parts[w] = (members, np.where(idx >= 0, members[np.maximum(idx, 0)], -1), cnt, dd)
    width = max(p[1].shape[1] for p in parts.values())
    idx, found, dd = np.full((count, width), -1, np.int64), np.zeros(count, np.int64), np.zeros((count, width))
    for members, gi, cnt, d in parts.values():
        sel = (members >= first) & (members < first + count)
        rows = members[sel] - first
        idx[rows, :gi.shape[1]], found[rows], dd[rows, :d.shape[1]] = gi[sel], cnt[sel], d[sel]
    return idx, found, dd


@np.errstate(all="ignore")
def proximity_terms(dd, found, k, radius, kind, weight, eps, order=None):
    """the contract's loop over the listed slots, nearest first (or in `order`, a [count, k] permutation of the slots): term = +0.0,
    then one FP64 addition per slot m < nf = min(found, k); every row at once, each operation a separately rounded numpy FP64 one"""
    count = len(found)
    nf = np.minimum(found, k)
    radius, weight, eps = np.float64(radius), np.float64(weight), np.float64(eps)
    term = np.zeros(count)
    slots = dd[:, :k] if dd.shape[1] >= k else np.concatenate([dd, np.zeros((count, k - dd.shape[1]))], axis=1)
    for m in range(k):
        col = slots[:, m] if order is None else slots[np.arange(count), order[:, m]]
        live = (m < nf) if order is None else (order[:, m] < nf)
        if kind == HINGE2:
            g = radius - np.sqrt(col)
            new = term + (weight * g) * g
        elif kind == INVERSE:
            new = term + weight / (col + eps)
        else:
            new = term + weight
        term = np.where(live, new, term)
    return term


def proximity_ref(x, first, count, k, radius, kind, weight, eps, worlds=None):
    """(term [count] FP64, found [count], uncapped) of mrs_swarm_proximity_cost_device; the call leaves accumulate ? c + term : 0.0 + term"""
    _, found, dd = neighbours_in_worlds(x, first, count, radius, worlds)
    return proximity_terms(dd, found, k, radius, kind, weight, eps), found


def add_bits(c, term):
    """what the call leaves in dev_cost: c + term, one FP64 addition (c = +0.0 without accumulate)"""
    with np.errstate(all="ignore"):
        return (np.zeros_like(term) if c is None else np.asarray(c, np.float64)) + term


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:  # (what IEEE gives: Python floats raise instead)
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


def brute_neighbours(x, first, count, radius, worlds=None):
    """the definition, one pair at a time, in Python floats: per query UAV the sorted list of (d2, j) of every neighbour"""
    rr = float(radius) * float(radius)
    out = []
    for i in range(first, first + count):
        nb = []
        if np.isfinite(x[i]).all():
            for j in range(len(x)):
                if j == i or not np.isfinite(x[j]).all() or (worlds is not None and worlds[j] != worlds[i]):
                    continue
                dx, dy, dz = float(x[j][0] - x[i][0]), float(x[j][1] - x[i][1]), float(x[j][2] - x[i][2])
                d2 = ((dx * dx) + dy * dy) + dz * dz
                if d2 < rr:
                    nb.append((d2, j))
        out.append(sorted(nb))
    return out


def brute_force(lists, k, radius, kind, weight, eps):
    """(term, found) of the contract from the lists of brute_neighbours, in Python floats"""
    terms = []
    for nb in lists:
        term = 0.0
        for d2, _ in nb[:k]:
            if kind == HINGE2:
                g = float(radius) - math.sqrt(d2)
                term = term + (float(weight) * g) * g
            elif kind == INVERSE:
                term = term + _div(float(weight), d2 + float(eps))
            else:
                term = term + float(weight)
        terms.append(term)
    return np.array(terms, np.float64), np.array([len(nb) for nb in lists], np.int64)


def lattice_set():
    """the set of test_nearest_gpu.test_ties_coincident_and_shared_buckets: a 2-m lattice, five coincident UAVs, a NaN UAV, a far one"""
    lat = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3) * 2.0 - 5.0
    return np.concatenate([lat, np.full((5, 3), 0.25), [[np.nan, 0, 0], [1e12, -3e11, 5.0], [-4.0, 7.0, 1.0]]])


# ---- tests ----

def test_restatement_equals_the_definition():
    rng = np.random.default_rng(17)
    sets = [(lattice_set(), (2.0, 2.0000001, 2.9, 3.5), 0, 0), (rng.uniform(-6, 6, (200, 3)), (0.7, 2.5, 6.0), 3, 4)]
    seen = set()
    for x, radii, first, short in sets:
        n = len(x)
        for radius in radii:
            for count in (n - first - short,):
                lists = brute_neighbours(x, first, count, radius)
                for kind in (HINGE2, INVERSE, COUNT):
                    for k, weight, eps in ((1, 1.0, 0.0), (8, -2.5, 1e-3), (32, 0.3, 0.0)):
                        got, gf = proximity_ref(x, first, count, k, radius, kind, weight, eps)
                        want, wf = brute_force(lists, k, radius, kind, weight, eps)
                        assert np.array_equal(gf, wf), (radius, k)
                        assert same_bits(got, want), (radius, kind, k, np.flatnonzero(got.view(np.int64) != want.view(np.int64))[:5])
                        seen.add((int(gf.max()) > k, int(gf.min()) == 0))
    assert any(c for c, _ in seen) and any(e for _, e in seen)  # capped rows and empty rows both occurred
    # worlds: a scene stacked on itself, labels by copy
    x = np.concatenate([rng.uniform(-3, 3, (30, 3))] * 3)
    worlds = np.repeat(np.array([7, -1, 2 ** 31 - 1]), 30)
    lists = brute_neighbours(x, 10, 70, 2.5, worlds)
    for kind in (HINGE2, INVERSE, COUNT):
        got, gf = proximity_ref(x, 10, 70, 8, 2.5, kind, 1.5, 0.25, worlds)
        want, wf = brute_force(lists, 8, 2.5, kind, 1.5, 0.25)
        assert np.array_equal(gf, wf) and same_bits(got, want)
        alone, af = proximity_ref(x[:30], 0, 30, 8, 2.5, kind, 1.5, 0.25)
        assert same_bits(got[20:50], alone) and np.array_equal(gf[20:50], af)
    assert (proximity_ref(x, 10, 70, 8, 2.5, COUNT, 1.5, 0.25)[1] >= 2).all()  # without labels the copies see each other


def test_restatement_on_the_special_rows():
    x = lattice_set()
    n = len(x)
    with np.errstate(invalid="ignore"):
        far = np.sqrt(((x[:216] - 0.25) ** 2).sum(axis=1)) > 2.5                   # lattice points away from the coincident five
    term, found = proximity_ref(x, 0, n, 4, 2.0, HINGE2, 1.0, 0.0)
    assert far.sum() > 150 and (found[:216][far] == 0).all() and same_bits(term[:216][far], np.zeros(far.sum()))  # strict <: 2 m is outside
    assert (found[216:221] >= 4).all() and same_bits(term[216:221], np.full(5, 16.0))  # coincident: d2 = 0, g = radius, four times
    assert found[n - 3] == 0 and same_bits(term[n - 3], 0.0)                       # the NaN UAV adds +0.0
    assert np.isposinf(proximity_ref(x, 0, n, 4, 2.0, INVERSE, 1.0, 0.0)[0][216:221]).all()
    assert np.isfinite(proximity_ref(x, 0, n, 4, 2.0, INVERSE, 1.0, 1e-3)[0]).all()
    assert same_bits(add_bits(np.array([-0.0]), np.array([0.0])), [0.0])           # -0.0 with no neighbour becomes +0.0


def test_symbol_is_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm, tensors
    assert hasattr(C.CDLL(swarm.LIB_PATH), "mrs_swarm_proximity_cost_device")
    assert "mrs_swarm_proximity_cost_device" in swarm.ABI_SYMBOLS
    assert callable(getattr(swarm.Swarm, "proximity_cost_device", None)) and callable(getattr(tensors, "proximity_cost", None))


def test_header_prototype_equals_the_argtypes(mrs):
    from mrs_multirotor_simulator_amd import swarm
    names, types = abi_prototype("mrs_swarm_proximity_cost_device")
    assert names == NAMES
    got = swarm.load_library().mrs_swarm_proximity_cost_device.argtypes
    assert [TYPES[t] for t in types] == list(got), (types, got)


def test_header_values_equal_the_python_ones(mrs):
    from mrs_multirotor_simulator_amd import swarm, tensors
    vals = {name: int(v) for name, v in re.findall(r"\b(MRS_PROX_[A-Z0-9_]+)\s*=\s*(\d+)", abi_header())}
    assert vals == {"MRS_PROX_HINGE2": 0, "MRS_PROX_INVERSE": 1, "MRS_PROX_COUNT": 2}
    for name, v in vals.items():
        assert getattr(swarm, name[4:]) == getattr(tensors, name[4:]) == v, name
    assert (HINGE2, INVERSE, COUNT) == (tensors.PROX_HINGE2, tensors.PROX_INVERSE, tensors.PROX_COUNT)


_Swarm = stand_in("proximity_cost_device")


def test_proximity_cost_refuses_bad_tensors(monkeypatch):
    """CPU tensors dressed as cuda tensors (only .device is faked; nothing is launched)"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    on = fake_cuda(monkeypatch)
    g, f64, i32 = _Swarm(), torch.float64, torch.int32
    cases = [
        (dict(out=torch.zeros(100, dtype=f64)), "is on cpu"),
        (dict(out=on(torch.zeros(100, dtype=f64), 1)), "the swarm lives on cuda:0"),
        (dict(out=on(torch.zeros(100, dtype=torch.float32))), "always torch.float64"),
        (dict(out=on(torch.zeros(99, dtype=f64))), "expected a vector of 100 elements"),
        (dict(out=on(torch.zeros(100, 1, dtype=f64))), "expected a vector of 100 elements"),
        (dict(out=on(torch.zeros(200, dtype=f64)[::2])), "vector is not contiguous"),
        (dict(out=[0.0] * 100), "expected a torch.Tensor"),
        (dict(out=None, accumulate=True), "accumulate=True needs the `out` vector"),
        (dict(found=torch.zeros(100, dtype=i32)), "is on cpu"),
        (dict(found=on(torch.zeros(100, dtype=i32), 1)), "the swarm lives on cuda:0"),
        (dict(found=on(torch.zeros(100, dtype=torch.int64))), "expected torch.int32"),
        (dict(found=on(torch.zeros(101, dtype=i32))), "expected a vector of 100 elements"),
        (dict(found=on(torch.zeros(200, dtype=i32)[::2])), "vector is not contiguous"),
        (dict(found=3), "expected a torch.Tensor"),
        (dict(first=10, count=50, out=on(torch.zeros(90, dtype=f64))), "expected a vector of 50 elements"),
    ]
    for kw, msg in cases:
        args = dict(out=on(torch.zeros(kw.get("count", 100), dtype=f64)))
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            T.proximity_cost(g, 5.0, **args)
    # a well-formed call passes every check of the tensor layer: it is the stand-in's library call that raises
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    for kw in (dict(), dict(accumulate=True), dict(found=on(torch.zeros(100, dtype=i32))), dict(kind=T.PROX_INVERSE, eps=0.1, k=32)):
        with pytest.raises(AssertionError, match="proximity_cost_device"):
            T.proximity_cost(g, 5.0, out=on(torch.zeros(100, dtype=f64)), **kw)


def test_proximity_cost_test_compiles(mrs):
    """tests/cpp/proximity_cost_test.cpp builds against the facade and the HIP runtime (run on the GPU by test_proximity_cost_gpu.py)"""
    from test_device_io_gpu import build_cpp
    assert os.path.exists(build_cpp("proximity_cost_test"))
