"""Collision worlds without a GPU: the scenario generator's preconditions, the per-world restatement against the definition and
against the reference's own kd-tree sets, the new symbols (exported, mirrored in swarm.py, declared in the header), the tensor checks
of tensors.set_worlds, and tests/cpp/worlds_test.cpp (the facade compiles; refusals that need no device)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import collision_thresholds as ct
import collision_worlds as cw
from collision_threshold_swarms import cluster_preconditions
from helpers import ROOT, abi_header, fake_cuda
from test_device_io_gpu import build_cpp

SYMBOLS = ("mrs_swarm_set_worlds", "mrs_swarm_get_worlds", "mrs_swarm_set_worlds_device")


def definition(pos, world, radius2):
    """{ j : world[j] == world[i], j != i, d2(i, j) < radius2 } with d2 = ((0 + dx^2) + dy^2) + dz^2, dx = x_i - x_j — pair by pair"""
    n = len(pos)
    out = []
    for i in range(n):
        d = pos[i][None, :] - pos
        d2 = ((0.0 + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep = (d2 < radius2) & (world == world[i])
        keep[i] = False
        out.append(np.nonzero(keep)[0])
    return out


@pytest.mark.parametrize("interleaved", [False, True], ids=["contiguous", "interleaved"])
def test_stacked_scenario_preconditions(interleaved):
    pos, world, af = cw.stacked(interleaved)
    parts = cw.split(world)
    assert len(pos) == 150 and [len(i) for _, i in parts] == [50, 50, 50] and [w for w, _ in parts] == list(cw.LABELS)
    assert min(cw.LABELS) < 0 and len(set(cw.LABELS)) == 3
    (_, a), (_, b), (_, c) = parts
    assert np.array_equal(pos[a], pos[b]) and not np.array_equal(pos[a], pos[c]), "world 1 is world 0's positions, world 2 is not"
    assert np.array_equal(af[a], af[b]) and len(set(af.tolist())) == 4
    assert np.array_equal(np.diff(a) == 1, np.full(49, not interleaved))
    arm, prop, mass = ct.constants(af)
    for crash in (False, True):
        r = cw.restatement(pos, world, arm, prop, mass, crash)
        touched = r["crashed"] != 0 if crash else np.abs(r["force"]).sum(axis=1) > 0
        for _, idx in parts:
            assert touched[idx].sum() >= 8, "a world without contacts"
        assert np.isfinite(r["force"]).all()
    lists = cw.list_sets(pos, world)
    assert 4 < max(len(x) for x in lists) <= cw.LIST_CAP
    z = np.zeros(len(pos))
    assert max(len(x) for x in ct.restatement(pos, z, z, z, False, radius2=ct.LIST_R2)["neighbours"]) > cw.LIST_CAP, "one world would fit the lists too"
    # both orders hold the same three swarms
    p0, w0, _ = cw.stacked(False)
    for (_, i), (_, j) in zip(parts, cw.split(w0)):
        assert np.array_equal(pos[i], p0[j])


def test_many_pairs_clusters_and_wide_preconditions():
    pos, world, _ = cw.many_pairs()  # (asserts 79 within the list radius, 1 in the own world)
    assert len(pos) == 80 and len(set(world.tolist())) == 40
    pos, world, af, cl = cw.clusters()
    n = len(pos) // 2
    assert np.array_equal(pos[:n], pos[n:]) and set(world[:n].tolist()) == {5} and set(world[n:].tolist()) == {-5}
    cluster_preconditions(pos[:n], af[:n], cl)
    pos, world, _ = cw.wide()
    assert len(pos) == 300 and sorted(np.unique(world, return_counts=True)[1].tolist()) == [50] * 6
    lists = cw.list_sets(pos, world)
    z = np.zeros(300)
    assert max(len(x) for x in lists) <= cw.LIST_CAP < max(len(x) for x in ct.restatement(pos, z, z, z, False, radius2=ct.LIST_R2)["neighbours"])
    assert sum(len(x) for x in lists) > 300


@pytest.mark.parametrize("name", ["stacked", "interleaved", "many pairs", "clusters", "wide"])
def test_restatement_is_the_definition(name):
    pos, world = {"stacked": cw.stacked(False), "interleaved": cw.stacked(True), "many pairs": cw.many_pairs(), "clusters": cw.clusters(),
                  "wide": cw.wide()}[name][:2]
    z = np.zeros(len(pos))
    for r2 in (3.0, ct.LIST_R2):
        got = cw.restatement(pos, world, z, z, z, False, radius2=r2)["neighbours"]
        want = definition(pos, world, r2)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), f"{name}: neighbour sets at radius^2 {r2}"
    # coincident UAVs of different worlds never meet
    if name in ("stacked", "clusters"):
        got = cw.restatement(pos, world, z, z, z, False)["neighbours"]
        for i in range(len(pos)):
            assert not np.any(np.all(pos[got[i]] == pos[i], axis=1))


@pytest.mark.parametrize("name", ["dense", "sparse", "grid12", "tmux400"])
def test_restatement_per_world_against_the_reference_kdtree(oracle, name):
    """the reference's nanoflann radiusSearch(3.0) sets (tests/golden/nanoflann_radius_sets.npz), three interleaved worlds: what the
    kd-tree returned for i, restricted to i's world and without i, is the restatement's set; where oracle/_ref is built, the library
    queried on each world's UAVs alone returns the same"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "nanoflann_radius_sets.npz"))
    pts, off, idx = (g[f"{name}_{k}"] for k in ("points", "offsets", "indices"))
    n = len(pts)
    world = np.array(cw.LABELS, dtype=np.int32)[np.arange(n) % 3]
    z = np.zeros(n)
    got = cw.restatement(pts, world, z, z, z, False)["neighbours"]
    for i in range(n):
        ref = sorted(int(j) for j in idx[off[i]:off[i + 1]] if j != i and world[j] == world[i])
        assert got[i].tolist() == ref, f"{name}: UAV {i}"
    if oracle.ref_lib() is not None:
        for _, members in cw.split(world):
            lo, li, _ = oracle.ref_radius_neighbours(pts[members], 3.0, 10)
            for k, i in enumerate(members):
                assert sorted(int(members[j]) for j in li[lo[k]:lo[k + 1]] if j != k) == got[i].tolist(), f"{name}: live kd-tree, UAV {i}"


def test_symbols_exported_mirrored_and_declared(mrs):
    from mrs_multirotor_simulator_amd import swarm
    L = C.CDLL(swarm.LIB_PATH)
    header = abi_header()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in swarm.ABI_SYMBOLS, name
        assert len(getattr(mrs.load_library(), name).argtypes) == len(re.search(name + r"\s*\(([^)]*)\)", header).group(1).split(",")), name
    for method in ("set_worlds", "get_worlds", "set_worlds_device"):
        assert callable(getattr(mrs.Swarm, method))
    facade = open(os.path.join(ROOT, "include", "mrs_multirotor_simulator", "uav_system", "uav_system.hpp")).read()
    assert all(f"void {m}(" in facade or f"> {m}(" in facade for m in ("setWorlds", "getWorlds", "setWorldsDevice"))


class _FakeSwarm:
    n = 100
    calls = []

    @staticmethod
    def device():
        return 0

    def set_worlds_device(self, *a):
        self.calls.append(a)


def test_tensors_set_worlds_refuses_bad_tensors(mrs, monkeypatch):
    """a host tensor, and (dressed as cuda:0 / cuda:1, as test_nearest does) wrong dtype, other device, wrong shape, too many labels:
    ValueError before any library call; a good vector reaches the library with its pointer, count and first"""
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    g = _FakeSwarm()
    with pytest.raises(ValueError, match="is on cpu"):
        T.set_worlds(g, torch.zeros(100, dtype=torch.int32))
    on = fake_cuda(monkeypatch)
    monkeypatch.setattr(T, "_stream", lambda dev: 0)
    i32 = torch.int32
    with pytest.raises(ValueError, match="dtype"):
        T.set_worlds(g, on(torch.zeros(100, dtype=torch.int64)))
    with pytest.raises(ValueError, match="dtype"):
        T.set_worlds(g, on(torch.zeros(100)))
    with pytest.raises(ValueError, match="lives on cuda:0"):
        T.set_worlds(g, on(torch.zeros(100, dtype=i32), 1))
    with pytest.raises(ValueError, match="int32 vector"):
        T.set_worlds(g, on(torch.zeros((100, 1), dtype=i32)))
    with pytest.raises(ValueError, match="do not fit"):
        T.set_worlds(g, on(torch.zeros(101, dtype=i32)))
    with pytest.raises(ValueError, match="do not fit"):  # a row too short for the range is a range too long for the row
        T.set_worlds(g, on(torch.zeros(60, dtype=i32)), first=41)
    with pytest.raises(ValueError, match="not contiguous"):
        T.set_worlds(g, on(torch.zeros(200, dtype=i32)[::2]))
    assert not g.calls
    w = on(torch.zeros(60, dtype=i32))
    T.set_worlds(g, w, first=40)
    assert g.calls == [(40, 60, w.data_ptr(), 0)]


def test_worlds_test_compiles_and_refuses_without_a_device(mrs):
    """tests/cpp/worlds_test.cpp builds against the facade; without an argument it checks the refusals that never reach the device"""
    out = subprocess.run([build_cpp("worlds_test")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok refusals_without_a_device" in out.stdout, out.stdout + out.stderr
