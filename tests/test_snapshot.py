"""CPU-side checks of the state snapshots (include/mrs_swarm.h, "state snapshots"): the two calls are exported and listed, a C++
compiler lays mrs_uav_snapshot_t out as SNAPSHOT_DTYPE says (496 B, every offset), the header's MRS_SNAP_* values are the Python ones,
tensors.save / load / snapshot_fields refuse what the library must never see, and tests/cpp/snapshot_test.cpp compiles.  CPU tensors
only: no pointer reaches the library."""
import ctypes as C
import os
import re
import subprocess

import pytest

from helpers import ROOT, abi_header, fake_cuda, stand_in

NEW_SYMBOLS = ["mrs_swarm_save_device", "mrs_swarm_load_device"]


def header_values():
    src = abi_header()
    vals = {name: eval(expr.strip(), {}) for name, expr in re.findall(r"\b(MRS_SNAP_[A-Z_]+)\s*=\s*([^,}\n]+)", src)}
    m = re.search(r"#define\s+MRS_SNAP_MAGIC\s+(0x[0-9A-Fa-f]+)u", src)
    vals["MRS_SNAP_MAGIC"] = int(m.group(1), 16)
    return vals


def test_new_symbols_are_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm
    L = C.CDLL(swarm.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in swarm.ABI_SYMBOLS, name


def test_header_values_equal_the_python_ones():
    from mrs_multirotor_simulator_amd import swarm, tensors
    vals = header_values()
    want = {"CRASHED": 1, "TAKEOFF": 2, "VPREV_SPLIT": 4, "LOADED": 0, "SKIPPED": 1, "BAD_AIRFRAME": 2, "BAD_INDEX": 3, "BAD_MAGIC": 4,
            "MAGIC": 0x50414E53}
    for name, v in want.items():
        assert vals[f"MRS_SNAP_{name}"] == getattr(swarm, f"SNAP_{name}") == getattr(tensors, f"SNAP_{name}") == v, name
    assert tensors.SNAP_BYTES == swarm.SNAPSHOT_DTYPE.itemsize == 496


def test_snapshot_record_layout_in_cpp(tmp_path):
    """what a C++ compiler makes of the header: sizeof and the offset of every field equal SNAPSHOT_DTYPE's"""
    from mrs_multirotor_simulator_amd import swarm
    dt = swarm.SNAPSHOT_DTYPE
    lines = ['#include <cstddef>', '#include "mrs_swarm.h"', f"static_assert(sizeof(mrs_uav_snapshot_t) == {dt.itemsize}, \"size\");",
             "static_assert(alignof(mrs_uav_snapshot_t) == 8, \"align\");"]
    for name in dt.names:
        lines.append(f"static_assert(offsetof(mrs_uav_snapshot_t, {name}) == {dt.fields[name][1]}, \"{name}\");")
        lines.append(f"static_assert(sizeof(mrs_uav_snapshot_t::{name}) == {dt.fields[name][0].itemsize}, \"size of {name}\");")
    lines.append("int main() { return 0; }")
    src = tmp_path / "snapshot_layout.cpp"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "snapshot_layout.o")])
    assert dt.itemsize % 16 == 0
    # the 60 doubles are the state columns F_X .. F_PID+23 in column order (swarm_layout.h)
    layout = open(os.path.join(ROOT, "mrs_multirotor_simulator_amd", "csrc", "swarm_layout.h")).read()
    col = {k: int(v) for k, v in re.findall(r"\b(F_[A-Z]+)\s*=\s*(\d+)", layout)}
    for name, f in (("x", "F_X"), ("v", "F_V"), ("v_prev", "F_VPREV"), ("R", "F_R"), ("omega", "F_W"), ("motor_rpm", "F_RPM"),
                    ("imu_acceleration", "F_IMU"), ("external_force", "F_FEXT"), ("initial_z", "F_INITZ"), ("pid", "F_PID")):
        assert dt.fields[name][1] == 8 * col[f], name
    assert dt.fields["flags"][1] == 8 * col["F_CMD"]


def test_snapshot_fields_share_memory():
    import torch
    from mrs_multirotor_simulator_amd import swarm, tensors
    rec = torch.zeros((5, tensors.SNAP_BYTES), dtype=torch.uint8)
    f = tensors.snapshot_fields(rec)
    assert set(f) == {n for n in swarm.SNAPSHOT_DTYPE.names if n != "_reserved"}
    assert f["R"].shape == (5, 3, 3) and f["pid"].shape == (5, 24) and f["initial_z"].shape == (5,) and f["flags"].dtype == torch.int32
    f["x"][:, 1] = 2.5
    f["R"][3, 2, 0] = -1.0
    f["pid"][4, 23] = 7.0
    f["initial_z"][2] = 3.0
    f["airframe"][1] = 9
    f["magic"][:] = tensors.SNAP_MAGIC
    a = rec.numpy().view(swarm.SNAPSHOT_DTYPE).reshape(5)
    assert (a["x"][:, 1] == 2.5).all() and a["R"][3, 2, 0] == -1.0 and a["pid"][4, 23] == 7.0 and a["initial_z"][2] == 3.0
    assert a["airframe"][1] == 9 and (a["magic"] == tensors.SNAP_MAGIC).all()
    assert (a["_reserved"] == 0).all() and (a["v"] == 0).all() and (a["flags"] == 0).all()
    with pytest.raises(ValueError, match="uint8"):
        tensors.snapshot_fields(torch.zeros((5, 62), dtype=torch.float64))
    with pytest.raises(ValueError, match="not contiguous"):
        tensors.snapshot_fields(torch.zeros((5, 2 * tensors.SNAP_BYTES), dtype=torch.uint8)[:, :tensors.SNAP_BYTES])


_NoSwarm = stand_in("save_device", "load_device")  # fails the test if any check lets a call through to the library


@pytest.fixture
def on(monkeypatch):
    """CPU tensors dressed as cuda:<index> ones (only .device is faked; nothing is launched), as test_device_io does"""
    return fake_cuda(monkeypatch)


def test_save_and_load_refuse_bad_tensors(on):
    import torch
    from mrs_multirotor_simulator_amd import tensors as T
    sw, B = _NoSwarm(), T.SNAP_BYTES
    u8 = torch.uint8
    with pytest.raises(ValueError, match="is on cpu"):
        T.save(sw, 0, 10, out=torch.zeros((10, B), dtype=u8))
    with pytest.raises(ValueError, match="is on cpu"):
        T.load(sw, torch.zeros((10, B), dtype=u8))
    with pytest.raises(ValueError, match="the swarm lives on cuda:0"):
        T.save(sw, 0, 10, out=on(torch.zeros((10, B), dtype=u8), 1))
    with pytest.raises(ValueError, match="dtype torch.float64, expected torch.uint8"):
        T.save(sw, 0, 10, out=on(torch.zeros((10, 62), dtype=torch.float64)))
    with pytest.raises(ValueError, match="dtype torch.float64, expected torch.uint8"):
        T.load(sw, on(torch.zeros((10, 62), dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"expected a \[10, >= 496\] matrix"):
        T.save(sw, 0, 10, out=on(torch.zeros((9, B), dtype=u8)))
    with pytest.raises(ValueError, match=r"must be \[10, 496\]"):
        T.save(sw, 0, 10, out=on(torch.zeros((10, B + 16), dtype=u8)))
    with pytest.raises(ValueError, match="records are not contiguous"):
        T.save(sw, 0, 10, out=on(torch.zeros((10, B + 16), dtype=u8)[:, :B]))
    with pytest.raises(ValueError, match="records are not contiguous"):
        T.load(sw, on(torch.zeros((10, 2 * B), dtype=u8)[:, B:]))
    with pytest.raises(ValueError, match="rows are not contiguous"):
        T.load(sw, on(torch.zeros((B, 10), dtype=u8).t()))
    with pytest.raises(ValueError, match="16-B boundary"):
        T.load(sw, on(torch.zeros(10 * B + 8, dtype=u8)[8:].view(10, B)))
    with pytest.raises(ValueError, match="records must be"):
        T.load(sw, on(torch.zeros(10 * B, dtype=u8)))
    recs = on(torch.zeros((4, B), dtype=u8))
    with pytest.raises(ValueError, match="dtype torch.int64, expected torch.int32"):
        T.load(sw, recs, index=on(torch.zeros(10, dtype=torch.int64)))
    with pytest.raises(ValueError, match="index must be an int32 vector"):
        T.load(sw, recs, index=on(torch.zeros((10, 1), dtype=torch.int32)))
    with pytest.raises(ValueError, match="vector is not contiguous"):
        T.load(sw, recs, index=on(torch.zeros(20, dtype=torch.int32)[::2]))
    with pytest.raises(ValueError, match="dtype torch.bool, expected torch.uint8"):
        T.load(sw, recs, index=on(torch.zeros(10, dtype=torch.int32)), status=on(torch.zeros(10, dtype=torch.bool)))
    with pytest.raises(ValueError, match="expected a vector of 10 elements"):
        T.load(sw, recs, index=on(torch.zeros(10, dtype=torch.int32)), status=on(torch.zeros(4, dtype=u8)))


def test_snapshot_test_compiles(mrs):
    """tests/cpp/snapshot_test.cpp builds against the facade and the HIP runtime (run on the GPU by test_snapshot_gpu.py)."""
    from test_device_io_gpu import build_cpp
    assert os.path.exists(build_cpp("snapshot_test"))
