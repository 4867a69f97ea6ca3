"""CPU-side checks of the device-resident I/O family (include/mrs_swarm.h, "device-resident callers"): the symbols are exported, the
header's MRS_OBS_* / MRS_DTYPE_* values are the ones mrs_multirotor_simulator_amd.tensors uses, mrs_swarm_gather_width returns the
table's widths, and tensors.check_tensor refuses what the library must never see.  CPU tensors only: no pointer reaches the library."""
import ctypes as C
import os
import re

import pytest

from helpers import ROOT, abi_header, fake_cuda

NEW_SYMBOLS = ["mrs_swarm_device", "mrs_swarm_gather_width", "mrs_swarm_set_input_device", "mrs_swarm_gather_device",
               "mrs_swarm_get_crashed_device", "mrs_swarm_reset_device"]
WIDTHS = {"POS": 3, "VEL": 3, "VEL_BODY": 3, "ROT": 9, "QUAT": 4, "OMEGA": 3, "IMU": 3, "RPM": 8}


def header_enums():
    vals = {}
    for name, expr in re.findall(r"\b(MRS_(?:OBS|DTYPE)_[A-Z0-9_]+)\s*=\s*([^,}\n]+)", abi_header()):
        vals[name] = eval(expr.strip(), {})  # "1 << 3", "0xFF", "0"
    return vals


def test_new_symbols_are_exported_and_listed(mrs):
    from mrs_multirotor_simulator_amd import swarm
    L = C.CDLL(swarm.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in swarm.ABI_SYMBOLS, name


def test_header_values_equal_the_python_ones(mrs):
    from mrs_multirotor_simulator_amd import tensors
    vals = header_enums()
    assert vals["MRS_DTYPE_F64"] == tensors.DTYPE_F64 == 0
    assert vals["MRS_DTYPE_F32"] == tensors.DTYPE_F32 == 1
    for i, g in enumerate(WIDTHS):
        assert vals[f"MRS_OBS_{g}"] == getattr(tensors, f"OBS_{g}") == 1 << i, g
    assert vals["MRS_OBS_ALL"] == tensors.OBS_ALL == 0xFF


def test_gather_width_table(mrs):
    from mrs_multirotor_simulator_amd import swarm, tensors
    for g, w in WIDTHS.items():
        assert swarm.gather_width(getattr(tensors, f"OBS_{g}")) == w, g
    assert swarm.gather_width(tensors.OBS_ALL) == 36
    assert swarm.gather_width(0) == 0
    assert swarm.gather_width(tensors.OBS_POS | tensors.OBS_VEL | tensors.OBS_ROT | tensors.OBS_OMEGA) == 18
    with pytest.raises(mrs.MrsError, match="unknown observation group"):
        swarm.gather_width(0x100)


def test_check_tensor_refuses_bad_tensors():
    import torch
    from mrs_multirotor_simulator_amd.tensors import check_tensor
    f32 = torch.float32
    with pytest.raises(ValueError, match="is on cpu"):
        check_tensor(torch.zeros(10, 3), 10, 3, f32, 0)
    with pytest.raises(ValueError, match="expected a torch.Tensor"):
        check_tensor([[0.0] * 3] * 10, 10, 3, f32, 0)
    with pytest.raises(ValueError, match="is on cpu"):
        check_tensor(torch.zeros(10, dtype=torch.bool), 10, None, torch.bool, 0)


def test_check_tensor_rules_past_the_device_check(monkeypatch):
    """The checks behind the device test, on CPU tensors dressed as cuda:0 ones (only .device is faked; nothing is launched)."""
    import torch
    from mrs_multirotor_simulator_amd import tensors
    on = fake_cuda(monkeypatch)
    f32, f64 = torch.float32, torch.float64
    ok = on(torch.zeros(10, 4))
    assert tensors.check_tensor(ok, 10, 4, f32, 0) == 4
    assert tensors.check_tensor(on(torch.zeros(10, 6)[:, :4]), 10, 4, f32, 0) == 6  # padded rows: the stride is the parent's width
    assert tensors.check_tensor(on(torch.zeros(10)), 10, None, f32, 0) == 1
    with pytest.raises(ValueError, match="the swarm lives on cuda:0"):
        tensors.check_tensor(on(torch.zeros(10, 4), 1), 10, 4, f32, 0)
    with pytest.raises(ValueError, match="dtype torch.float32, expected torch.float64"):
        tensors.check_tensor(ok, 10, 4, f64, 0)
    with pytest.raises(ValueError, match="stride of the last dimension is 10"):
        tensors.check_tensor(on(torch.zeros(4, 10).t()), 10, 4, f32, 0)
    with pytest.raises(ValueError, match=r"expected a \[10, >= 4\] matrix"):
        tensors.check_tensor(on(torch.zeros(9, 4)), 10, 4, f32, 0)
    with pytest.raises(ValueError, match=r"expected a \[10, >= 5\] matrix"):
        tensors.check_tensor(ok, 10, 5, f32, 0)
    with pytest.raises(ValueError, match=r"expected a \[10, >= 4\] matrix"):
        tensors.check_tensor(on(torch.zeros(40)), 10, 4, f32, 0)
    with pytest.raises(ValueError, match="expected a vector of 10 elements"):
        tensors.check_tensor(ok, 10, None, f32, 0)
    with pytest.raises(ValueError, match="vector is not contiguous"):
        tensors.check_tensor(on(torch.zeros(20)[::2]), 10, None, f32, 0)


def test_package_import_does_not_import_torch():
    import subprocess
    import sys
    code = "import sys; import mrs_multirotor_simulator_amd; print('torch' in sys.modules)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    assert out == "False"


def test_device_io_test_compiles(mrs):
    """tests/cpp/device_io_test.cpp builds against the facade and the HIP runtime (run on the GPU by test_device_io_gpu.py)."""
    from test_device_io_gpu import build_cpp
    assert os.path.exists(build_cpp())
