"""The owning types of csrc/hip_owned.h (device buffer, pinned block, event, stream) WITHOUT a GPU: tests/cpp/hip_owned_test.cpp is
compiled against a malloc-backed stand-in for the HIP runtime (tests/cpp/hip_stub) that counts every call and can fail the k-th
allocation.  What the owners do on a real device is covered by tests/test_resource_lifetime_gpu.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hip_owned_cpp():
    cpp = os.path.join(ROOT, "tests", "cpp")
    exe = os.path.join(cpp, "hip_owned_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(cpp, "hip_stub"), os.path.join(cpp, "hip_owned_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    for tag in ("moves", "reserve", "failed_allocations", "event_idempotent", "destruction_order", "counters"):
        assert f"ok {tag}" in out.stdout, out.stdout
