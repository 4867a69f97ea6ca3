"""Builds libmrs_swarm.so (HIP kernels + C ABI) in-tree for gfx950 with hipcc.

hipcc cross-compiles without a GPU, so this also is the "does it build" check on the CPU-only container.
"""
import contextlib
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmrs_swarm.so")
ARCH = "gfx950"

# (source, -ffp-contract) — the LITERAL kernel and all host/init arithmetic must not be FMA-contracted
UNITS = [
    ("step_kernel_literal.hip", "off"),
    ("step_kernel_fast.hip", "fast"),
    ("collide.hip", "off"),
    ("collide_export.hip", "off"),
    ("outputs.hip", "off"),
    ("device_io.hip", "off"),  # off: its observation rows equal the publisher payloads of outputs.hip bit for bit
    ("nearest.hip", "off"),  # off: d2 = ((dx*dx) + dy*dy) + dz*dz literally, which a numpy restatement reproduces bit for bit
    ("obstacles.hip", "off"),  # off: the signed distances of include/mrs_swarm.h literally, which a numpy restatement reproduces bit for bit
    ("obstacle_contact.hip", "off"),  # off: thr = (arm_length + prop_radius) + margin and the same signed distances, bit for bit against numpy
    ("range_scan.hip", "off"),  # off: the ray tests of include/mrs_swarm.h literally, which a numpy restatement reproduces bit for bit
    ("range_scan_uavs.hip", "off"),  # off: the same ray tests for UAV spheres, bit for bit against the numpy restatement
    ("nearest_visible.hip", "off"),  # off: d2, the sight line's direction and the same ray tests, bit for bit against the numpy restatement
    ("snapshot.hip", "off"),  # no arithmetic (records are copied bit for bit); off like every other unit
    # host side: C ABI, single-GPU tick, sharded tick, the three transports (transport_local and transport_peer hold the kernels of
    # their collectives, the others none)
    ("host_api.hip", "off"),
    ("tick_single.hip", "off"),
    ("tick_sharded.hip", "off"),
    ("transport_rccl.hip", "off"),
    ("transport_local.hip", "off"),
    ("transport_peer.hip", "off"),
]
DEPS = ["step_device.inc", "rollout_device.inc", "rollout_rate_device.inc", "rollout_cost_device.inc", "rollout_tick_device.inc", "collide_device.inc", "collide_work.h", "swarm_layout.h", "pose_math.h", "obs_row.h", "hip_owned.h", "host_internal.h", "sharded_protocol.h", "obstacle_grid.h", "obstacle_set.h", "obstacle_contact.h", "range_scan_math.h", "range_scan_common.h", "nn_hash.h", "nn_slot.h", "sight_math.h", os.path.join("..", "..", "include", "mrs_swarm.h")]


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: libmrs_swarm.so cannot be built (there is no CPU fallback)")
    return exe


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)


def build_library(force=False, verbose=False, out=None, extra_flags=None):
    """out, extra_flags: a variant for the measurement tools (tools/build_variants.sh), linked to `out`.  extra_flags maps unit names
    to lists of extra compiler flags: those units are compiled into a temporary directory, every other unit is the regular object."""
    extra_flags = extra_flags or {}
    if not set(extra_flags) <= {src for src, _ in UNITS} or (extra_flags and not out):
        raise ValueError("a variant names units of UNITS and is linked to a path of its own")
    hipcc = _hipcc()
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    deps = [os.path.join(CSRC, d) for d in DEPS]
    lib = out or LIB
    with tempfile.TemporaryDirectory() if extra_flags else contextlib.nullcontext() as vardir:
        objs = []
        for src, contract in UNITS:
            s = os.path.join(CSRC, src)
            o = os.path.join(vardir if src in extra_flags else objdir, src.replace(".hip", ".o"))
            if force or src in extra_flags or _stale(o, [s] + deps):
                _run([hipcc, "-O3", f"--offload-arch={ARCH}", "-fPIC", "-std=c++17", f"-ffp-contract={contract}", "-fno-fast-math", "-Wall",
                      "-Wno-unused-function", *extra_flags.get(src, ()), "-c", s, "-o", o], verbose)
            objs.append(o)
        if force or extra_flags or _stale(lib, objs):
            _run([hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", lib] + objs, verbose)
    return lib


if __name__ == "__main__":  # no options: the library, from scratch; --out PATH [--flags UNIT=FLAGS ...]: a variant
    import argparse
    import shlex

    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--flags", action="append", default=[], metavar="UNIT=FLAGS", help="e.g. collide.hip=-DMRS_SKIN=0.75")
    a = ap.parse_args()
    variant = {}
    for unit, _, flags in (f.partition("=") for f in a.flags):
        variant.setdefault(unit, []).extend(shlex.split(flags))
    print(build_library(force=not a.out, verbose=not a.out, out=a.out, extra_flags=variant))
