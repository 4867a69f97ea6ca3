"""The table of fused step kernels stays complete: every MRS_FUSED_RUN_KERNEL(name, ...) instantiation of step_device.inc has a row in
test_run_fusion_gpu.FUSED_KERNELS naming the cases that force it, no row names a kernel that no longer exists, and every named case is
a case of that file."""
import os
import re

import step_regimes as R
import test_run_fusion_gpu as F

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mrs_multirotor_simulator_amd", "csrc",
                   "step_device.inc")


def test_every_fused_kernel_has_a_row_and_every_row_a_kernel():
    with open(SRC) as f:
        names = set(re.findall(r"^MRS_FUSED_RUN_KERNEL\(\s*(\w+)\s*,", f.read(), flags=re.M))
    assert len(names) == 2 * (F.D - 1), sorted(names)  # depths 2 .. D, with and without nt
    assert names == set(F.FUSED_KERNELS), sorted(names ^ set(F.FUSED_KERNELS))


def test_every_row_names_cases_that_exist():
    sizes = {"37", "64", "1000", str(F.N_SPLIT), str(F.N_BUF), str(R.N_BUF_LAST), str(R.N_W3_FIRST)}
    for kernel, where in F.FUSED_KERNELS.items():
        assert where, kernel
        for w in where:
            m = re.fullmatch(r"(\w+)\[(\d+)-(literal|fast)\]", w)
            assert m and callable(getattr(F, m.group(1), None)) and m.group(2) in sizes, f"{kernel}: {w}"
            # the launcher's rule (step_regimes.py, held against the source by test_step_regimes.py): *_nt_fuseD where the single
            # step is an nt kernel
            nt = R.fused_nt(int(m.group(2)), m.group(3) == "fast")
            assert nt == ("_nt_" in kernel), f"{kernel}: {w} launches the other addressing variant"
