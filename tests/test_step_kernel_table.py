"""The step-kernel matrix stays complete: every entry point step_device.inc compiles has a row in
test_step_variants_gpu.STEP_KERNELS naming the test that forces it, and no row names a kernel that no longer exists."""
import importlib
import os
import re

import step_regimes as R
import test_step_variants_gpu as V

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mrs_multirotor_simulator_amd", "csrc",
                   "step_device.inc")


def step_kernel_entry_points(text):
    """names of the MRS_STEP_KERNEL*(name, ...) instantiations, leaving out the measurement-only #ifdef MRS_EXP_* branches"""
    names, skip = set(), []  # skip: one flag per open #if, True inside the measurement-only branch
    for line in text.splitlines():
        s = line.strip()
        if s.startswith("#if"):
            skip.append(bool(re.match(r"#if(def|\s+defined)?\s*\(?\s*MRS_EXP_", s)))
        elif s.startswith("#else") or s.startswith("#elif"):
            skip[-1] = False
        elif s.startswith("#endif"):
            skip.pop()
        elif not any(skip):
            m = re.match(r"MRS_STEP_KERNEL\w*\(\s*(\w+)\s*,", s)
            if m:
                names.add(m.group(1))
    return names


def test_every_step_kernel_has_a_row_in_the_variant_matrix():
    with open(SRC) as f:
        names = step_kernel_entry_points(f.read())
    assert len(names) >= 24, sorted(names)
    table = set(V.STEP_KERNELS)
    assert not names - table, f"step kernels without a row in STEP_KERNELS: {sorted(names - table)}"
    assert not table - names, f"rows of STEP_KERNELS naming kernels step_device.inc no longer compiles: {sorted(table - names)}"


def test_every_row_names_a_test_and_form_that_exist():
    forms = {"test_single_gpu_variant": set(V.SINGLE_FORMS), "test_sharded_matrix": set(V.SHARDED_FORMS),
             "test_sharded_pointer_kernels": set(V.POINTER_FORMS)}
    for kernel, where in V.STEP_KERNELS.items():
        assert where, kernel
        for w in where:
            if "::" in w:  # a case of another module: the module has that test, and the case names a size step_regimes.py names
                m = re.fullmatch(r"(\w+)::(\w+)\[(?:(?:model|position)-)?(?:(\d+)-)?(literal|fast)\]", w)
                assert m and callable(getattr(importlib.import_module(m.group(1)), m.group(2), None)), f"{kernel}: {w} names no test"
                if m.group(3):
                    cascade = "[position-" in w
                    assert R.regime(int(m.group(3)), m.group(4) == "fast", cascade) == ("w3" if kernel.endswith("_w3") else "buf"), f"{kernel}: {w}"
                continue
            m = re.match(r"(\w+)\[(\w+)\]", w)
            assert m and callable(getattr(V, m.group(1), None)), f"{kernel}: {w} is no test of test_step_variants_gpu"
            assert m.group(2) in forms[m.group(1)], f"{kernel}: {m.group(1)} has no form {m.group(2)}"


def test_the_table_reader_leaves_out_measurement_branches():
    text = ("MRS_STEP_KERNEL(a_kernel, (64), true)\n#ifdef MRS_EXP_X\nMRS_STEP_KERNEL_BND(b_kernel, (64), false)\n#else\n"
            "MRS_STEP_KERNEL_BND(b_kernel, (64), true)\n#endif\n#ifdef MRS_EXP_Y\nMRS_STEP_KERNEL(c_only_measured, (64))\n#endif\n"
            "#if MRS_FAST\nMRS_STEP_KERNEL_COLL_P(d_kernel, (64), x)\n#endif\n")
    assert step_kernel_entry_points(text) == {"a_kernel", "b_kernel", "d_kernel"}
