"""step_regimes.py stays the launcher's rule: the thresholds of step_kernel_choice (step_device.inc) and of the two-stream rule
(tick_single.hip) are read out of the sources, step_regimes.regime() is held against a rule evaluated from THOSE numbers at every
threshold +-1 block, and every named size of the GPU tests must lie in the regime its name says.  No GPU."""
import os
import re

import pytest

import step_regimes as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mrs_multirotor_simulator_amd", "csrc")
MOVE = ("the launcher's thresholds moved: move the constants and the named sizes of tests/step_regimes.py with them (one size on each "
        "side of every threshold), and the cases of test_run_fusion_gpu.py, test_run_imu_elision_gpu.py and test_step_regimes_gpu.py "
        "follow; ")


def source_thresholds(step_text, tick_text, layout_text):
    """the numbers of the launcher's rule, from the lines that apply them"""
    def one(pattern, text, what):
        m = re.findall(pattern, text, flags=re.M)
        assert len(m) == 1, f"{what}: expected one match of {pattern!r} in the source, found {len(m)} - the rule has changed shape"
        return m[0]

    t = {}
    a, b = one(r"^\s*k\.w3\s*=.*\bnb > (\d+) \* (\d+)\)", step_text, "three-wave rule")
    t["w3_above"] = int(a) * int(b)
    t["nt_max"] = int(one(r"^\s*k\.nt\s*=.*\(nb <= (\d+) \|\| hbm_stream\)", step_text, "nt rule"))
    t["nt_cascade_max"] = int(one(r"^\s*k\.nt_cascade\s*=.*\(nb <= (\d+) \|\| hbm_stream\)", step_text, "cascade nt rule"))
    m, c, h = one(r"^\s*const bool hbm_stream\s*=.*sw\.npad \* \(variant == 1 \? ([\d.]+) : ([\d.]+)\) >= ([\d.e]+);", step_text,
                  "HBM-streaming rule")
    t["bytes_model"], t["bytes_cascade"], t["hbm_bytes"] = float(m), float(c), float(h)
    t["split_min_blocks"] = int(one(r"^\s*static const int split_min_blocks\s*=.*:\s*(\d+);", tick_text, "two-stream rule"))
    t["split_min_launches"] = int(one(r"^\s*const bool split\s*=.*>= split_min_blocks && \(n_steps \+ per_launch - 1\) / per_launch >= (\d+);",
                                      tick_text, "two-stream rule"))
    t["f_count"] = int(one(r"^\s*F_COUNT = (\d+)\s*$", layout_text, "state columns"))
    return t


def source_regime(t, n, fast, cascade):
    """step_kernel_choice, line by line, with the numbers read from the source"""
    nb = (n + 63) // 64
    npad = max(nb, 1) * 64
    buf = t["f_count"] * npad * 8 < 1 << 32
    hbm_stream = buf and fast and npad * (t["bytes_cascade"] if cascade else t["bytes_model"]) >= t["hbm_bytes"]
    w3 = buf and not hbm_stream and fast and nb > t["w3_above"]
    nt = buf and not w3 and fast and (nb <= (t["nt_cascade_max"] if cascade else t["nt_max"]) or hbm_stream)
    if not buf:
        return "pointer"
    if hbm_stream:
        assert nt
        return "hbm_nt"
    return "w3" if w3 else "nt" if nt else "buf"


@pytest.fixture(scope="module")
def T():
    texts = [open(os.path.join(CSRC, f)).read() for f in ("step_device.inc", "tick_single.hip", "swarm_layout.h")]
    return source_thresholds(*texts)


def test_the_constants_are_the_sources(T):
    mine = dict(w3_above=R.W3_ABOVE_BLOCKS, nt_max=R.NT_MAX_BLOCKS, nt_cascade_max=R.NT_CASCADE_MAX_BLOCKS, bytes_model=R.BYTES_MODEL,
                bytes_cascade=R.BYTES_CASCADE, hbm_bytes=R.HBM_BYTES, split_min_blocks=R.SPLIT_MIN_BLOCKS,
                split_min_launches=R.SPLIT_MIN_LAUNCHES, f_count=R.F_COUNT)
    moved = {k: (mine[k], T[k]) for k in mine if mine[k] != T[k]}
    assert not moved, MOVE + f"(step_regimes.py, source): {moved}"


def test_regime_is_the_sources_rule_at_every_threshold(T):
    """each threshold of the source, in blocks, +-1 block, with full and one-lane tail blocks; both families, both flavours"""
    edges = {T["nt_max"], T["nt_cascade_max"], T["w3_above"], T["split_min_blocks"], 1,
             int(T["hbm_bytes"] / T["bytes_model"]) // 64 + 1, int(T["hbm_bytes"] / T["bytes_cascade"]) // 64 + 1,
             ((1 << 32) // (T["f_count"] * 8)) // 64 + 1}
    seen = set()
    for nb in sorted(edges):
        for b in (nb - 1, nb, nb + 1):
            for n in ((b - 1) * 64 + 1, b * 64 - 1, b * 64, b * 64 + 1):
                if n < 1:
                    continue
                for fast in (False, True):
                    for cascade in (False, True):
                        want = source_regime(T, n, fast, cascade)
                        got = R.regime(n, fast, cascade)
                        assert got == want, MOVE + f"n={n} ({R.blocks(n)} blocks), fast={fast}, cascade={cascade}: regime() says {got}, the source {want}"
                        assert R.fuses(n, fast, cascade) == (not cascade and want != "pointer")
                        seen.add((fast, cascade, want))
    for fast, cascade in ((True, False), (True, True)):  # every regime of the table was met on both sides of its thresholds
        assert {r for f, c, r in seen if (f, c) == (fast, cascade)} == set(R.REGIMES), sorted(seen)
    assert {r for f, c, r in seen if not f} == {"buf", "pointer"}, "LITERAL takes the two-wave kernels at every size"


def test_every_named_size_lies_where_its_name_says(T):
    for name, (n, cascade, want) in R.NAMED.items():
        got = source_regime(T, n, True, cascade)
        assert got == want, MOVE + f"{name} = {n} ({R.blocks(n)} blocks, cascade={cascade}) is named for '{want}', the source launches '{got}' there"
        assert R.regime(n, True, cascade) == want and source_regime(T, n, False, cascade) == R.regime(n, False, cascade) == "buf", name
    # the pairs straddle their thresholds by one UAV, and the tail block of the upper size holds one lane
    for lo, hi, at in ((R.N_NT_LAST, R.N_BUF_FIRST, T["nt_max"]), (R.N_BUF_LAST, R.N_W3_FIRST, T["w3_above"]),
                       (R.N_CASCADE_NT_LAST, R.N_CASCADE_BUF_FIRST, T["nt_cascade_max"]),
                       (R.N_ONE_STREAM_LAST, R.N_TWO_STREAMS_FIRST, T["split_min_blocks"] - 1)):
        assert hi == lo + 1 and lo == at * 64 and R.blocks(lo) == at and R.blocks(hi) == at + 1, MOVE + f"{lo}, {hi} should straddle {at} blocks"
    assert (R.N_NT_LAST, R.N_BUF_FIRST, R.N_BUF_LAST, R.N_W3_FIRST, R.N_CASCADE_NT_LAST, R.N_CASCADE_BUF_FIRST) == \
        (121_600, 121_601, 131_072, 131_073, 57_600, 57_601), MOVE + "the cases written into the kernel tables name these sizes"


def test_the_two_stream_rule(T):
    for n in (R.N_ONE_STREAM_LAST, R.N_TWO_STREAMS_FIRST, R.N_BUF_LAST, R.N_W3_FIRST):
        for launches in (T["split_min_launches"] - 1, T["split_min_launches"]):
            want = (n + 63) // 64 >= T["split_min_blocks"] and launches >= T["split_min_launches"]
            assert R.two_streams(n, launches) == want, MOVE + f"n={n}, {launches} launches"
    assert not R.two_streams(R.N_ONE_STREAM_LAST, 100) and R.two_streams(R.N_TWO_STREAMS_FIRST, 4)
    # what the GPU cases count on: a fused run of 4D + 3 = 19 steps is five launches, a run of 7 unfused steps seven
    assert R.two_streams(R.N_W3_FIRST, (19 + 3) // 4) and R.two_streams(R.N_CASCADE_BUF_FIRST, 7) is False and R.two_streams(R.N_BUF_LAST, 7)


def test_fused_kernel_choice_follows_the_regime():
    """the fused launch is *_nt_fuseD exactly where the single step is an nt kernel; above 2048 blocks it stays the two-wave *_fuseD"""
    assert R.fused_nt(R.N_NT_LAST, True) and not R.fused_nt(R.N_BUF_FIRST, True) and not R.fused_nt(R.N_W3_FIRST, True)
    assert not R.fused_nt(1000, False) and R.fuses(R.N_W3_FIRST, True, False) and not R.fuses(R.N_W3_FIRST, True, True)
    assert R.fused_nt(4_000_000, True) and R.regime(4_000_000, True, False) == R.regime(2_000_000, True, True) == "hbm_nt"
    assert R.regime(1_000_000, True, False) == "w3" and R.regime(100_000, True, False) == "nt" and R.regime(100_000, True, True) == "buf"
