"""The launcher's kernel-choice rule (step_kernel_choice in step_device.inc) restated in Python, and the swarm sizes the GPU tests use
to stand on each side of every threshold of it.  tests/test_step_regimes.py reads the thresholds out of the sources and holds this
restatement and the named sizes against them: a threshold that moves in the source fails there, with the sizes to move.

A step launch takes its kernel from the size of the WHOLE swarm, in blocks of 64 UAVs (LITERAL: always the two-wave `*_buf`):

  family       nt kernels      two-wave *_buf       three-wave *_w3     nt again (HBM streaming)
  model-only   <= 1900 blocks  1901 .. 2048 blocks  > 2048 blocks       npad * 412 B >= 1.4 GB
  cascade      <= 900 blocks   901 .. 2048 blocks   > 2048 blocks       npad * 796 B >= 1.4 GB

and the pointer-addressed kernels once the state array (F_COUNT columns of npad doubles) no longer fits a 32-bit buffer offset.  A
plain run of a model-only swarm (no mixed-airframe blocks, buffer-addressed) is fused: `*_nt_fuseD` where the single step is an nt
kernel, the two-wave `*_fuseD` everywhere else - also where the single step is the three-wave kernel."""

BLOCK = 64
NT_MAX_BLOCKS = 1900           # model-only FAST: *_nt up to here
NT_CASCADE_MAX_BLOCKS = 900    # cascade FAST: *_nt up to here
W3_ABOVE_BLOCKS = 2 * 1024     # FAST: three-wave kernels above
HBM_BYTES = 1.4e9              # FAST: moved bytes per step from which the nt kernels stream again
BYTES_MODEL, BYTES_CASCADE = 412.0, 796.0  # moved bytes per UAV-step
F_COUNT = 86                   # state columns (swarm_layout.h): buffer addressing while F_COUNT * npad * 8 < 2^32
SPLIT_MIN_BLOCKS = 1024        # tick_single.hip: a run takes the two-stream form from this many blocks on ...
SPLIT_MIN_LAUNCHES = 4         # ... when it is at least this many launches

REGIMES = ("nt", "buf", "w3", "hbm_nt", "pointer")


def blocks(n):
    return (n + BLOCK - 1) // BLOCK


def regime(n, fast, cascade):
    """the member of the step family a single-step launch of a swarm of n UAVs takes (no tuning aid set)"""
    nb = blocks(n)
    npad = max(nb, 1) * BLOCK
    if F_COUNT * npad * 8 >= 1 << 32:
        return "pointer"
    if not fast:
        return "buf"
    if npad * (BYTES_CASCADE if cascade else BYTES_MODEL) >= HBM_BYTES:
        return "hbm_nt"
    if nb > W3_ABOVE_BLOCKS:
        return "w3"
    return "nt" if nb <= (NT_CASCADE_MAX_BLOCKS if cascade else NT_MAX_BLOCKS) else "buf"


def fuses(n, fast, cascade):
    """a plain step_n(dt, K, 1) of such a swarm (one airframe type per block) is issued as fused launches"""
    return not cascade and regime(n, fast, cascade) != "pointer"


def fused_nt(n, fast):
    """the fused launches of a model-only swarm are the *_nt_fuseD kernels (else the two-wave *_fuseD)"""
    return regime(n, fast, False) in ("nt", "hbm_nt")


def two_streams(n, launches):
    return blocks(n) >= SPLIT_MIN_BLOCKS and launches >= SPLIT_MIN_LAUNCHES


# ---- the named sizes of the GPU tests: one on each side of every threshold ----------------------------------------------------
N_NT_LAST = NT_MAX_BLOCKS * BLOCK                  # 121 600 UAVs, 1900 blocks: the last model-only size on the nt kernels
N_BUF_FIRST = N_NT_LAST + 1                        # 121 601 UAVs, 1901 blocks (a one-lane tail block): the first on *_buf
N_BUF_LAST = W3_ABOVE_BLOCKS * BLOCK               # 131 072 UAVs, 2048 full blocks: the last on the two-wave *_buf
N_W3_FIRST = N_BUF_LAST + 1                        # 131 073 UAVs, 2049 blocks (a one-lane tail block): the first on *_w3
N_CASCADE_NT_LAST = NT_CASCADE_MAX_BLOCKS * BLOCK  # 57 600 UAVs, 900 blocks: the last cascade size on the nt kernel
N_CASCADE_BUF_FIRST = N_CASCADE_NT_LAST + 1        # 57 601 UAVs, 901 blocks: the first cascade size on *_buf
N_ONE_STREAM_LAST = (SPLIT_MIN_BLOCKS - 1) * BLOCK  # 65 472 UAVs, 1023 blocks: runs stay on one stream
N_TWO_STREAMS_FIRST = N_ONE_STREAM_LAST + 1        # 65 473 UAVs, 1024 blocks: runs of four or more launches take two streams

# (name, n, cascade) -> what FAST launches there; LITERAL launches "buf" at every one of them
NAMED = {
    "N_NT_LAST": (N_NT_LAST, False, "nt"),
    "N_BUF_FIRST": (N_BUF_FIRST, False, "buf"),
    "N_BUF_LAST": (N_BUF_LAST, False, "buf"),
    "N_W3_FIRST": (N_W3_FIRST, False, "w3"),
    "N_CASCADE_NT_LAST": (N_CASCADE_NT_LAST, True, "nt"),
    "N_CASCADE_BUF_FIRST": (N_CASCADE_BUF_FIRST, True, "buf"),
    "N_BUF_LAST (cascade)": (N_BUF_LAST, True, "buf"),
    "N_W3_FIRST (cascade)": (N_W3_FIRST, True, "w3"),
}
