"""torch tensors in and out of a Swarm without the host: commands, observations, rollouts, nearest-neighbour observations, masked resets,
crash flags and state snapshots for a controller, policy or reward that lives on the swarm's GPU (include/mrs_swarm.h, "device-resident callers").

Every call passes torch's current stream of the swarm's device as the caller stream: the library fences its own stream against it, so
tensors written on that stream before the call are what the kernel reads, and work queued after the call sees the result.  Tensors are
checked (check_tensor) before any library call: CPU tensors, tensors of another device, rows whose last dimension is not contiguous and
wrong dtypes or shapes are refused with a ValueError.  Row k of every tensor belongs to UAV first + k.

Imports torch; the package itself does not.
"""
import collections

import torch

from .swarm import (ACTUATOR_CMD, ATTITUDE_CMD, DTYPE_F32, DTYPE_F64, INPUT_UNKNOWN, MAX_MOTORS, NN_ALL, NN_DIST, NN_MAX_K,  # noqa: F401
                    NN_REL_POS, NN_REL_POS_BODY, NN_REL_VEL, NN_REL_VEL_BODY, OBS_ALL, OBS_IMU, OBS_OMEGA, OBS_POS, OBS_QUAT, OBS_ROT,
                    OBS_RPM, OBS_VEL, OBS_VEL_BODY, PROX_COUNT, PROX_HINGE2, PROX_INVERSE, SNAP_BAD_AIRFRAME, SNAP_BAD_INDEX, SNAP_BAD_MAGIC, SNAP_CRASHED, SNAP_LOADED,
                    SNAP_MAGIC, SNAP_SKIPPED, SNAP_TAKEOFF, SNAP_VPREV_SPLIT, SNAPSHOT_DTYPE, TILT_HDG_RATE_CMD, gather_width, nearest_width,
                    OBST_ALL_WORLDS, OBST_BOX, OBST_CYLINDER, OBST_MAX, OBST_MAX_K, OBST_SPHERE, OBSTACLE_DTYPE, ON_ALL, ON_DIST, ON_REL, ON_REL_BODY,
                    SCAN_BODY_FRAME, SCAN_GROUND, SCAN_HIT_GROUND, SCAN_HIT_NONE, SCAN_MAX_BEAMS, UAVSCAN_HIT_UAV, CONTACT_CRASH, obstacle_width)

_DTYPES = {torch.float64: DTYPE_F64, torch.float32: DTYPE_F32}
SNAP_BYTES = SNAPSHOT_DTYPE.itemsize  # 496: one mrs_uav_snapshot_t


def _check_device(t, name, dtypes, device_index):
    """Refuse `t` unless it is a tensor on cuda:`device_index` whose dtype is one of `dtypes`.  The messages open with `name`; None:
    an unnamed tensor, in check_tensor's wording."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name + ': ' if name else ''}expected a torch.Tensor, got {type(t).__name__}")
    who = name or "tensor"
    if t.device.type != "cuda":
        raise ValueError(f"{who} is on {t.device}: device-resident calls need a tensor on cuda:{device_index}"
                         + ("" if name else " (use the host calls of Swarm for CPU data)"))
    if t.device.index != device_index:
        raise ValueError(f"{who} is on {t.device}, the swarm lives on cuda:{device_index}")
    if t.dtype not in dtypes:
        raise ValueError(f"{who} has dtype {t.dtype}, expected {' or '.join(str(d) for d in dtypes)}")


def check_tensor(t, rows, min_width, dtype, device_index):
    """Refuse `t` unless it is a tensor on cuda:`device_index` of `dtype` with `rows` rows whose last dimension is contiguous.
    min_width None: a vector of `rows` elements; else a [rows, >= min_width] matrix.  Returns the row stride in elements (the
    distance between two rows; the columns past min_width are padding the library does not touch).  Needs no GPU."""
    _check_device(t, None, (dtype,), device_index)
    if min_width is None:
        if t.dim() != 1 or t.shape[0] != rows:
            raise ValueError(f"expected a vector of {rows} elements, got shape {tuple(t.shape)}")
        if rows > 1 and t.stride(0) != 1:
            raise ValueError(f"vector is not contiguous (stride {t.stride(0)})")
        return 1
    if t.dim() != 2 or t.shape[0] != rows or t.shape[1] < min_width:
        raise ValueError(f"expected a [{rows}, >= {min_width}] matrix, got shape {tuple(t.shape)}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"rows are not contiguous: the stride of the last dimension is {t.stride(1)}, must be 1")
    stride = t.stride(0) if rows > 1 else t.shape[1]
    if stride < t.shape[1]:
        raise ValueError(f"rows overlap: row stride {stride} < row width {t.shape[1]}")
    return stride


def _dtype_code(dtype):
    if dtype not in _DTYPES:
        raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype}")
    return _DTYPES[dtype]


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _count(swarm, first, count):
    return swarm.n - first if count is None else int(count)


def command_width(mode, n_cols):
    """payload elements per row of a setInput mode (mrs_swarm_set_input; ACTUATOR: the row's own width, at most MAX_MOTORS)"""
    if mode == INPUT_UNKNOWN:
        return 0
    if mode == ACTUATOR_CMD:
        return min(n_cols, MAX_MOTORS)
    if mode == ATTITUDE_CMD:
        return 10
    if mode == TILT_HDG_RATE_CMD:
        return 5
    return 4


def gather(swarm, groups, first=0, count=None, dtype=torch.float32, out=None):
    """The OBS_* groups of UAVs [first, first + count) as a [count, gather_width(groups)] tensor on the swarm's device (or into `out`, a
    [count, >= width] tensor whose columns past the width are left alone)."""
    count = _count(swarm, first, count)
    width = gather_width(groups)
    dev = swarm.device()
    if out is None:
        out = torch.empty((count, width), dtype=dtype, device=torch.device("cuda", dev))
    code = _dtype_code(out.dtype)
    stride = check_tensor(out, count, width, out.dtype, dev)
    swarm.gather_device(first, count, groups, out.data_ptr(), code, stride, _stream(dev))
    return out[:, :width] if out.shape[1] > width else out


def set_input(swarm, mode, rows, first=0):
    """UavSystem::setInput of `mode` for UAVs [first, first + rows.shape[0]) from a [count, width] FP32 / FP64 tensor (the payload layouts of
    Swarm.set_input).  ACTUATOR rows must be dense: their width is the number of motors given."""
    dev = swarm.device()
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
        raise ValueError("rows must be a [count, width] tensor")
    code = _dtype_code(rows.dtype)
    count = rows.shape[0]
    width = command_width(mode, rows.shape[1])
    stride = check_tensor(rows, count, width, rows.dtype, dev)
    if mode == ACTUATOR_CMD and count > 1 and stride != rows.shape[1]:
        raise ValueError("actuator rows must be dense (row stride == number of motors)")
    ptr = rows.data_ptr() if width > 0 and count > 0 else 0
    swarm.set_input_device(first, count, mode, ptr, code, stride, _stream(dev))


def apply_force(swarm, rows, first=0):
    """UavSystem::applyForce for UAVs [first, first + rows.shape[0]) from a [count, >= 3] FP32 / FP64 tensor: world frame, newtons, latched
    until the next applyForce or evaluated collision tick (mrs_swarm_apply_force_device).  Columns past the third are padding."""
    dev = swarm.device()
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
        raise ValueError("rows must be a [count, >= 3] tensor")
    code = _dtype_code(rows.dtype)
    count = rows.shape[0]
    stride = check_tensor(rows, count, 3, rows.dtype, dev)
    swarm.apply_force_device(first, count, rows.data_ptr() if count > 0 else 0, code, stride, _stream(dev))


def _check_steps(t, name, steps, rows, min_width, dtype, device_index):
    """Refuse `t` unless it is a [steps, rows, >= min_width] tensor on cuda:`device_index` of `dtype` (steps None: any number >= 1) whose
    rows are contiguous and whose row blocks follow each other densely: stride(0) == rows * stride(1).  Returns the row stride."""
    _check_device(t, name, (dtype,), device_index)
    if t.dim() != 3 or t.shape[0] < 1 or (steps is not None and t.shape[0] != steps) or t.shape[1] != rows or t.shape[2] < min_width:
        raise ValueError(f"{name}: expected a [{'T' if steps is None else steps}, {rows}, >= {min_width}] tensor, got shape {tuple(t.shape)}")
    if t.shape[2] > 1 and t.stride(2) != 1:
        raise ValueError(f"{name}: rows are not contiguous: the stride of the last dimension is {t.stride(2)}, must be 1")
    stride = t.stride(1) if rows > 1 else t.shape[2]
    if stride < t.shape[2]:
        raise ValueError(f"{name}: rows overlap: row stride {stride} < row width {t.shape[2]}")
    if t.shape[0] > 1 and t.stride(0) != rows * stride:
        raise ValueError(f"{name}: the step dimension is not dense (stride(0) = {t.stride(0)}, expected {rows} x {stride})")
    return stride


def _check_crash_rows(t, blocks, rows, device_index):
    """Refuse `t` unless it is a dense [blocks, rows] torch.bool / torch.uint8 tensor on cuda:`device_index` (block j at byte j * rows)."""
    _check_device(t, "crashed", (torch.bool, torch.uint8), device_index)
    if t.dim() != 2 or t.shape[0] != blocks or t.shape[1] != rows:
        raise ValueError(f"crashed: expected a [{blocks}, {rows}] tensor, got shape {tuple(t.shape)}")
    if (rows > 1 and t.stride(1) != 1) or (blocks > 1 and t.stride(0) != rows):
        raise ValueError(f"crashed: the crash rows are not dense (strides {tuple(t.stride())}, expected ({rows}, 1))")


def _row_blocks(t, name, blocks, count, w, dtype, dev):
    """Row blocks that are [blocks, count, >= w] (a row per UAV) or [blocks, 1, w] (one dense row per block for all UAVs), as the targets
    of rollout_cost.  Returns the row stride, 0 for shared rows."""
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[0] != blocks or t.shape[1] not in (1, count) or t.shape[2] < w:
        raise ValueError(f"{name}: expected a [{blocks}, {count} or 1, >= {w}] tensor, got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.shape[1] == 1:  # one row per block: its stride is that of the first dimension
        stride = check_tensor(t[:, 0, :], blocks, w, dtype, dev)
        if count != 1:
            if blocks > 1 and stride != w:
                raise ValueError(f"{name}: shared rows must be dense, [{blocks}, 1, {w}], got a row stride of {stride}")
            return 0
        return stride
    return _check_steps(t, name, blocks, count, w, dtype, dev)


# What the six rollout wrappers share.  Every wrapper is _rollout_head, then the blocks its kind takes (_obs_rows; _feedback;
# _evaluation), then its library call; the blocks raise in the order the wrappers call them, and that order is part of the interface:
# a call with several faults reports the first.
_Head = collections.namedtuple("_Head", "dev dtype code blocks count steps hold every width cstride cptr")


def _rollout_head(swarm, mode, commands, hold, every, every_name, noun, payload=False):
    """The command side of a rollout: commands [B, count, >= width] on the swarm's device, held for `hold` steps each, a report or an
    evaluation after every `every` (the argument `every_name`; default: hold) of the B * hold `noun` ("steps" or "ticks") of the call.
    payload: the mode must have payload elements.  Returns the _Head the blocks and the library call read: the device, the commands'
    dtype and its code, B, count, B * hold, hold and every as ints, the payload width, the command row stride and the command pointer
    (0 when no element would be read)."""
    dev = swarm.device()
    if not isinstance(commands, torch.Tensor) or commands.dim() != 3:
        raise ValueError("commands must be a [T, count, width] tensor")
    hold = int(hold)
    if hold < 1:
        raise ValueError(f"hold must be at least 1, got {hold}")
    code = _dtype_code(commands.dtype)
    blocks, count = commands.shape[0], commands.shape[1]
    steps = blocks * hold
    every = hold if every is None else int(every)
    if every < 1 or steps % every != 0:
        raise ValueError(f"{every_name} must be at least 1 and divide the {steps} {noun} of the call, got {every}")
    width = command_width(mode, commands.shape[2])
    if payload and width < 1:
        raise ValueError("a feedback rollout needs a mode with a payload")
    cstride = _check_steps(commands, "commands", None, count, width, commands.dtype, dev)
    if mode == ACTUATOR_CMD and count > 1 and cstride != commands.shape[2]:
        raise ValueError("actuator rows must be dense (row stride == number of motors)")
    cptr = commands.data_ptr() if width > 0 and count > 0 else 0
    return _Head(dev, commands.dtype, code, blocks, count, steps, hold, every, width, cstride, cptr)


def _obs_rows(h, groups, out):
    """The observation rows of rollout and rollout_ticks: `out` is [steps // every, count, >= gather_width(groups)] of the commands' dtype,
    allocated when None.  Returns (the rows the wrapper returns: `out` without its columns past the width, None when groups == 0; the
    pointer; the row stride)."""
    owidth = gather_width(groups)
    if not groups:
        return None, 0, owidth
    if out is None:
        out = torch.empty((h.steps // h.every, h.count, owidth), dtype=h.dtype, device=torch.device("cuda", h.dev))
    if isinstance(out, torch.Tensor) and out.dtype != h.dtype:
        raise ValueError(f"out has dtype {out.dtype}, the commands {h.dtype}: one dtype serves both")
    ostride = _check_steps(out, "out", h.steps // h.every, h.count, owidth, h.dtype, h.dev)
    return (out[:, :, :owidth] if out.shape[2] > owidth else out), out.data_ptr(), ostride


def _one_dtype(h, **tensors):
    """Refuse a tensor among `tensors` (by argument name; what is no tensor is left to the check of its shape) of another dtype than the
    commands'."""
    for name, t in tensors.items():
        if isinstance(t, torch.Tensor) and t.dtype != h.dtype:
            raise ValueError(f"{name} has dtype {t.dtype}, the commands {h.dtype}: one dtype serves commands, "
                             f"{', '.join(list(tensors)[:-1])} and {list(tensors)[-1]}")


def _cost_vector(out, count, accumulate, dev):
    """The FP64 [count] cost vector of a costed call: `out`, or a new one when None, which accumulate=True refuses"""
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs the `out` vector it adds to")
        out = torch.empty(count, dtype=torch.float64, device=torch.device("cuda", dev))
    if isinstance(out, torch.Tensor) and out.dtype != torch.float64:
        raise ValueError(f"out has dtype {out.dtype}: the cost vector is always torch.float64")
    check_tensor(out, count, None, torch.float64, dev)
    return out


def _evaluation(h, groups, targets, weights, out, accumulate, alone, refusal):
    """The cost side of the four costed wrappers.  With E = steps // every evaluations and w = gather_width(groups): targets is
    [E, count or 1, >= w] (_row_blocks), weights [E or 1, >= w], both of the commands' dtype, and `out` the cost vector (_cost_vector).
    Returns (out, (target pointer, target stride, weight pointer, weight stride), cost pointer).
    groups == 0 leaves no column to compare and takes no targets and no weights.  What it means is the wrapper's, told by `alone`;
    `refusal` is the message of a call that does not fit it:
      None       nothing: refused (rollout_cost);
      "crash"    the crash cost alone, with `out` as ever (rollout_tick_cost);
      "nothing"  a run without a cost: `out` stays None and accumulate false, and None is returned (rollout_feedback);
      "either"   the crash cost alone into a given `out`, a run without a cost without one: `out` is never allocated, and accumulate
                 needs it (rollout_tick_feedback)."""
    w, evals = gather_width(groups), h.steps // h.every
    rows = (0, 0, 0, 0)
    if w == 0:
        if alone is None or targets is not None or weights is not None or (alone == "nothing" and (out is not None or accumulate)):
            raise ValueError(refusal)
        if alone != "crash" and out is None and not accumulate:
            return None, rows, 0
    else:
        _one_dtype(h, targets=targets, weights=weights)  # (nothing left to refuse behind _feedback, which compares these two as well)
        tstride = _row_blocks(targets, "targets", evals, h.count, w, h.dtype, h.dev)
        if not isinstance(weights, torch.Tensor) or weights.dim() != 2 or weights.shape[0] not in (1, evals):
            raise ValueError(f"weights: expected a [{evals} or 1, >= {w}] tensor, got "
                             f"{tuple(weights.shape) if isinstance(weights, torch.Tensor) else type(weights).__name__}")
        wstride = check_tensor(weights, weights.shape[0], w, h.dtype, h.dev)
        rows = (targets.data_ptr(), tstride, weights.data_ptr(), 0 if weights.shape[0] == 1 else wstride)
    out = _cost_vector(out, h.count, accumulate, h.dev)
    return out, rows, out.data_ptr()


def _feedback(h, fb_groups, gains, refs, targets, weights):
    """The feedback side of the two feedback wrappers: gains [Bg, W_c, W_o] or [Bg, W_c, W_o, count], dense, and refs
    [Bg, count or 1, >= W_o] (_row_blocks), Bg in {1, B}, W_o = gather_width(fb_groups) >= 1; one dtype for them, the commands and the
    cost side's tensors.  Returns (gain pointer, gain_per_uav, gain blocks, ref pointer, ref stride, ref blocks), as the library takes them."""
    wo = gather_width(fb_groups)
    if wo == 0:
        raise ValueError("fb_groups must select at least one observation group: a feedback needs columns")
    _one_dtype(h, gains=gains, refs=refs, targets=targets, weights=weights)
    if not isinstance(gains, torch.Tensor) or gains.dim() not in (3, 4):
        raise ValueError(f"gains: expected a [Bg, {h.width}, {wo}] (shared) or [Bg, {h.width}, {wo}, {h.count}] (per UAV, UAV-minor) tensor, got "
                         f"{tuple(gains.shape) if isinstance(gains, torch.Tensor) else type(gains).__name__}")
    per_uav = gains.dim() == 4
    want = (h.width, wo, h.count) if per_uav else (h.width, wo)
    if gains.shape[0] not in (1, h.blocks) or tuple(gains.shape[1:]) != want:
        raise ValueError(f"gains: expected a [{h.blocks} or 1, {', '.join(str(x) for x in want)}] tensor, got {tuple(gains.shape)}")
    if gains.device.type != "cuda" or gains.device.index != h.dev:
        raise ValueError(f"gains is on {gains.device}, the swarm lives on cuda:{h.dev}")
    if not gains.is_contiguous():
        raise ValueError("gains must be dense" + (": [Bg, W_c, W_o, count] with the UAV index last (g.permute(0, 2, 3, 1).contiguous())"
                                                  if per_uav else ": [Bg, W_c, W_o], row-major"))
    if not isinstance(refs, torch.Tensor) or refs.dim() != 3 or refs.shape[0] not in (1, h.blocks):
        raise ValueError(f"refs: expected a [{h.blocks} or 1, {h.count} or 1, >= {wo}] tensor, got "
                         f"{tuple(refs.shape) if isinstance(refs, torch.Tensor) else type(refs).__name__}")
    rstride = _row_blocks(refs, "refs", refs.shape[0], h.count, wo, h.dtype, h.dev)
    return gains.data_ptr(), int(per_uav), gains.shape[0], refs.data_ptr(), rstride, refs.shape[0]


def rollout(swarm, mode, commands, dt, groups=OBS_POS | OBS_VEL | OBS_QUAT, first=0, out=None, hold=1, obs_every=None, forces=None,
            force_hold=None):
    """B * hold steps of the whole swarm in which UAVs [first, first + count) take command row block j before step j * hold, keep it for
    `hold` steps (setInput latches), and report the OBS_* groups of `groups` after every `obs_every` steps (default: `hold`, a row block
    per command; B * hold: the final state only).  With hold == 1 (mrs_swarm_rollout_device): `for t: set_input(swarm, mode,
    commands[t], first); swarm.step_n(dt, 1); gather(swarm, groups, first, count, out=out[t])`, bit for bit in LITERAL, in one call;
    with obs_every == hold (mrs_swarm_rollout_rate_device): `for j: set_input(commands[j]); swarm.step_n(dt, hold); gather(out=out[j])`.
    commands: [B, count, >= width] FP32 / FP64 (the payload layouts of set_input; ACTUATOR rows are dense).  obs_every must be >= 1 and
    divide B * hold.  out: [B * hold // obs_every, count, >= gather_width(groups)] of the same dtype, allocated when None; returned
    (None when groups == 0).  UAVs outside the range are stepped with their own commands.
    forces: [Bf, count, >= 3] of the commands' dtype: UAVs of the range take force row block j (applyForce: world frame, newtons) before
    step j * force_hold and keep it for `force_hold` steps (default: B * hold // Bf; it must be >= 1 and Bf * force_hold == B * hold) —
    the loop above with `apply_force(swarm, forces[j], first)` in it, in one call (mrs_swarm_rollout_force_device).  Afterwards the range
    carries the last force block."""
    h = _rollout_head(swarm, mode, commands, hold, obs_every, "obs_every", "steps")
    if forces is not None:
        fstride = _check_steps(forces, "forces", None, h.count, 3, h.dtype, h.dev)
        fhold = h.steps // forces.shape[0] if force_hold is None else int(force_hold)
        if fhold < 1 or forces.shape[0] * fhold != h.steps:
            raise ValueError(f"force_hold must be at least 1 and {forces.shape[0]} force blocks x force_hold must be the {h.steps} steps of "
                             f"the call, got {fhold}")
    rows, optr, ostride = _obs_rows(h, groups, out)
    if forces is not None:
        swarm.rollout_force_device(first, h.count, mode, dt, h.steps, h.hold, h.every, fhold, h.cptr, h.code, h.cstride, forces.data_ptr(),
                                   fstride, groups, optr, ostride, _stream(h.dev))
    elif h.hold == 1 and h.every == 1:
        swarm.rollout_device(first, h.count, mode, dt, h.steps, h.cptr, h.code, h.cstride, groups, optr, ostride, _stream(h.dev))
    else:
        swarm.rollout_rate_device(first, h.count, mode, dt, h.steps, h.hold, h.every, h.cptr, h.code, h.cstride, groups, optr, ostride,
                                  _stream(h.dev))
    return rows


def rollout_cost(swarm, mode, commands, dt, groups, targets, weights, first=0, hold=1, cost_every=None, out=None, accumulate=False):
    """rollout(hold=hold, obs_every=cost_every) that returns one FP64 number per UAV instead of row blocks: after every `cost_every` steps
    (default: `hold`; B * hold: a terminal cost) the FP64 observation row of `groups` of UAV first + k is compared with its target row, and
    `sum over columns of (weight * d) * d`, d = row - target, is added to the UAV's cost (mrs_swarm_rollout_cost_device; the arithmetic is
    FP64, unfused, columns ascending, evaluations in order, in both flavours).  commands: as in rollout.  With E = B * hold // cost_every
    evaluations and w = gather_width(groups): targets is [E, count, >= w] (a row per UAV) or [E, 1, w] (one dense row per evaluation for
    all UAVs); weights is [E, >= w] (a row per evaluation: a heavier last row is a terminal cost) or [1, >= w]; both of the commands'
    dtype.  out: a float64 [count] vector, allocated when None; accumulate=True adds to what `out` holds (two calls over the halves of a
    horizon give the bits of one call), else it is overwritten.  Returns out.  No observation row is written."""
    h = _rollout_head(swarm, mode, commands, hold, cost_every, "cost_every", "steps")
    out, rows, optr = _evaluation(h, groups, targets, weights, out, accumulate, None,
                                  "groups must select at least one observation group: a cost needs columns")
    swarm.rollout_cost_device(first, h.count, mode, dt, h.steps, h.hold, h.every, h.cptr, h.code, h.cstride, groups, *rows, optr,
                              bool(accumulate), _stream(h.dev))
    return out


def rollout_ticks(swarm, mode, commands, dt, crash, rebounce, groups=OBS_POS | OBS_VEL | OBS_QUAT, first=0, out=None, hold=1, obs_every=None,
                  crashed=None):
    """B * hold ticks of the whole swarm in one call (mrs_swarm_rollout_tick_device): each tick is a step of every UAV, then the
    collision pass `swarm.handle_collisions(True, crash, rebounce)`.  UAVs [first, first + count) take command row block j before tick
    j * hold and keep it for `hold` ticks; after every `obs_every` ticks (default: `hold`) the OBS_* groups of `groups` and the crash
    flags of the range are reported, taken after the tick's step and before its collision pass.  It is the loop `for t: set_input(...);
    swarm.tick_n(dt, 1, True, crash, rebounce); gather(...); crashed(...)` with the rows taken between the step and the collision pass,
    bit for bit in LITERAL, with one host wait per call.
    commands, out: as in rollout.  crashed: a dense torch.bool or torch.uint8 [B * hold // obs_every, count] tensor, allocated (bool) when
    None; crashed=False asks for no crash rows.  Returns (rows or None when groups == 0, crashed or None).  The collision pass of the last
    tick stays pending: the next step or tick evaluates it."""
    h = _rollout_head(swarm, mode, commands, hold, obs_every, "obs_every", "ticks")
    rows, optr, ostride = _obs_rows(h, groups, out)
    kptr = 0
    if crashed is False:
        crashed = None
    else:
        if crashed is None:
            crashed = torch.empty((h.steps // h.every, h.count), dtype=torch.bool, device=torch.device("cuda", h.dev))
        _check_crash_rows(crashed, h.steps // h.every, h.count, h.dev)
        kptr = crashed.data_ptr()
    swarm.rollout_tick_device(first, h.count, mode, dt, h.steps, h.hold, h.every, h.cptr, h.code, h.cstride, groups, optr, ostride, kptr,
                              bool(crash), float(rebounce), _stream(h.dev))
    return rows, crashed


def rollout_tick_cost(swarm, mode, commands, dt, crash, rebounce, groups, targets, weights, crash_cost=0.0, first=0, hold=1, cost_every=None,
                      out=None, accumulate=False):
    """rollout_ticks(hold=hold, obs_every=cost_every) that returns one FP64 number per UAV instead of row blocks
    (mrs_swarm_rollout_tick_cost_device): after every `cost_every` ticks (default: `hold`), between the tick's step and its collision
    pass, the term of rollout_cost (the FP64 row of `groups` against its target row under the weight row) is added to the UAV's cost,
    and then `crash_cost` if the UAV has crashed — two separately rounded FP64 additions, in that order.  The crash flag is a level: a
    UAV that crashed early pays at every later evaluation; a crash caused by the last tick's collision pass stays pending with it and is
    charged by the next horizon.  commands, targets, weights, out, accumulate: as in rollout_cost.  groups == 0 (then targets and
    weights stay None) is the crash cost alone.  Returns out.  No observation row and no crash byte is written; the collision pass of
    the last tick stays pending."""
    h = _rollout_head(swarm, mode, commands, hold, cost_every, "cost_every", "ticks")
    out, rows, optr = _evaluation(h, groups, targets, weights, out, accumulate, "crash",
                                  "groups == 0 is the crash cost alone: it takes no targets and no weights")
    swarm.rollout_tick_cost_device(first, h.count, mode, dt, h.steps, h.hold, h.every, h.cptr, h.code, h.cstride, groups, *rows,
                                   float(crash_cost), optr, bool(accumulate), bool(crash), float(rebounce), _stream(h.dev))
    return out


def rollout_feedback(swarm, mode, commands, dt, fb_groups, gains, refs, cost_groups=0, targets=None, weights=None, first=0, hold=1,
                     cost_every=None, out=None, accumulate=False):
    """rollout_cost whose commands are NOMINAL commands: at the start of command block b (every `hold` steps) the command of UAV
    first + k is formed in the step kernel as `commands[b, k] + G[b, k] @ (refs[b, k] - o)`, o being the FP64 observation row of
    `fb_groups` before the step (what gather(fb_groups, float64) would return), and held for the block
    (mrs_swarm_rollout_feedback_device: FP64, unfused, e[j] = ref[j] - o[j], then per payload element c the sum over ascending j of
    G[c][j] * e[j] added to the nominal command, in both flavours).  The call is the loop gather -> that arithmetic -> set_input ->
    `hold` steps, bit for bit, without a launch or a host round trip per tick; the feedback has no memory, so a horizon cut into calls
    (accumulate=True from the second on) gives the bits of one call.
    With B = commands.shape[0], W_c = command_width(mode) and W_o = gather_width(fb_groups) >= 1, Bg in {1, B} (one block for the whole
    call, or one per command block):
      refs   [Bg, count, >= W_o] (a setpoint row per UAV) or [Bg, 1, W_o] (one dense row per block for all UAVs);
      gains  3-D [Bg, W_c, W_o], dense: one gain matrix for all UAVs; or
             4-D [Bg, W_c, W_o, count], dense, UAV-MINOR: a gain matrix per UAV.  A UAV's gain is W_c * W_o numbers (4 x 18 doubles are
             576 B, more than a step moves); with the UAV index last each of the W_c * W_o loads of a 64-lane wave is one coalesced
             request, where a matrix per row would touch 64 cache lines per load.  From a [Bg, count, W_c, W_o] tensor:
             `g.permute(0, 2, 3, 1).contiguous()`.
    One dtype serves commands, gains, refs, targets and weights.  cost_groups, targets, weights, cost_every, out, accumulate: as in
    rollout_cost; cost_groups == 0 (then targets, weights and out stay None) is a pure closed-loop run and returns None."""
    h = _rollout_head(swarm, mode, commands, hold, cost_every, "cost_every", "steps", payload=True)
    fb = _feedback(h, fb_groups, gains, refs, targets, weights)
    out, rows, optr = _evaluation(h, cost_groups, targets, weights, out, accumulate, "nothing",
                                  "cost_groups == 0 is a run without a cost: targets, weights and out must stay None")
    swarm.rollout_feedback_device(first, h.count, mode, dt, h.steps, h.hold, h.every, h.cptr, h.code, h.cstride, fb_groups, *fb, cost_groups,
                                  *rows, optr, bool(accumulate), _stream(h.dev))
    return out


def rollout_tick_feedback(swarm, mode, commands, dt, crash, rebounce, fb_groups, gains, refs, cost_groups=0, targets=None, weights=None,
                          crash_cost=0.0, first=0, hold=1, cost_every=None, out=None, accumulate=False):
    """rollout_tick_cost whose commands are NOMINAL commands, as rollout_feedback's are (mrs_swarm_rollout_tick_feedback_device): at the
    start of command block b (every `hold` ticks) the command of UAV first + k is formed in the fused step + collision kernel as
    `commands[b, k] + G[b, k] @ (refs[b, k] - o)`, o being the FP64 observation row of `fb_groups` before the step, and held for the
    block; every `cost_every` ticks (default: `hold`), between the tick's step and its collision pass, the evaluation of
    rollout_tick_cost is added to the UAV's cost.  The call is the loop gather -> the feedback law -> set_input -> tick, bit for bit,
    with one host wait and one stream fence per call instead of one per command block; the feedback has no memory, so a horizon cut
    into calls (accumulate=True from the second on) gives the bits of one call.  gains, refs: as in rollout_feedback.  cost_groups,
    targets, weights, crash_cost, out, accumulate: as in rollout_tick_cost, except that `out` is not allocated when cost_groups == 0:
      cost_groups != 0                 the term and the crash cost (out is allocated if None);
      cost_groups == 0 with an `out`   the crash cost alone (targets and weights stay None);
      cost_groups == 0, out None       a pure closed-loop run with no evaluation at all: returns None.
    Returns out.  The collision pass of the last tick stays pending."""
    h = _rollout_head(swarm, mode, commands, hold, cost_every, "cost_every", "ticks", payload=True)
    fb = _feedback(h, fb_groups, gains, refs, targets, weights)
    out, rows, optr = _evaluation(h, cost_groups, targets, weights, out, accumulate, "either",
                                  "cost_groups == 0 is the crash cost alone (with an `out`) or a run without a cost: it takes no targets and no "
                                  "weights")
    swarm.rollout_tick_feedback_device(first, h.count, mode, dt, h.steps, h.hold, h.every, h.cptr, h.code, h.cstride, fb_groups, *fb,
                                       cost_groups, *rows, float(crash_cost), optr, bool(accumulate), bool(crash), float(rebounce),
                                       _stream(h.dev))
    return out


def crashed(swarm, first=0, count=None, out=None):
    """UavSystem::hasCrashed of UAVs [first, first + count) as a bool tensor on the swarm's device"""
    count = _count(swarm, first, count)
    dev = swarm.device()
    if out is None:
        out = torch.empty(count, dtype=torch.bool, device=torch.device("cuda", dev))
    check_tensor(out, count, None, torch.bool, dev)
    swarm.get_crashed_device(first, count, out.data_ptr(), _stream(dev))
    return out


def reset(swarm, mask, pos, heading=None, takeoff=True, first=0):
    """UavSystem(params, pos[k], heading[k]) again, on the device, for every UAV first + k with mask[k] set (mask: bool or uint8 vector of
    count elements; pos: [count, 3], heading: [count] or None, both FP32 or FP64, read for masked rows only).  Commands, feed-forwards,
    mode, airframe and hold flag are kept (mrs_swarm_reset_device)."""
    dev = swarm.device()
    if not isinstance(mask, torch.Tensor):
        raise ValueError("mask must be a tensor")
    count = mask.shape[0] if mask.dim() >= 1 else -1
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"mask has dtype {mask.dtype}, expected torch.bool or torch.uint8")
    check_tensor(mask, count, None, mask.dtype, dev)
    if not isinstance(pos, torch.Tensor):
        raise ValueError("pos must be a tensor")
    code = _dtype_code(pos.dtype)
    if check_tensor(pos, count, 3, pos.dtype, dev) != 3 and count > 1:
        raise ValueError("pos rows must be dense [count, 3]")
    if pos.shape[1] != 3:
        raise ValueError(f"pos must be [count, 3], got shape {tuple(pos.shape)}")
    hptr = 0
    if heading is not None:
        check_tensor(heading, count, None, pos.dtype, dev)
        hptr = heading.data_ptr()
    swarm.reset_device(first, count, mask.data_ptr(), pos.data_ptr(), hptr, code, takeoff, _stream(dev))


def nearest(swarm, k, radius, fields=NN_REL_POS | NN_DIST, first=0, count=None, dtype=torch.float32, out=None, index=None, counts=None):
    """The k nearest other UAVs within `radius` of each UAV of [first, first + count), nearest first, ties to the lower index
    (mrs_swarm_nearest_device).  Returns (rows, index, counts) on the swarm's device: rows [count, k * w] of `dtype` holding k slots of
    the NN_* fields of `fields` in bit order (w = nearest_width(fields, 1); None when fields == 0), index int32 [count, k] (-1: empty
    slot, whose fields are 0) and counts int32 [count] (neighbours listed).  `out` ([count, >= k * w]), `index` ([count, >= k]) and
    `counts` ([count]) are used instead of new tensors when given; columns past the widths are left alone."""
    count = _count(swarm, first, count)
    width = nearest_width(fields, k)
    dev = swarm.device()
    tdev = torch.device("cuda", dev)
    code, stride, rows_ptr = DTYPE_F32, 0, 0
    if fields:
        if out is None:
            out = torch.empty((count, width), dtype=dtype, device=tdev)
        code = _dtype_code(out.dtype)
        stride = check_tensor(out, count, width, out.dtype, dev)
        rows_ptr = out.data_ptr()
    if index is None:
        index = torch.empty((count, k), dtype=torch.int32, device=tdev)
    istride = check_tensor(index, count, k, torch.int32, dev)
    if counts is None:
        counts = torch.empty(count, dtype=torch.int32, device=tdev)
    check_tensor(counts, count, None, torch.int32, dev)
    swarm.nearest_device(first, count, k, radius, fields, rows_ptr, code, stride, index.data_ptr(), istride, counts.data_ptr(), _stream(dev))
    rows = None
    if fields:
        rows = out[:, :width] if out.shape[1] > width else out
    return rows, (index[:, :k] if index.shape[1] > k else index), counts


def proximity_cost(swarm, radius, k=8, kind=PROX_HINGE2, weight=1.0, eps=0.0, first=0, count=None, out=None, accumulate=False, found=False):
    """A separation penalty over the k nearest other UAVs within `radius` of each UAV of [first, first + count), one FP64 number per UAV
    (mrs_swarm_proximity_cost_device): the neighbours of nearest(), nearest first, summed as weight * (radius - d)^2 (PROX_HINGE2),
    weight / (d2 + eps) (PROX_INVERSE) or weight (PROX_COUNT) per listed neighbour.  `out` is a dense torch.float64 [count] vector on
    the swarm's device (a new one when None); accumulate=True adds the term to what `out` holds (the vector of the cost rollouts) and
    needs it.  found: False, True (a new int32 [count] vector) or an int32 [count] vector: the number of neighbours within the radius,
    not capped by k.  Returns (out, found or None).  No simulation state is written; a pending collision tick stays pending."""
    count = _count(swarm, first, count)
    dev = swarm.device()
    out = _cost_vector(out, count, accumulate, dev)
    fptr = 0
    if found is True:
        found = torch.empty(count, dtype=torch.int32, device=torch.device("cuda", dev))
    if found is False or found is None:
        found = None
    else:
        check_tensor(found, count, None, torch.int32, dev)
        fptr = found.data_ptr()
    swarm.proximity_cost_device(first, count, k, radius, kind, weight, eps, out.data_ptr(), bool(accumulate), fptr, _stream(dev))
    return out, found


def _host_array(a, name, dtype, shape):
    """`a` (a tensor of any device, or anything numpy takes) as a host array of `dtype` and `shape` (-1: the obstacle count)"""
    import numpy as np
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.ndim != len(shape) or any(s != -1 and a.shape[d] != s for d, s in enumerate(shape)):
        raise ValueError(f"{name} must have shape [{', '.join('M' if s == -1 else str(s) for s in shape)}], got {tuple(a.shape)}")
    if a.dtype.kind not in "biuf":
        raise ValueError(f"{name} has dtype {a.dtype}, expected numbers")
    return a.astype(dtype)


def set_obstacles(swarm, kinds, centres, sizes, worlds=None, all_worlds=None):
    """Replaces the swarm's static obstacle set (mrs_swarm_set_obstacles): M obstacles of kinds [M] (OBST_SPHERE: radius sizes[:, 0];
    OBST_BOX: axis-aligned, half-extents sizes; OBST_CYLINDER: vertical, radius sizes[:, 0], half-height sizes[:, 2], inf: a pillar
    without ends) at centres [M, 3]; sizes is [M, 3].  worlds [M] (default 0): the world label whose UAVs see the obstacle; all_worlds
    [M] bool (default False): seen by the UAVs of every label.  Tensors (of any device) or arrays: the set is static and travels through
    the host.  M = 0 clears the set.  Obstacles are seen by the queries and scans only: UAVs fly through them unless obstacle_contacts(crash=True) marks them."""
    import numpy as np
    kinds = _host_array(kinds, "kinds", np.int32, (-1,))
    m = len(kinds)
    rec = np.zeros(m, OBSTACLE_DTYPE)
    rec["kind"] = kinds
    rec["c"] = _host_array(centres, "centres", np.float64, (m, 3))
    rec["h"] = _host_array(sizes, "sizes", np.float64, (m, 3))
    if worlds is not None:
        rec["world"] = _host_array(worlds, "worlds", np.int32, (m,))
    if all_worlds is not None:
        rec["flags"] = np.where(_host_array(all_worlds, "all_worlds", np.bool_, (m,)), OBST_ALL_WORLDS, 0)
    if m > OBST_MAX:
        raise ValueError(f"{m} obstacles: at most {OBST_MAX}")
    if not np.isin(rec["kind"], (OBST_SPHERE, OBST_BOX, OBST_CYLINDER)).all():
        raise ValueError("kinds must be OBST_SPHERE, OBST_BOX or OBST_CYLINDER")
    if not np.isfinite(rec["c"]).all():
        raise ValueError("centres must be finite")
    used = np.stack([np.ones(m, bool), rec["kind"] == OBST_BOX, rec["kind"] != OBST_SPHERE], axis=1)
    pillar = np.zeros((m, 3), bool)
    pillar[:, 2] = (rec["kind"] == OBST_CYLINDER) & (rec["h"][:, 2] == np.inf)
    with np.errstate(invalid="ignore"):
        if (used & ~pillar & ~(np.isfinite(rec["h"]) & (rec["h"] >= 0))).any():
            raise ValueError("sizes must be finite and >= 0 (a cylinder's half-height may be inf)")
    swarm.set_obstacles(rec)


def nearest_obstacles(swarm, k, radius, fields=ON_REL | ON_DIST, first=0, count=None, dtype=torch.float32, out=None, index=None, counts=None):
    """The k nearest static obstacles within `radius` (signed distance to the solid) of each UAV of [first, first + count), nearest first,
    ties to the lower obstacle index (mrs_swarm_nearest_obstacles_device).  Returns (rows, index, counts) shaped like nearest()'s: rows
    [count, k * w] of `dtype` holding k slots of the ON_* fields of `fields` in bit order (w = obstacle_width(fields, 1); None when
    fields == 0), index int32 [count, k] (obstacle indices; -1: empty slot, whose fields are 0) and counts int32 [count].  `out`, `index`
    and `counts` are used instead of new tensors when given; columns past the widths are left alone."""
    count = _count(swarm, first, count)
    width = obstacle_width(fields, k)
    dev = swarm.device()
    tdev = torch.device("cuda", dev)
    code, stride, rows_ptr = DTYPE_F32, 0, 0
    if fields:
        if out is None:
            out = torch.empty((count, width), dtype=dtype, device=tdev)
        code = _dtype_code(out.dtype)
        stride = check_tensor(out, count, width, out.dtype, dev)
        rows_ptr = out.data_ptr()
    if index is None:
        index = torch.empty((count, k), dtype=torch.int32, device=tdev)
    istride = check_tensor(index, count, k, torch.int32, dev)
    if counts is None:
        counts = torch.empty(count, dtype=torch.int32, device=tdev)
    check_tensor(counts, count, None, torch.int32, dev)
    swarm.nearest_obstacles_device(first, count, k, radius, fields, rows_ptr, code, stride, index.data_ptr(), istride, counts.data_ptr(),
                                   _stream(dev))
    rows = None
    if fields:
        rows = out[:, :width] if out.shape[1] > width else out
    return rows, (index[:, :k] if index.shape[1] > k else index), counts


def obstacle_cost(swarm, radius, k=8, kind=PROX_HINGE2, weight=1.0, first=0, count=None, out=None, accumulate=False, found=False):
    """A penalty over the k nearest static obstacles within `radius` of each UAV of [first, first + count), one FP64 number per UAV
    (mrs_swarm_obstacle_cost_device): the obstacles of nearest_obstacles(), nearest first, summed as weight * (radius - sd)^2
    (PROX_HINGE2, growing the deeper the UAV is inside) or weight (PROX_COUNT) per listed obstacle; PROX_INVERSE is refused.  out,
    accumulate and found are those of proximity_cost().  Returns (out, found or None).  No simulation state is written; a pending
    collision tick stays pending."""
    if kind == PROX_INVERSE:
        raise ValueError("PROX_INVERSE is not an obstacle cost kind (PROX_HINGE2 or PROX_COUNT)")
    count = _count(swarm, first, count)
    dev = swarm.device()
    out = _cost_vector(out, count, accumulate, dev)
    fptr = 0
    if found is True:
        found = torch.empty(count, dtype=torch.int32, device=torch.device("cuda", dev))
    if found is False or found is None:
        found = None
    else:
        check_tensor(found, count, None, torch.int32, dev)
        fptr = found.data_ptr()
    swarm.obstacle_cost_device(first, count, k, radius, kind, weight, out.data_ptr(), bool(accumulate), fptr, _stream(dev))
    return out, found


def _contact_vector(t, name, count, dtype, dev):
    """an optional [count] output of obstacle_contacts(): (tensor or None, pointer) — True: a new vector of `dtype`; a tensor: checked and
    filled; None or False: none"""
    if t is True:
        t = torch.empty(count, dtype=dtype, device=torch.device("cuda", dev))
    if t is False or t is None:
        return None, 0
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be True, None or a {dtype} [{count}] tensor on the swarm's device, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{name} has dtype {t.dtype}, expected {dtype}")
    check_tensor(t, count, None, dtype, dev)
    return t, t.data_ptr()


def obstacle_contacts(swarm, margin=0.0, crash=False, first=0, count=None, hit=None, index=None, sd=None, counts=None, cost=None, hit_cost=0.0):
    """Which UAVs of [first, first + count) touch a static obstacle (mrs_swarm_obstacle_contacts_device): UAV i touches obstacle j when j
    applies to its world and the signed distance sd_ij < (arm_length + prop_radius) + margin of its airframe, strictly.  Returns
    (hit, index, sd, counts), each a [count] vector on the swarm's device or None: hit uint8 (1: touching), index int32 (the touching
    obstacle of smallest (sd, index), -1: none), sd float64 (that signed distance, inf: none), counts int32 (touching obstacles, not
    capped).  Each takes True (a new vector), a tensor to fill, or None (not computed).  cost: a dense torch.float64 [count] vector,
    cost[k] += hit_cost where UAV first + k touches (the vector of the cost rollouts; other elements are not written).  crash=True marks
    the touching UAVs crashed as Swarm.crash() does — their motors stop at the next step and they fall — after evaluating a pending
    collision tick; with crash=False no simulation state is written and a pending collision tick stays pending.  The test is a snapshot of
    the positions, not a sweep: call it often enough for the speeds and walls at hand."""
    import math
    try:
        margin = float(margin)
    except (TypeError, ValueError):
        raise ValueError(f"margin must be a finite number >= 0, got {margin!r}") from None
    if not (math.isfinite(margin) and margin >= 0):
        raise ValueError(f"margin must be a finite number >= 0, got {margin!r}")
    count = _count(swarm, first, count)
    if first < 0 or count < 0 or first + count > swarm.n:
        raise ValueError(f"UAVs [{first}, {first + count}) do not fit a swarm of {swarm.n} UAVs")
    dev = swarm.device()
    hit, hit_ptr = _contact_vector(hit, "hit", count, torch.uint8, dev)
    index, index_ptr = _contact_vector(index, "index", count, torch.int32, dev)
    sd, sd_ptr = _contact_vector(sd, "sd", count, torch.float64, dev)
    counts, counts_ptr = _contact_vector(counts, "counts", count, torch.int32, dev)
    cost_ptr = 0
    if cost is not None:
        if not isinstance(cost, torch.Tensor):
            raise ValueError(f"cost must be a torch.float64 [{count}] tensor on the swarm's device, got {type(cost).__name__}")
        if cost.dtype != torch.float64:
            raise ValueError(f"cost has dtype {cost.dtype}: the cost vector is always torch.float64")
        check_tensor(cost, count, None, torch.float64, dev)
        hit_cost = float(hit_cost)
        if not math.isfinite(hit_cost):
            raise ValueError(f"hit_cost must be finite, got {hit_cost!r}")
        cost_ptr = cost.data_ptr()
    if not crash and all(t is None for t in (hit, index, sd, counts, cost)):
        raise ValueError("nothing to do: ask for an output (hit, index, sd, counts, cost) or crash=True")
    if count == 0:  # (an empty vector has no address to hand over)
        return hit, index, sd, counts
    swarm.obstacle_contacts_device(first, count, margin, CONTACT_CRASH if crash else 0, hit_ptr, index_ptr, sd_ptr, counts_ptr, cost_ptr,
                                   float(hit_cost) if cost_ptr else 0.0, _stream(dev))
    return hit, index, sd, counts


def nearest_visible(swarm, k, radius, fields=NN_REL_POS | NN_DIST, first=0, count=None, dtype=torch.float32, out=None, index=None, counts=None,
                    visible=True, hidden=True):
    """nearest() for observers that need a line of sight (mrs_swarm_nearest_visible_device): of the other UAVs within `radius` of each UAV
    of [first, first + count), the k nearest that no static obstacle hides (set_obstacles), nearest first, ties to the lower index.  A
    candidate at distance d > 0 in direction u is hidden when an obstacle that applies to the observer's world, within `radius` of the
    observer on every axis, is entered by the beam from the observer along u strictly before d; coincident UAVs always see each other.
    Hidden candidates take no slot: these are the first k visible ones, not the k nearest filtered afterwards.  Returns
    (rows, index, counts, visible, hidden): rows, index and counts as nearest() returns them (counts = min(visible, k)); visible and
    hidden int32 [count], the numbers of visible and of hidden candidates, not capped by k — each takes True (a new vector), a tensor to
    fill, or None (not computed).  `out`, `index`, `counts`: used instead of new tensors when given (index=False / counts=False: not
    computed); columns past the widths are left alone.  Without obstacles the first three are bit for bit those of nearest()."""
    import math
    try:
        radius = float(radius)
    except (TypeError, ValueError):
        raise ValueError(f"radius must be a finite number > 0, got {radius!r}") from None
    if not (math.isfinite(radius) and radius > 0):
        raise ValueError(f"radius must be a finite number > 0, got {radius!r}")
    count = _count(swarm, first, count)
    if first < 0 or count < 0 or first + count > swarm.n:
        raise ValueError(f"UAVs [{first}, {first + count}) do not fit a swarm of {swarm.n} UAVs")
    width = nearest_width(fields, k)
    dev = swarm.device()
    tdev = torch.device("cuda", dev)
    code, stride, rows_ptr = DTYPE_F32, 0, 0
    if fields:
        if out is None:
            out = torch.empty((count, width), dtype=dtype, device=tdev)
        code = _dtype_code(out.dtype)
        stride = check_tensor(out, count, width, out.dtype, dev)
        rows_ptr = out.data_ptr()
    istride, index_ptr = 0, 0
    if index is None:
        index = torch.empty((count, k), dtype=torch.int32, device=tdev)
    if index is False:
        index = None
    else:
        istride = check_tensor(index, count, k, torch.int32, dev)
        index_ptr = index.data_ptr()
    counts, counts_ptr = _contact_vector(True if counts is None else counts, "counts", count, torch.int32, dev)
    visible, visible_ptr = _contact_vector(visible, "visible", count, torch.int32, dev)
    hidden, hidden_ptr = _contact_vector(hidden, "hidden", count, torch.int32, dev)
    if not fields and all(t is None for t in (index, counts, visible, hidden)):
        raise ValueError("nothing to do: ask for an output (fields, index, counts, visible or hidden)")
    if count > 0:  # (an empty tensor has no address to hand over)
        swarm.nearest_visible_device(first, count, k, radius, fields, rows_ptr, code, stride, index_ptr, istride, counts_ptr, visible_ptr,
                                     hidden_ptr, _stream(dev))
    rows = None
    if fields:
        rows = out[:, :width] if out.shape[1] > width else out
    if index is not None and index.shape[1] > k:
        index = index[:, :k]
    return rows, index, counts, visible, hidden


def scan_ring(n, elevation=0.0):
    """n unit vectors [n, 3] (numpy, FP64) evenly spaced in azimuth, beam 0 along +x, counter-clockwise seen from above, all at
    `elevation` radians above the xy plane: a planar lidar's pattern for set_scan_beams()."""
    import numpy as np
    if n < 1:
        raise ValueError(f"scan_ring needs n >= 1, got {n}")
    az = 2.0 * np.pi * np.arange(n) / n
    return _unit(np.stack([np.cos(az) * np.cos(elevation), np.sin(az) * np.cos(elevation), np.full(n, np.sin(elevation))], axis=1))


def scan_grid(n_h, n_v, fov_h, fov_v):
    """n_v rows of n_h unit vectors [n_v * n_h, 3] (numpy, FP64) around +x: azimuths evenly spaced over [-fov_h / 2, fov_h / 2] (left
    to right: descending azimuth), elevations over [fov_v / 2, -fov_v / 2] (top row first), radians; a single column or row looks
    straight ahead.  A depth camera's pattern for set_scan_beams(), row-major like an image."""
    import numpy as np
    if n_h < 1 or n_v < 1:
        raise ValueError(f"scan_grid needs n_h >= 1 and n_v >= 1, got {n_h} x {n_v}")
    az = np.linspace(fov_h / 2.0, -fov_h / 2.0, n_h) if n_h > 1 else np.zeros(1)
    el = np.linspace(fov_v / 2.0, -fov_v / 2.0, n_v) if n_v > 1 else np.zeros(1)
    el, az = (a.reshape(-1) for a in np.meshgrid(el, az, indexing="ij"))
    return _unit(np.stack([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)], axis=1))


def _unit(v):
    """rows of v over their norms (what cos and sin leave is a few ulps from 1: far inside the setter's 1e-9)"""
    import numpy as np
    return v / np.sqrt((v * v).sum(axis=1, keepdims=True))


def set_scan_beams(swarm, dirs):
    """Replaces the swarm's beam pattern of the range scans (mrs_swarm_set_scan_beams): dirs [B, 3], unit vectors (a tensor of any
    device, or an array; scan_ring() and scan_grid() make some).  One pattern for every UAV, B <= SCAN_MAX_BEAMS; B = 0 clears it.
    Rows that are not finite or whose squared norm differs from 1 by more than 1e-9 are refused: range_scan() never normalises."""
    import numpy as np
    d = _host_array(dirs, "dirs", np.float64, (-1, 3))
    if len(d) > SCAN_MAX_BEAMS:
        raise ValueError(f"{len(d)} beams: at most {SCAN_MAX_BEAMS}")
    if not np.isfinite(d).all():
        raise ValueError("dirs must be finite")
    with np.errstate(over="ignore"):
        if (np.abs(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) - 1.0) > 1e-9).any():
            raise ValueError("dirs must be unit vectors (squared norm within 1e-9 of 1)")
    swarm.set_scan_beams(d)


def range_scan(swarm, max_range, body_frame=True, ground=False, first=0, count=None, dtype=torch.float32, out=None, hits=None):
    """One range per beam of the swarm's pattern (set_scan_beams) for each UAV of [first, first + count), cast from the UAV's position
    against the static obstacles that apply to it and, with ground=True, the ground plane of its airframe
    (mrs_swarm_range_scan_device).  body_frame: the beams turn with the UAV's attitude (else they are world directions).  Returns
    (ranges, hits): ranges [count, B] of `dtype` (max_range where nothing is hit closer than that), hits int32 [count, B] (the obstacle
    index, SCAN_HIT_NONE or SCAN_HIT_GROUND) when hits=True or a tensor is given, else None.  `out` and `hits` are used instead of new
    tensors when given; columns past B are left alone.  No simulation state is written; a pending collision tick stays pending."""
    count = _count(swarm, first, count)
    dev = swarm.device()
    max_range, nb = _scan_args(swarm, max_range)
    out, code, stride = _scan_ranges(out, count, nb, dtype, dev)
    hits, hptr, hstride = _scan_int_rows(hits, count, nb, dev)
    flags = (SCAN_BODY_FRAME if body_frame else 0) | (SCAN_GROUND if ground else 0)
    swarm.range_scan_device(first, count, max_range, flags, out.data_ptr(), code, stride, hptr, hstride, _stream(dev))
    return _first_columns(out, nb), _first_columns(hits, nb)


def _scan_args(swarm, max_range):
    """(max_range as a float, beams of the swarm's pattern) of a scan, or the ValueError of a max_range that is no finite number > 0 or
    of a swarm without a pattern"""
    import math
    try:
        max_range = float(max_range)  # (numpy scalars and one-element tensors too)
    except (TypeError, ValueError):
        raise ValueError(f"max_range must be a finite number > 0, got {max_range!r}") from None
    if not (math.isfinite(max_range) and max_range > 0):
        raise ValueError(f"max_range must be a finite number > 0, got {max_range!r}")
    nb = swarm.scan_beam_count()
    if nb == 0:
        raise ValueError("no beam pattern set: call set_scan_beams() first")
    return max_range, nb


def _scan_ranges(out, count, nb, dtype, dev):
    """the range rows of a scan: (tensor, dtype code, stride) of `out`, or of a new [count, nb] tensor of `dtype`"""
    if out is None:
        out = torch.empty((count, nb), dtype=dtype, device=torch.device("cuda", dev))
    return out, _dtype_code(out.dtype), check_tensor(out, count, nb, out.dtype, dev)


def _scan_int_rows(rows, count, nb, dev):
    """an optional int32 output of a scan (hit or UAV indices): (tensor or None, pointer, stride) — True: a new [count, nb] tensor; a
    tensor: checked and filled; None or False: none"""
    if rows is True:
        rows = torch.empty((count, nb), dtype=torch.int32, device=torch.device("cuda", dev))
    if rows is False or rows is None:
        return None, 0, 0
    stride = check_tensor(rows, count, nb, torch.int32, dev)
    return rows, rows.data_ptr(), stride


def _first_columns(t, nb):
    return None if t is None else t[:, :nb] if t.shape[1] > nb else t


def range_scan_uavs(swarm, max_range, body_frame=True, ground=False, first=0, count=None, dtype=torch.float32, out=None, hits=None, uavs=None):
    """range_scan() that also sees the other UAVs of each observer's world (mrs_swarm_range_scan_uavs_device): UAV j is the closed sphere
    of radius arm_length + prop_radius of its airframe around its position.  Per beam the obstacles are considered first, then the UAVs
    (the nearest, ties to the lower index; it takes the beam only when strictly nearer than the obstacle), then the ground.  Returns
    (ranges, hit, uav): ranges as range_scan(); hit int32 [count, B] with UAVSCAN_HIT_UAV where a UAV took the beam; uav int32 [count, B]
    with that UAV's index, -1 elsewhere.  hits / uavs: True for new tensors, a tensor to fill, None for none (returned as None).  No
    simulation state is written; a pending collision tick stays pending."""
    count = _count(swarm, first, count)
    dev = swarm.device()
    max_range, nb = _scan_args(swarm, max_range)
    out, code, stride = _scan_ranges(out, count, nb, dtype, dev)
    hits, hptr, hstride = _scan_int_rows(hits, count, nb, dev)
    uavs, uptr, ustride = _scan_int_rows(uavs, count, nb, dev)
    flags = (SCAN_BODY_FRAME if body_frame else 0) | (SCAN_GROUND if ground else 0)
    swarm.range_scan_uavs_device(first, count, max_range, flags, out.data_ptr(), code, stride, hptr, hstride, uptr, ustride, _stream(dev))
    return _first_columns(out, nb), _first_columns(hits, nb), _first_columns(uavs, nb)


def set_worlds(swarm, worlds, first=0):
    """Collision-world labels of UAVs [first, first + len(worlds)) from an int32 vector on the swarm's device
    (mrs_swarm_set_worlds_device): UAVs interact through the collision pass, and appear in each other's rows of nearest(), only if
    their labels are equal.  The fork of a planner: save the M-UAV scene, load(index=i % M) into S * M UAVs, set_worlds(i // M)."""
    if not isinstance(worlds, torch.Tensor) or worlds.dim() != 1:
        raise ValueError("worlds must be an int32 vector")
    count = worlds.shape[0]
    if first < 0 or first + count > swarm.n:
        raise ValueError(f"{count} labels from UAV {first} on do not fit a swarm of {swarm.n} UAVs")
    dev = swarm.device()
    check_tensor(worlds, count, None, torch.int32, dev)
    swarm.set_worlds_device(first, count, worlds.data_ptr(), _stream(dev))


def _check_records(records, rows, dev):
    """records: a dense torch.uint8 [rows, SNAP_BYTES] tensor on the swarm's device, 16-B aligned"""
    check_tensor(records, rows, SNAP_BYTES, torch.uint8, dev)
    if records.shape[1] != SNAP_BYTES:
        raise ValueError(f"records must be [{rows}, {SNAP_BYTES}], got shape {tuple(records.shape)}")
    if rows > 1 and records.stride(0) != SNAP_BYTES:
        raise ValueError(f"records are not contiguous (row stride {records.stride(0)}, expected {SNAP_BYTES})")
    if records.data_ptr() % 16:
        raise ValueError("records must start on a 16-B boundary")


def save(swarm, first=0, count=None, out=None):
    """The whole simulation state of UAVs [first, first + count) as snapshot records (mrs_swarm_save_device): a torch.uint8
    [count, SNAP_BYTES] tensor on the swarm's device, one SNAPSHOT_DTYPE record per row (snapshot_fields gives views of the fields).
    `out` is used instead of a new tensor when given."""
    count = _count(swarm, first, count)
    dev = swarm.device()
    if out is None:
        out = torch.empty((count, SNAP_BYTES), dtype=torch.uint8, device=torch.device("cuda", dev))
    _check_records(out, count, dev)
    swarm.save_device(first, count, out.data_ptr(), _stream(dev))
    return out


def load(swarm, records, first=0, index=None, status=None):
    """Write snapshot records back (mrs_swarm_load_device).  Without `index`, UAV first + k <- records[k] for every row of `records`;
    with `index` (an int32 vector), UAV first + k <- records[index[k]] (one record may go to many UAVs; -1 leaves the UAV alone).
    Command, feed-forwards, mode, airframe and hold flag are kept.  Returns the uint8 status vector (SNAP_LOADED, SNAP_SKIPPED,
    SNAP_BAD_AIRFRAME, SNAP_BAD_INDEX, SNAP_BAD_MAGIC), written into `status` when given."""
    dev = swarm.device()
    if not isinstance(records, torch.Tensor) or records.dim() != 2:
        raise ValueError("records must be a [n_records, SNAP_BYTES] torch.uint8 tensor")
    n_records = records.shape[0]
    _check_records(records, n_records, dev)
    if index is None:
        count, iptr = n_records, 0
    else:
        if not isinstance(index, torch.Tensor) or index.dim() != 1:
            raise ValueError("index must be an int32 vector")
        count = index.shape[0]
        check_tensor(index, count, None, torch.int32, dev)
        iptr = index.data_ptr()
    if status is None:
        status = torch.empty(count, dtype=torch.uint8, device=torch.device("cuda", dev))
    check_tensor(status, count, None, torch.uint8, dev)
    swarm.load_device(first, count, records.data_ptr(), n_records, iptr, status.data_ptr(), _stream(dev))
    return status


def snapshot_fields(records):
    """Views of the fields of snapshot records ([n, SNAP_BYTES] torch.uint8) that share their memory: x, v, v_prev, omega,
    imu_acceleration, external_force [n, 3], R [n, 3, 3], motor_rpm [n, 8], initial_z [n], pid [n, 24] (float64), flags, airframe,
    magic [n] (int32; SNAP_* bits in flags).  Editing a view edits the records, so a caller can move saved UAVs before loading them."""
    if not isinstance(records, torch.Tensor) or records.dtype != torch.uint8 or records.dim() != 2 or records.shape[1] != SNAP_BYTES:
        raise ValueError("records must be a [n, SNAP_BYTES] torch.uint8 tensor")
    if records.shape[0] > 1 and records.stride(0) != SNAP_BYTES or records.stride(1) != 1:
        raise ValueError("records are not contiguous")
    d, w = records.view(torch.float64), records.view(torch.int32)
    out = {}
    for name in SNAPSHOT_DTYPE.names:
        dt, off = SNAPSHOT_DTYPE.fields[name][:2]
        if name == "_reserved":
            continue
        if dt.base.kind == "f":
            a, size = off // 8, max(1, dt.itemsize // 8)
            out[name] = d[:, a] if not dt.shape else d[:, a:a + size].unflatten(1, dt.shape)
        else:
            out[name] = w[:, off // 4]
    return out
