"""Mask slices interpolated on the GPU: shape-based interpolation (Raya and Udupa) between the slices of a mask stack -- every bracketing
plane becomes a SIGNED squared distance map, two maps are blended with integer weights and cut at zero (``csrc/distance.hip`` behind
``octseg_stack_signed_distance`` and ``octseg_signed_blend``).  It repairs what only the slice axis shows and ``lesions.clean_volume`` does not:
a lesion the network skipped in one frame (one lesion turned into two), a frame the operator rejects; and it makes the slices in between that
a longitudinal view or a near-isotropic volume needs.  The reference has no counterpart.

    sd2 = signed_distance_stack(stack)                          # int32 CUDA [N, channels, H, W]
    blend_planes(sd2, plan, out, made=None)                     # the thin wrapper: plan rows -> planes of ``out``
    plan = gap_plan(present, max_gap, frames=None)              # pure numpy: which planes to make, from which, with which weights
    bridged = bridge_gaps(stack, max_gap=1, frames=None)        # a new stack, gaps of at most max_gap slices filled, rejected frames re-made
    dense = resample_stack(stack, factor)                       # [(N - 1) * factor + 1, H, W, channels]
    report = bridge_report(plan, made, names)                   # JSON-clean: per class the slices made, from which, how many pixels

``stack`` is float32 CUDA [N, H, W, channels], any value != 0 set; a plane is one (slice, channel) pair.  Definitions (DESIGN.md section 5s,
``include/octseg.h``):

* ``sd2``: at a set pixel ``+d2`` to the nearest clear pixel of the plane (>= 1), at a clear pixel ``-d2`` to the nearest set pixel (<= -1),
  ``-DIST_NONE`` everywhere on an empty plane, ``+DIST_NONE`` on a full one, never 0:
  ``where(m, distance_stack(to='clear'), -distance_stack(to='set'))``.
* The BLEND of planes a and b with integer weights ``0 <= wa, wb <= 32767``, not both 0: with ``s = sign(sd2) * sqrt(|sd2|)`` (``DIST_NONE`` is
  infinite) a pixel is set iff ``wa * s_a + wb * s_b > 0``, decided in integers: a weight of 0 removes its side; equal signs decide; opposite
  finite signs compare ``w^2 * |sd2|`` in int64; an infinite side beats a finite one; two infinite sides go by the weights; a tie is clear.
* A PLAN is int32 [M, 6], rows ``(channel, out_slice, lo, hi, w_lo, w_hi)``: plane ``(out_slice, channel)`` of the output becomes the blend of
  planes ``(lo, channel)`` and ``(hi, channel)`` as 0.0 / 1.0.  Planes no row names are not touched.

Everything is integer: results EQUAL the scipy restatement of ``tests/interp_ref.py``, no tolerance.  What the method cannot do, by design: it
knows no correspondence between slices, so objects that do not overlap vanish (two radius-8 discs 20 px apart blend to nothing; vasa vasorum
blobs that move between frames give nothing back); nothing is extrapolated past the first or last present slice; weights are integers; no key
is added to ``lesion_report`` / ``analyze_stack`` / ``plaque_report``; 3-D hole fill and 3-D closing are not part of it.
"""
import numpy as np
import torch

from . import _lib as L
from .distance import DEFAULT_SCRATCH, DIST_NONE, _check, _names

MAX_WEIGHT = 32767


def _signed_chunk(n, h, w, channels, scratch_bytes, device):
    """(slices per call, scratch tensor, its bytes) under the budget; one slice is the smallest chunk."""
    per_slice = int(L.lib().octseg_signed_distance_scratch_bytes(1, h, w, channels))
    step = max(min(n, int(scratch_bytes) // per_slice), 1)
    need = int(L.lib().octseg_signed_distance_scratch_bytes(step, h, w, channels))
    return step, torch.empty((need,), dtype=torch.uint8, device=device), need


def signed_distance_stack(stack, scratch_bytes=DEFAULT_SCRATCH):
    """int32 CUDA [N, channels, H, W]: the signed squared distance of every pixel of every plane (module docstring).  Processed in chunks of
    slices under ``scratch_bytes``; the result does not depend on the chunking.  The input is not modified."""
    stack, n, h, w, sc = _check(stack)
    out = torch.empty((n, sc, h, w), dtype=torch.int32, device=stack.device)
    with torch.cuda.device(stack.device):
        step, scratch, nbytes = _signed_chunk(n, h, w, sc, scratch_bytes, stack.device)
        for i in range(0, n, step):
            m = min(step, n - i)
            L.check(L.lib().octseg_stack_signed_distance(L.ptr(stack[i:i + m]), m, h, w, sc, L.ptr(scratch), nbytes, L.ptr(out[i:i + m]),
                                                         L.stream_ptr()))
    return out


def check_plan(plan, keys, channels, n_out):
    """``plan`` as a contiguous int32 numpy [M, 6], or ``ValueError``: no row, a row outside ``channels`` / ``n_out`` output slices / ``keys``
    key slices, a weight outside 0..32767 or both weights 0, two rows that name the same output plane."""
    if torch.is_tensor(plan):
        plan = plan.cpu().numpy()
    plan = np.asarray(plan)
    if plan.ndim != 2 or plan.shape[1] != 6 or plan.shape[0] < 1 or not np.issubdtype(plan.dtype, np.integer):
        raise ValueError(f'plan must be integers [M, 6] with M >= 1: rows (channel, out_slice, lo, hi, w_lo, w_hi), got {plan.dtype} {plan.shape}')
    plan = plan.astype(np.int64)
    c, o, lo, hi, wa, wb = plan.T
    if ((c < 0) | (c >= channels)).any():
        raise ValueError(f'a plan row names a channel outside 0..{channels - 1}')
    if ((o < 0) | (o >= n_out)).any():
        raise ValueError(f'a plan row names an output slice outside 0..{n_out - 1}')
    if ((lo < 0) | (lo >= keys) | (hi < 0) | (hi >= keys)).any():
        raise ValueError(f'a plan row names a key slice outside 0..{keys - 1}')
    if ((wa < 0) | (wa > MAX_WEIGHT) | (wb < 0) | (wb > MAX_WEIGHT)).any():
        raise ValueError(f'weights must lie in 0..{MAX_WEIGHT}')
    if ((wa == 0) & (wb == 0)).any():
        raise ValueError('a plan row has both weights 0')
    if np.unique(o * channels + c).size != plan.shape[0]:
        raise ValueError('two plan rows name the same output plane')
    return np.ascontiguousarray(plan.astype(np.int32))


def blend_planes(sd2, plan, out, made=None):
    """The thin wrapper of ``octseg_signed_blend``: every row ``(channel, out_slice, lo, hi, w_lo, w_hi)`` of ``plan`` (array-like int [M, 6])
    writes plane ``(out_slice, channel)`` of ``out`` (float32 CUDA [N_out, H, W, channels], contiguous, written in place) as 0.0 / 1.0, the
    blend of planes ``(lo, channel)`` and ``(hi, channel)`` of ``sd2`` (int32 CUDA [K, channels, H, W]); planes no row names keep their values.
    ``made`` (int32 CUDA [M], optional) receives the set pixels of each written plane.  ``ValueError`` before the call for rows out of range,
    weights outside 0..32767 or both 0, and two rows that name the same output plane.  Returns ``out``."""
    if not (torch.is_tensor(sd2) and sd2.is_cuda and sd2.dtype == torch.int32 and sd2.dim() == 4 and sd2.is_contiguous()):
        raise ValueError('sd2 must be a contiguous int32 CUDA tensor [K, channels, H, W]')
    if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 4 and out.is_contiguous()):
        raise ValueError('out must be a contiguous float32 CUDA tensor [N_out, H, W, channels]')
    k, sc, h, w = (int(v) for v in sd2.shape)
    n_out = int(out.shape[0])
    if tuple(out.shape[1:]) != (h, w, sc) or out.device != sd2.device or 0 in sd2.shape or n_out < 1:
        raise ValueError(f'out {tuple(out.shape)} must be [N_out, {h}, {w}, {sc}] on the device of sd2, nothing empty')
    plan = check_plan(plan, k, sc, n_out)
    m = int(plan.shape[0])
    if made is not None and not (torch.is_tensor(made) and made.is_cuda and made.dtype == torch.int32 and made.is_contiguous()
                                 and tuple(made.shape) == (m,) and made.device == sd2.device):
        raise ValueError(f'made must be a contiguous int32 CUDA tensor [{m}] on the device of sd2')
    with torch.cuda.device(sd2.device):
        plan_dev = torch.from_numpy(plan).to(sd2.device)
        L.check(L.lib().octseg_signed_blend(L.ptr(sd2), k, h, w, sc, L.ptr(plan_dev), m, L.ptr(out), n_out, L.ptr(made), L.stream_ptr()))
    return out


def _runs(flags):
    """The maximal runs of True in a 1-D bool array as (first, last) pairs."""
    idx = np.flatnonzero(flags)
    if idx.size == 0:
        return []
    cut = np.flatnonzero(np.diff(idx) > 1)
    return list(zip(idx[np.r_[0, cut + 1]].tolist(), idx[np.r_[cut, idx.size - 1]].tolist()))


def gap_plan(present, max_gap, frames=None):
    """The plan (int32 numpy [M, 6], rows ``(channel, out_slice, lo, hi, w_lo, w_hi)`` sorted by channel, then slice; M may be 0) that bridges
    the gaps of a stack.  Pure numpy.  ``present`` bool [N, channels]: whether plane (slice, channel) holds a pixel.

    * For channel c, a maximal run of absent slices STRICTLY between two present slices ``lo < hi`` with ``hi - lo - 1 <= max_gap`` yields the rows
      ``(c, k, lo, hi, hi - k, k - lo)`` for every k in between: the nearer neighbour weighs more.  A run that touches either end of the stack is
      never filled: nothing is extrapolated.
    * ``frames``: the slices the operator REJECTS.  Their planes are re-made for EVERY channel from the nearest accepted slices ``lo < k < hi`` on
      either side, whatever those planes hold, with the same weights (an empty neighbour is at minus infinity: nothing appears unless both
      neighbours hold the class).  A rejected run at an end of the stack is a copy of the nearest accepted slice a (``(c, k, a, a, 1, 0)``: weight
      0 on the missing side).  A rejected run longer than ``max_gap``, or a stack with no accepted slice, raises ``ValueError``.  A rejected
      slice counts as absent in every channel and is never a neighbour, and the first rule writes no row for it: it has the rows of this rule."""
    present = np.asarray(present)
    if present.ndim != 2 or present.dtype != np.bool_ or 0 in present.shape:
        raise ValueError(f'present must be a bool array [N, channels], got {present.dtype} {present.shape}')
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or int(max_gap) < 0:
        raise ValueError(f'max_gap must be an integer >= 0, got {max_gap!r}')
    max_gap = int(max_gap)
    n, channels = present.shape
    rejected = np.zeros((n,), bool)
    if frames is not None:
        for f in frames:
            if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or not 0 <= int(f) < n:
                raise ValueError(f'frames must be slice numbers in 0..{n - 1}, got {f!r}')
            rejected[int(f)] = True
    rows = []
    if rejected.any():
        if rejected.all():
            raise ValueError('every slice is rejected: there is nothing to re-make them from')
        for a, b in _runs(rejected):
            if b - a + 1 > max_gap:
                raise ValueError(f'rejected slices {a}..{b}: a run of {b - a + 1} is longer than max_gap={max_gap}')
            lo, hi = a - 1, b + 1
            for c in range(channels):
                for k in range(a, b + 1):
                    if lo < 0:
                        rows.append((c, k, hi, hi, 1, 0))
                    elif hi >= n:
                        rows.append((c, k, lo, lo, 1, 0))
                    else:
                        rows.append((c, k, lo, hi, hi - k, k - lo))
    for c in range(channels):
        have = present[:, c] & ~rejected
        idx = np.flatnonzero(have)
        for lo, hi in zip(idx[:-1].tolist(), idx[1:].tolist()):
            if 1 <= hi - lo - 1 <= max_gap:
                rows.extend((c, k, lo, hi, hi - k, k - lo) for k in range(lo + 1, hi) if not rejected[k])
    rows.sort()
    return np.array(rows, dtype=np.int32).reshape(-1, 6)


def bridge_gaps(stack, max_gap=1, frames=None, return_plan=False, scratch_bytes=DEFAULT_SCRATCH):
    """A new stack in which the planes ``gap_plan`` names are interpolated from their neighbours: gaps of at most ``max_gap`` slices inside a
    class are filled, the slices listed in ``frames`` are re-made for every class.  Every other plane is copied as it is; the input is not
    modified.  Presence comes from the device (one reduction and one small copy to the host); only the key slices the plan names are gathered
    and mapped.  ``return_plan=True``: ``(stack, plan, made)`` with ``plan`` the int32 numpy [M, 6] of ``gap_plan`` and ``made`` int32 numpy
    [M], the set pixels of every plane made."""
    stack, n, h, w, sc = _check(stack)
    present = (stack != 0).any(dim=2).any(dim=1).cpu().numpy()
    plan = gap_plan(present, max_gap, frames)
    out = stack.clone()
    made = np.zeros((plan.shape[0],), np.int32)
    if plan.shape[0]:
        keys = np.unique(plan[:, 2:4])
        local = plan.copy()
        local[:, 2:4] = np.searchsorted(keys, plan[:, 2:4])
        with torch.cuda.device(stack.device):
            sd2 = signed_distance_stack(stack[torch.from_numpy(keys.astype(np.int64)).to(stack.device)], scratch_bytes)
            made_dev = torch.empty((plan.shape[0],), dtype=torch.int32, device=stack.device)
            blend_planes(sd2, local, out, made_dev)
        made = made_dev.cpu().numpy()
    return (out, plan, made) if return_plan else out


def resample_plan(first, last, factor, channels, with_first=True):
    """The plan rows of ``resample_stack`` for the key slices ``first .. last`` (numbers inside a window that starts at key slice ``first``):
    output slice ``i * factor + j`` between keys i and i + 1 blends them with weights ``(factor - j, j)``; a key slice is its own map's sign
    (``(c, i * factor, i, i, 1, 0)``).  Sorted by output slice, then channel."""
    rows = []
    for o in range(first * factor + (0 if with_first else 1), last * factor + 1):
        i, j = divmod(o, factor)
        for c in range(channels):
            rows.append((c, o, i - first, i - first, 1, 0) if j == 0 else (c, o, i - first, i - first + 1, factor - j, j))
    return np.array(rows, dtype=np.int32).reshape(-1, 6)


def resample_stack(stack, factor, scratch_bytes=DEFAULT_SCRATCH):
    """float32 CUDA [(N - 1) * factor + 1, H, W, channels]: ``factor - 1`` slices interpolated between every two neighbours.  Key slice i is
    output slice ``i * factor``, copied as 0.0 / 1.0; slice j of a gap is the blend of its two key slices with weights ``(factor - j, j)``.
    ``factor`` is an integer in 1..32767; ``factor=1`` is the identity (as 0.0 / 1.0).  Works in windows of key slices: a window's scratch and
    maps (per slice ``octseg_signed_distance_scratch_bytes(1, ...)`` + 4 bytes per pixel and channel) stay under ``scratch_bytes``, two key
    slices being the smallest window; the result does not depend on the windows."""
    if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)) or not 1 <= int(factor) <= MAX_WEIGHT:
        raise ValueError(f'factor must be an integer in 1..{MAX_WEIGHT}, got {factor!r}')
    factor = int(factor)
    stack, n, h, w, sc = _check(stack)
    out = torch.empty(((n - 1) * factor + 1, h, w, sc), dtype=torch.float32, device=stack.device)
    per_slice = int(L.lib().octseg_signed_distance_scratch_bytes(1, h, w, sc)) + 4 * h * w * sc
    window = min(n, max(int(scratch_bytes) // per_slice, 2))
    first = 0
    while True:
        last = min(first + window - 1, n - 1)
        sd2 = signed_distance_stack(stack[first:last + 1], scratch_bytes)
        plan = resample_plan(first, last, factor, sc, with_first=first == 0)
        plan[:, 1] -= first * factor
        blend_planes(sd2, plan, out[first * factor:last * factor + 1])
        if last == n - 1:
            return out
        first = last


def bridge_report(plan, made, names=None, classes=None, channels=None):
    """A JSON-clean dict of what ``bridge_gaps`` made: ``{class name: {'slice', 'lo', 'hi', 'w_lo', 'w_hi', 'pixels', 'image'}}``, lists with one
    entry per plane made, in slice order -- the slice, the two slices it was blended from and their weights, the set pixels made, and the slice's
    image name (``names[slice]``; ``None`` without names).  ``classes`` as in ``distance.surface_metrics``: None = the pipeline's layout, or the
    names of the channels in order; ``channels``: the stack's channel count (default: what the plan and the class layout need).  Pure host."""
    plan = np.asarray(plan, np.int64).reshape(-1, 6)
    made = np.asarray(made, np.int64).reshape(-1)
    if made.shape[0] != plan.shape[0]:
        raise ValueError(f'{plan.shape[0]} plan rows but {made.shape[0]} pixel counts')
    if channels is None:
        channels = max(int(plan[:, 0].max()) + 1 if plan.shape[0] else 1, len(classes) if classes is not None else 4)
    by_channel = dict(_names(classes, int(channels)))
    out = {name: {k: [] for k in ('slice', 'lo', 'hi', 'w_lo', 'w_hi', 'pixels', 'image')} for name in by_channel.values()}
    for (c, o, lo, hi, wa, wb), px in sorted(zip(map(tuple, plan.tolist()), made.tolist())):
        if c not in by_channel:
            continue
        col = out[by_channel[c]]
        for k, v in zip(('slice', 'lo', 'hi', 'w_lo', 'w_hi', 'pixels'), (o, lo, hi, wa, wb, px)):
            col[k].append(int(v))
        col['image'].append(None if names is None else str(names[o]))
    return out
