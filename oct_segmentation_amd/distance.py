"""Boundary distances on the GPU: exact Euclidean distance maps of the mask stacks the pipeline carries, the Hausdorff family between a predicted
and a ground-truth stack, and the shortest lumen-to-lipid distance (``csrc/distance.hip`` behind ``octseg_stack_boundary``,
``octseg_stack_distance`` and the ``octseg_pair_distance_*`` calls).  The reference scores overlap only; this has no counterpart there.

    edge = boundary_stack(stack)                               # float32 0 / 1, the input's layout
    d2 = distance_stack(stack, to='boundary')                  # int32 CUDA [N, channels, H, W], SQUARED distances; DIST_NONE where there is no target
    d2, offsets, target_count = directed_distances(pred, truth)
    report = surface_metrics(pred, truth)                      # per class and slice: hd, hd95, assd, dice, iou
    cap = cap_distance(stack)                                  # per slice: the shortest lipid-core-to-lumen distance and where it is attained

``stack`` is float32 CUDA [N, H, W, channels], any value != 0 set; a plane is one (slice, channel) pair.  Definitions:

* The BOUNDARY of a plane is ``m & ~erode(m)`` with the 4-neighbour cross, the outside of the frame counting as clear, so a set pixel on the frame
  edge is boundary: ``m & ~scipy.ndimage.binary_erosion(m, generate_binary_structure(2, 1), border_value=0)``.
* A DISTANCE runs from pixel centre to pixel centre.  The device works on squared distances in int32 (``rint(distance_transform_edt(~target) **
  2)``), no floating point in any decision; ``sqrt`` is taken in float64 on the host.  Two touching masks are at distance 1.
* DIRECTED distances from A to B: for every boundary pixel of A the distance to the nearest boundary pixel of B.
  ``hd`` = the larger of the two directed maxima, ``hd95`` = the larger of the two directed ``np.percentile(., 95)`` (linear interpolation),
  ``assd`` = (sum A->B + sum B->A) / (n_A + n_B).  A slice where either mask is empty has no distance: ``None`` for all three.
* ``dice`` / ``iou`` come from the set-pixel counts of the same call, with smp's ``zero_division=1.0`` convention of ``metrics.py``.
* With ``ratio`` given, distances are divided by it as ``analysis.py`` divides its lengths; without it they are pixels.

Limits, refused with a message: H, W <= 4096 (squared distances stay below 2^25), at most 16 channels, N * pairs < 2^31.  Everything is integer:
results EQUAL the scipy restatement of ``tests/distance_ref.py``, no tolerance.  Out of scope: surfel-weighted or
sub-pixel surface distances, ``thickness='contour'`` (still refused by ``analysis``); nothing is added to ``plaque_report`` / ``analyze_stack``.

    python -m oct_segmentation_amd.distance pred_dir truth_dir [save_dir]      # mask TIFFs of equal names -> save_dir/surface_metrics.json

The same over the VOLUME the slices form (the ``octseg_volume_*`` distance calls; DESIGN.md section 5p, pinned by ``tests/distance3d_ref.py``):

    edge = boundary_volume(stack)                              # the 3-D boundary, float32 0 / 1
    d2 = distance_volume(stack, to='boundary', slice_step=10)  # int32 [N, channels, H, W]: (slice_step * dz)^2 + dy^2 + dx^2 to the nearest target voxel
    d2, offsets, target_count = directed_distances_volume(pred, truth, slice_step=10)
    report = volume_surface_metrics(pred, truth, slice_step=10)    # per class, one scalar each: n_pred, n_truth, hd, hd95, assd, dice, iou
    cap = cap_distance_volume(stack, slice_step=10)            # {'distance', 'at': (z, y, x), 'd2'} or None

* Each channel is read as a volume of N slices.  ``slice_step`` is the distance between neighbouring slices in pixels, an INTEGER >= 1 (rational
  spacing is out of scope); the squared distance between two voxels is ``(slice_step * dz)^2 + dy^2 + dx^2``, centre to centre, in int32
  (``rint(distance_transform_edt(~T, sampling=(slice_step, 1, 1)) ** 2)``).
* The 3-D BOUNDARY is ``m & ~erode(m)`` with the 6-neighbour cross, everything outside the volume clear: ``m & ~binary_erosion(m,
  generate_binary_structure(3, 1), border_value=0)``.  Every set voxel of the first and last slice is boundary, and with N <= 2 every set voxel
  is; there is no "open ends" variant.
* The TARGET of a distance is a part (``set``, ``clear``, the 3-D ``boundary``) taken over the whole volume of one channel: ``DIST_NONE``
  everywhere when the part is empty in the whole volume, never decided per slice.  A segment of the lists is a pair of channels.
* Further limits: ``slice_step * (N - 1) <= 32767`` (a squared distance stays below 2^30 + 2^25), ``N * H * W <= 2^32`` (the packed minimum
  holds the voxel index in 32 bits).  The per-slice map exists for a band of rows of all slices at a time (6 bytes per voxel of the band and
  target channel, under ``scratch_bytes``; ``volume_bands``); a budget below the one-row band raises and names the bytes needed.

    python -m oct_segmentation_amd.distance pred_dir truth_dir [save_dir] slice_step=K     # additionally save_dir/surface_metrics_3d.json
"""
import json
import os
import sys
from glob import glob

import numpy as np
import torch

from . import _lib as L
from .model import CLASS_IDS

DIST_NONE = 0x7fffffff
MAX_SIDE = 4096
MAX_CHANNELS = 16
PARTS = {'set': 0, 'clear': 1, 'boundary': 2}
DEFAULT_SCRATCH = 512 << 20


def check_extents(n, h, w, channels, pairs=1):
    """The limits of the kernels as ``ValueError``: empty extents, a side above 4096, more than 16 channels, N * pairs >= 2^31."""
    n, h, w, channels, pairs = int(n), int(h), int(w), int(channels), int(pairs)
    if n < 1 or h < 1 or w < 1 or channels < 1:
        raise ValueError('empty batch or frame')
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f'frame {h} x {w}: sides of at most {MAX_SIDE} (squared distances must stay below 2^25)')
    if channels > MAX_CHANNELS:
        raise ValueError(f'at most {MAX_CHANNELS} channels, got {channels}')
    if pairs < 1 or n * pairs >= 2 ** 31:
        raise ValueError(f'{n} slices x {pairs} pairs: at least one pair and fewer than 2^31 (slice, pair) segments')


def _check(stack):
    if not (torch.is_tensor(stack) and stack.is_cuda and stack.dtype == torch.float32 and stack.dim() == 4):
        raise ValueError('stack must be a float32 CUDA tensor [N, H, W, channels]')
    if 0 in stack.shape:
        raise ValueError('empty batch or frame')
    n, h, w, sc = (int(v) for v in stack.shape)
    check_extents(n, h, w, sc)
    return stack.contiguous(), n, h, w, sc


def _part(name, what):
    if name not in PARTS:
        raise ValueError(f"{what} must be one of {sorted(PARTS)}, got {name!r}")
    return PARTS[name]


def _chunk(n, h, w, ca, cb, pairs, scratch_bytes, device):
    """(slices per call, scratch tensor, its bytes) under the budget; one slice is the smallest chunk."""
    per_slice = int(L.lib().octseg_distance_scratch_bytes(1, h, w, ca, cb, pairs))
    step = max(min(n, int(scratch_bytes) // per_slice), 1)
    need = int(L.lib().octseg_distance_scratch_bytes(step, h, w, ca, cb, pairs))
    return step, torch.empty((need,), dtype=torch.uint8, device=device), need


def boundary_stack(stack, scratch_bytes=DEFAULT_SCRATCH):
    """The boundary of every plane (module docstring): float32 0.0 / 1.0 in the input's layout; the input is not modified."""
    stack, n, h, w, sc = _check(stack)
    out = torch.empty_like(stack)
    with torch.cuda.device(stack.device):
        step, scratch, nbytes = _chunk(n, h, w, sc, 0, 0, scratch_bytes, stack.device)
        for i in range(0, n, step):
            m = min(step, n - i)
            L.check(L.lib().octseg_stack_boundary(L.ptr(stack[i:i + m]), m, h, w, sc, L.ptr(scratch), nbytes, L.ptr(out[i:i + m]), L.stream_ptr()))
    return out


def distance_stack(stack, to='set', scratch_bytes=DEFAULT_SCRATCH):
    """int32 CUDA [N, channels, H, W]: the SQUARED Euclidean distance of every pixel to the nearest pixel of its own plane's ``to`` part --
    ``'set'`` (0 on the mask), ``'clear'`` (0 outside it: the depth inside the mask) or ``'boundary'``; ``DIST_NONE`` on a plane whose target is
    empty.  Processed in chunks of slices under ``scratch_bytes``; the result does not depend on the chunking."""
    to = _part(to, 'to')
    stack, n, h, w, sc = _check(stack)
    out = torch.empty((n, sc, h, w), dtype=torch.int32, device=stack.device)
    with torch.cuda.device(stack.device):
        step, scratch, nbytes = _chunk(n, h, w, sc, 0, 0, scratch_bytes, stack.device)
        for i in range(0, n, step):
            m = min(step, n - i)
            L.check(L.lib().octseg_stack_distance(L.ptr(stack[i:i + m]), m, h, w, sc, to, L.ptr(scratch), nbytes, L.ptr(out[i:i + m]), L.stream_ptr()))
    return out


def _check_pair(src, dst, pairs):
    src, n, h, w, ca = _check(src)
    dst, n2, h2, w2, cb = _check(dst)
    if (n, h, w) != (n2, h2, w2) or src.device != dst.device:
        raise ValueError(f'the two stacks must agree in slices, frame size and device, got {tuple(src.shape)} and {tuple(dst.shape)}')
    if pairs is None:
        if ca != cb:
            raise ValueError(f'pairs=None pairs equal channels, but the stacks have {ca} and {cb}')
        pairs = [(c, c) for c in range(ca)]
    pairs = [(int(a), int(b)) for a, b in pairs]
    for a, b in pairs:
        if not (0 <= a < ca and 0 <= b < cb):
            raise ValueError(f'pair {(a, b)} is outside stacks of {ca} and {cb} channels')
    check_extents(n, h, w, max(ca, cb), len(pairs))
    return src, dst, pairs, n, h, w, ca, cb


def _counts(src, dst, pairs_dev, npairs, sp, dp, dims, scratch_bytes):
    n, h, w, ca, cb = dims
    counts = torch.empty((n, npairs, 2), dtype=torch.int32, device=src.device)
    overlap = torch.empty((n, npairs, 3), dtype=torch.int32, device=src.device)
    step, scratch, nbytes = _chunk(n, h, w, ca, cb, npairs, scratch_bytes, src.device)
    for i in range(0, n, step):
        m = min(step, n - i)
        L.check(L.lib().octseg_pair_distance_counts(L.ptr(src[i:i + m]), L.ptr(dst[i:i + m]), m, h, w, ca, cb, L.ptr(pairs_dev), npairs, sp, dp,
                                                    L.ptr(scratch), nbytes, L.ptr(counts[i:i + m]), L.ptr(overlap[i:i + m]), L.stream_ptr()))
    return counts, overlap


def _fill_keys(src, dst, pairs_dev, npairs, sp, dp, dims, offsets_dev, keys, capacity, scratch_bytes):
    """The second launch of ``directed_distances``: one key per query pixel into ``keys[:capacity]``.  A key whose position lies outside the
    capacity is dropped on the device and turns into a ``RuntimeError`` here; nothing is ever stored past ``capacity``."""
    n, h, w, ca, cb = dims
    overflow = torch.zeros((1,), dtype=torch.int32, device=src.device)
    step, scratch, nbytes = _chunk(n, h, w, ca, cb, npairs, scratch_bytes, src.device)
    for i in range(0, n, step):
        m = min(step, n - i)
        L.check(L.lib().octseg_pair_distance_keys(L.ptr(src[i:i + m]), L.ptr(dst[i:i + m]), m, h, w, ca, cb, L.ptr(pairs_dev), npairs, sp, dp,
                                                  L.ptr(scratch), nbytes, i * npairs, L.ptr(offsets_dev[i * npairs:]), L.ptr(keys), int(capacity),
                                                  L.ptr(overflow), L.stream_ptr()))
    if int(overflow.item()):
        raise RuntimeError(f'directed_distances: the key buffer of {int(capacity)} entries is too small for the query pixels; keys were dropped')


def _lists(src, dst, pairs, src_part, dst_part, scratch_bytes):
    """``(d2, offsets, target_count, overlap)`` as numpy: see ``directed_distances``; ``overlap`` int32 [N, P, 3] = |a & b|, |a|, |b|."""
    sp, dp = _part(src_part, 'src_part'), _part(dst_part, 'dst_part')
    src, dst, pairs, n, h, w, ca, cb = _check_pair(src, dst, pairs)
    npairs, dims = len(pairs), (n, h, w, ca, cb)
    with torch.cuda.device(src.device):
        pairs_dev = torch.tensor(pairs, dtype=torch.int32, device=src.device).reshape(npairs, 2)
        counts, overlap = _counts(src, dst, pairs_dev, npairs, sp, dp, dims, scratch_bytes)
        host = torch.cat([counts, overlap], dim=2).cpu().numpy()               # the one synchronisation: the offsets need the counts
        offsets = np.zeros((n * npairs + 1,), np.int64)
        np.cumsum(host[:, :, 0].reshape(-1), out=offsets[1:])
        total = int(offsets[-1])
        if total:
            keys = torch.empty((total,), dtype=torch.int64, device=src.device)
            _fill_keys(src, dst, pairs_dev, npairs, sp, dp, dims, torch.from_numpy(offsets[:-1].copy()).to(src.device), keys, total, scratch_bytes)
            keys = torch.sort(keys).values
            seg = (keys >> 32).cpu().numpy()
            d2 = (keys & 0xffffffff).cpu().numpy()
            if not np.array_equal(np.bincount(seg, minlength=n * npairs), np.diff(offsets)):
                raise RuntimeError('directed_distances: the keys written do not match the counted query pixels')
        else:
            d2 = np.zeros((0,), np.int64)
    return d2, offsets, host[:, :, 1].copy(), host[:, :, 2:].copy()


def directed_distances(src, dst, pairs=None, src_part='boundary', dst_part='boundary', scratch_bytes=DEFAULT_SCRATCH):
    """For every slice and every ``(src channel, dst channel)`` of ``pairs`` (default: equal channels), the SQUARED distance from each pixel of the
    source plane's ``src_part`` to the nearest pixel of the target plane's ``dst_part`` (parts: ``'boundary'``, ``'set'``, ``'clear'``).
    Returns ``(d2, offsets, target_count)``: ``d2`` int64 numpy, the values of segment ``s = slice * len(pairs) + pair`` are
    ``d2[offsets[s]:offsets[s + 1]]`` in ascending order; ``offsets`` int64 [N * P + 1]; ``target_count`` int32 [N, P], the target pixels.
    Where the target is empty the values are ``DIST_NONE``.  Two launches with one host synchronisation between them (the offsets are the
    running sum of the query counts); ``torch.sort`` over the keys makes the result independent of the order the pixels were written in."""
    return _lists(src, dst, pairs, src_part, dst_part, scratch_bytes)[:3]


def _names(classes, channels):
    """Channel -> class name.  None: the pipeline's layout, channel ``CLASS_IDS[name] - 1``; a list: channel i holds ``classes[i]``."""
    if classes is None:
        return [(cid - 1, name) for name, cid in sorted(CLASS_IDS.items(), key=lambda kv: kv[1]) if cid <= channels]
    classes = [str(c) for c in classes]
    if len(classes) > channels or len(set(classes)) != len(classes):
        raise ValueError(f'{len(classes)} class names (distinct ones) for a stack of {channels} channels')
    return list(enumerate(classes))


def build_surface_metrics(d2, offsets, counts, classes, ratio=None, percentile=95):
    """The report of ``surface_metrics`` from the integers.  Pure host, float64 numpy.
    ``d2`` = ``(pred -> truth, truth -> pred)``, each the sorted squared distances of ``directed_distances``; ``offsets`` = their two offset
    arrays [N * P + 1]; ``counts`` int [N, P, 3] = |pred & truth|, |pred|, |truth| set pixels; ``classes`` the P names.
    Returns ``{name: {'slice', 'n_pred', 'n_truth', 'hd', 'hd95', 'assd', 'dice', 'iou'}}``, every value a list with one entry per slice:
    ``n_pred`` / ``n_truth`` the boundary pixels, the three distances ``None`` where either is 0 (module docstring)."""
    d_ab, d_ba = (np.asarray(v, np.int64) for v in d2)
    o_ab, o_ba = (np.asarray(v, np.int64) for v in offsets)
    counts = np.asarray(counts, np.int64)
    classes = [str(c) for c in classes]
    if counts.ndim != 3 or counts.shape[1:] != (len(classes), 3):
        raise ValueError(f'counts {counts.shape} must be [N, {len(classes)}, 3]')
    n, p = counts.shape[:2]
    if o_ab.shape != (n * p + 1,) or o_ba.shape != (n * p + 1,) or o_ab[-1] != d_ab.size or o_ba[-1] != d_ba.size:
        raise ValueError('offsets must be [N * P + 1] and end at the length of their list')
    if ratio is not None and not float(ratio) > 0:
        raise ValueError(f'ratio must be positive, got {ratio}')
    scale = 1.0 if ratio is None else 1.0 / float(ratio)
    keys = ('slice', 'n_pred', 'n_truth', 'hd', 'hd95', 'assd', 'dice', 'iou')
    out = {name: {k: [] for k in keys} for name in classes}
    for i in range(n):
        for k, name in enumerate(classes):
            s = i * p + k
            a = np.sqrt(d_ab[o_ab[s]:o_ab[s + 1]].astype(np.float64))
            b = np.sqrt(d_ba[o_ba[s]:o_ba[s + 1]].astype(np.float64))
            col = out[name]
            col['slice'].append(i)
            col['n_pred'].append(int(a.size))
            col['n_truth'].append(int(b.size))
            if a.size and b.size:
                col['hd'].append(float(max(a.max(), b.max()) * scale))
                col['hd95'].append(float(max(np.percentile(a, percentile), np.percentile(b, percentile)) * scale))
                col['assd'].append(float((a.sum() + b.sum()) / (a.size + b.size) * scale))
            else:
                col['hd'].append(None)
                col['hd95'].append(None)
                col['assd'].append(None)
            inter, na, nb = (int(v) for v in counts[i, k])
            col['dice'].append(2.0 * inter / (na + nb) if na + nb else 1.0)
            col['iou'].append(inter / (na + nb - inter) if na + nb - inter else 1.0)
    return out


def _surface_lists(pred, truth, pairs, scratch_bytes=DEFAULT_SCRATCH):
    """``(d2, offsets, counts)`` for ``build_surface_metrics``: the two directed boundary lists and the overlap counts."""
    d_ab, o_ab, _, overlap = _lists(pred, truth, pairs, 'boundary', 'boundary', scratch_bytes)
    d_ba, o_ba, _, _ = _lists(truth, pred, pairs, 'boundary', 'boundary', scratch_bytes)
    return (d_ab, d_ba), (o_ab, o_ba), overlap


def surface_metrics(pred, truth, classes=None, ratio=None, percentile=95, scratch_bytes=DEFAULT_SCRATCH):
    """Boundary agreement of two mask stacks per class and slice: ``hd``, ``hd95``, ``assd`` (module docstring) next to ``dice`` and ``iou``.
    ``pred`` / ``truth`` float32 CUDA [N, H, W, channels]; ``classes``: None = the pipeline's layout (channel ``CLASS_IDS[name] - 1``), or the
    names of the channels in order.  Returns the dict of ``build_surface_metrics``."""
    sc, sc2 = _check(pred)[4], _check(truth)[4]
    if sc != sc2:
        raise ValueError(f'pred and truth must have equal channels, got {sc} and {sc2}')
    names = _names(classes, sc)
    d2, offsets, counts = _surface_lists(pred, truth, [(ch, ch) for ch, _ in names], scratch_bytes)
    return build_surface_metrics(d2, offsets, counts, [name for _, name in names], ratio=ratio, percentile=percentile)


def build_cap_distance(keys, w, ratio=None):
    """``cap_distance``'s dict from the packed minima (uint64 [N], ``d2 << 32 | y * W + x``; all ones = no lipid pixel, ``d2 == DIST_NONE`` = no
    lumen pixel).  Pure host."""
    keys = np.asarray(keys).astype(np.uint64).reshape(-1)
    if ratio is not None and not float(ratio) > 0:
        raise ValueError(f'ratio must be positive, got {ratio}')
    scale = 1.0 if ratio is None else 1.0 / float(ratio)
    out = {'slice': [], 'distance': [], 'at': [], 'd2': []}
    for i, k in enumerate(keys.tolist()):
        d2, pix = k >> 32, k & 0xffffffff
        if k == 2 ** 64 - 1 or d2 == DIST_NONE:
            continue
        out['slice'].append(i)
        out['distance'].append(float(np.sqrt(np.float64(d2)) * scale))
        out['at'].append((int(pix // w), int(pix % w)))
        out['d2'].append(int(d2))
    return out


def pair_minimum(src, dst, pairs=None, src_part='set', dst_part='set', scratch_bytes=DEFAULT_SCRATCH):
    """uint64 numpy [N, P]: per slice and pair the minimum over the source part's pixels of ``d2 << 32 | (y * W + x)`` -- the smallest squared
    distance to the target part and, among the pixels that attain it, the first in raster order; all ones without a source pixel."""
    sp, dp = _part(src_part, 'src_part'), _part(dst_part, 'dst_part')
    src, dst, pairs, n, h, w, ca, cb = _check_pair(src, dst, pairs)
    npairs = len(pairs)
    with torch.cuda.device(src.device):
        pairs_dev = torch.tensor(pairs, dtype=torch.int32, device=src.device).reshape(npairs, 2)
        out = torch.empty((n, npairs), dtype=torch.int64, device=src.device)
        step, scratch, nbytes = _chunk(n, h, w, ca, cb, npairs, scratch_bytes, src.device)
        for i in range(0, n, step):
            m = min(step, n - i)
            L.check(L.lib().octseg_pair_distance_min(L.ptr(src[i:i + m]), L.ptr(dst[i:i + m]), m, h, w, ca, cb, L.ptr(pairs_dev), npairs, sp, dp,
                                                     L.ptr(scratch), nbytes, L.ptr(out[i:i + m]), L.stream_ptr()))
    return out.cpu().numpy().view(np.uint64)


def cap_distance(stack, classes=None, lumen='Lumen', lipid='Lipid core', ratio=None, scratch_bytes=DEFAULT_SCRATCH):
    """The shortest distance from a lipid-core pixel to a lumen pixel per slice -- the cap thickness that needs no centre and no rays
    (``polar.plaque_report`` walks A-lines from the frame centre and crosses the cap obliquely when the catheter sits off the lumen's centre).
    ``classes`` as in ``surface_metrics``.  Returns ``{'slice', 'distance', 'at', 'd2'}``, lists over the slices that hold BOTH classes:
    ``distance`` = sqrt(d2) pixel centre to pixel centre (touching masks: 1), divided by ``ratio`` when given; ``at`` = ``(y, x)`` of the lipid
    pixel that attains it, the first in raster order; ``d2`` the squared distance in pixels."""
    channels = int(_check(stack)[4])
    by_name = {name: ch for ch, name in _names(classes, channels)}
    for name in (lumen, lipid):
        if name not in by_name:
            raise ValueError(f'class {name!r} has no channel in a stack of {channels} (known: {sorted(by_name)})')
    keys = pair_minimum(stack, stack, [(by_name[lipid], by_name[lumen])], 'set', 'set', scratch_bytes)
    return build_cap_distance(keys[:, 0], int(stack.shape[2]), ratio=ratio)


# ---- the same over the volume the slices form
MAX_SPAN = 32767
MAX_VOXELS = 2 ** 32


def check_slice_step(slice_step, n):
    """``slice_step`` as an int, or ``ValueError``: only integers >= 1 are taken (rational spacing is out of scope), and ``slice_step * (N - 1)``
    may not exceed 32767, so that a squared distance stays below 2^30 + 2^25 and so below ``DIST_NONE``."""
    if isinstance(slice_step, bool) or not isinstance(slice_step, (int, np.integer)):
        raise ValueError(f'slice_step must be an integer number of pixels, got {slice_step!r}')
    s = int(slice_step)
    if s < 1:
        raise ValueError(f'slice_step must be at least 1, got {s}')
    if s * (int(n) - 1) > MAX_SPAN:
        raise ValueError(f'slice_step {s} over {int(n)} slices: slice_step * (N - 1) must stay within {MAX_SPAN} (squared distances in int32)')
    return s


def check_volume(n, h, w):
    """``N * H * W <= 2^32``: the packed minimum carries the voxel index in 32 bits."""
    if int(n) * int(h) * int(w) > MAX_VOXELS:
        raise ValueError(f'volume {n} x {h} x {w}: at most 2^32 voxels (the packed minimum holds the voxel index in 32 bits)')


def volume_bands(n, h, w, channels_a, channels_b=0, pairs=0, scratch_bytes=DEFAULT_SCRATCH):
    """``(rows, bands, bytes)``: the rows of a band of the volume calls under the budget -- the most that fit, as the library itself chooses
    for a scratch of ``bytes`` --, the number of bands that makes, and the scratch to allocate.  ``ValueError`` naming the bytes needed when a
    band of one row does not fit."""
    need = lambda rows: int(L.lib().octseg_volume_distance_scratch_bytes(n, h, w, channels_a, channels_b, pairs, rows))
    one = need(1)
    if one == 0:
        raise ValueError(f'the volume calls refuse {n} x {h} x {w} with {channels_a} / {channels_b} channels and {pairs} pairs')
    if int(scratch_bytes) < one:
        raise ValueError(f'scratch_bytes {int(scratch_bytes)} is below the {one} bytes a band of one row needs')
    lo, hi = 1, h
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        if need(mid) <= int(scratch_bytes):
            lo = mid
        else:
            hi = mid - 1
    return lo, -(-h // lo), need(lo)


def _flat_scratch(n, h, w, ca, cb, pairs, device, scratch_bytes):
    """The scratch of the calls that take no distance map: the bit planes of the whole volume, which cannot be banded."""
    nbytes = int(L.lib().octseg_volume_distance_scratch_bytes(n, h, w, ca, cb, pairs, 0))
    if int(scratch_bytes) < nbytes:
        raise ValueError(f'scratch_bytes {int(scratch_bytes)} is below the {nbytes} bytes the bit planes of the volume need')
    return torch.empty((nbytes,), dtype=torch.uint8, device=device), nbytes


def boundary_volume(stack, scratch_bytes=DEFAULT_SCRATCH):
    """The 3-D boundary of every channel's volume: ``m & ~erode(m)`` with the 6-neighbour cross, everything outside the volume clear
    (``m & ~scipy.ndimage.binary_erosion(m, generate_binary_structure(3, 1), border_value=0)`` per channel), float32 0.0 / 1.0 in the input's
    layout.  Every set voxel of the first and of the last slice is boundary; with N <= 2 every set voxel is.  The input is not modified.  The
    scratch is the bit planes of the whole volume (1/4 byte per voxel and channel): a ``scratch_bytes`` below that raises and names the need."""
    stack, n, h, w, sc = _check(stack)
    check_volume(n, h, w)
    out = torch.empty_like(stack)
    with torch.cuda.device(stack.device):
        scratch, nbytes = _flat_scratch(n, h, w, sc, 0, 0, stack.device, scratch_bytes)
        L.check(L.lib().octseg_volume_boundary(L.ptr(stack), n, h, w, sc, L.ptr(scratch), nbytes, L.ptr(out), L.stream_ptr()))
    return out


def distance_volume(stack, to='set', slice_step=1, scratch_bytes=DEFAULT_SCRATCH):
    """int32 CUDA [N, channels, H, W]: the SQUARED distance ``(slice_step * dz)^2 + dy^2 + dx^2`` of every voxel to the nearest voxel of its own
    channel's ``to`` part over the WHOLE volume -- ``'set'``, ``'clear'`` or the 3-D ``'boundary'`` of ``boundary_volume`` --
    (``rint(distance_transform_edt(~T, sampling=(slice_step, 1, 1)) ** 2)``); ``DIST_NONE`` everywhere in a channel whose part is empty in the
    whole volume.  ``slice_step``: the distance between neighbouring slices in pixels, an integer >= 1.  The per-slice map is held for a band of
    rows of all slices at a time under ``scratch_bytes`` (``volume_bands``); the result does not depend on the banding."""
    to = _part(to, 'to')
    check_slice_step(slice_step, 1)
    stack, n, h, w, sc = _check(stack)
    check_volume(n, h, w)
    s = check_slice_step(slice_step, n)
    out = torch.empty((n, sc, h, w), dtype=torch.int32, device=stack.device)
    with torch.cuda.device(stack.device):
        nbytes = volume_bands(n, h, w, sc, 0, 0, scratch_bytes)[2]
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=stack.device)
        L.check(L.lib().octseg_volume_distance(L.ptr(stack), n, h, w, sc, to, s, L.ptr(scratch), nbytes, L.ptr(out), L.stream_ptr()))
    return out


def _shape4(stack):
    """The four extents of a stack before anything is asked of the device, so that the refusals that need no GPU come first."""
    shape = tuple(getattr(stack, 'shape', ()))
    if len(shape) != 4:
        raise ValueError('stack must be a float32 CUDA tensor [N, H, W, channels]')
    return tuple(int(v) for v in shape)


def _check_volume_pair(src, dst, pairs, slice_step):
    check_slice_step(slice_step, 1)
    a, b = _shape4(src), _shape4(dst)
    if a[:3] != b[:3]:
        raise ValueError(f'the two stacks must agree in slices, frame size and device, got {a} and {b}')
    src, dst, pairs, n, h, w, ca, cb = _check_pair(src, dst, pairs)
    check_volume(n, h, w)
    return src, dst, pairs, (n, h, w, ca, cb), check_slice_step(slice_step, n)


def _fill_keys_volume(src, dst, pairs_dev, npairs, sp, dp, s, dims, offsets_dev, keys, capacity, scratch_bytes):
    """The second launch of ``directed_distances_volume``: one key per query voxel into ``keys[:capacity]``; a key past the capacity is dropped
    on the device and turns into a ``RuntimeError`` here."""
    n, h, w, ca, cb = dims
    overflow = torch.zeros((1,), dtype=torch.int32, device=src.device)
    nbytes = volume_bands(n, h, w, ca, cb, npairs, scratch_bytes)[2]
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=src.device)
    L.check(L.lib().octseg_volume_pair_distance_keys(L.ptr(src), L.ptr(dst), n, h, w, ca, cb, L.ptr(pairs_dev), npairs, sp, dp, s, L.ptr(scratch), nbytes,
                                                     0, L.ptr(offsets_dev), L.ptr(keys), int(capacity), L.ptr(overflow), L.stream_ptr()))
    if int(overflow.item()):
        raise RuntimeError(f'directed_distances_volume: the key buffer of {int(capacity)} entries is too small for the query voxels; keys were dropped')


def _lists_volume(src, dst, pairs, src_part, dst_part, slice_step, scratch_bytes):
    """``(d2, offsets, target_count, overlap)`` as numpy: see ``directed_distances_volume``; ``overlap`` int64 [P, 3] = |a & b|, |a|, |b|."""
    sp, dp = _part(src_part, 'src_part'), _part(dst_part, 'dst_part')
    src, dst, pairs, dims, s = _check_volume_pair(src, dst, pairs, slice_step)
    n, h, w, ca, cb = dims
    npairs = len(pairs)
    with torch.cuda.device(src.device):
        pairs_dev = torch.tensor(pairs, dtype=torch.int32, device=src.device).reshape(npairs, 2)
        both = torch.empty((npairs * 5,), dtype=torch.int64, device=src.device)
        scratch, nbytes = _flat_scratch(n, h, w, ca, cb, npairs, src.device, scratch_bytes)
        L.check(L.lib().octseg_volume_pair_distance_counts(L.ptr(src), L.ptr(dst), n, h, w, ca, cb, L.ptr(pairs_dev), npairs, sp, dp, L.ptr(scratch), nbytes,
                                                           L.ptr(both), L.ptr(both[npairs * 2:]), L.stream_ptr()))
        del scratch
        host = both.cpu().numpy()                                              # the one synchronisation: the offsets need the counts
        counts, overlap = host[:npairs * 2].reshape(npairs, 2), host[npairs * 2:].reshape(npairs, 3)
        offsets = np.zeros((npairs + 1,), np.int64)
        np.cumsum(counts[:, 0], out=offsets[1:])
        total = int(offsets[-1])
        if total:
            keys = torch.empty((total,), dtype=torch.int64, device=src.device)
            _fill_keys_volume(src, dst, pairs_dev, npairs, sp, dp, s, dims, torch.from_numpy(offsets[:-1].copy()).to(src.device), keys, total,
                              scratch_bytes)
            keys = torch.sort(keys).values
            seg = (keys >> 32).cpu().numpy()
            d2 = (keys & 0xffffffff).cpu().numpy()
            if not np.array_equal(np.bincount(seg, minlength=npairs), np.diff(offsets)):
                raise RuntimeError('directed_distances_volume: the keys written do not match the counted query voxels')
        else:
            d2 = np.zeros((0,), np.int64)
    return d2, offsets, counts[:, 1].copy(), overlap.copy()


def directed_distances_volume(src, dst, pairs=None, src_part='boundary', dst_part='boundary', slice_step=1, scratch_bytes=DEFAULT_SCRATCH):
    """``directed_distances`` over the volume: for every ``(src channel, dst channel)`` of ``pairs`` (default: equal channels), the SQUARED
    distance ``(slice_step * dz)^2 + dy^2 + dx^2`` from each voxel of the source channel's ``src_part`` to the nearest voxel of the target
    channel's ``dst_part`` anywhere in the volume (parts: the 3-D ``'boundary'``, ``'set'``, ``'clear'``).  Returns ``(d2, offsets,
    target_count)``: ``d2`` int64 numpy, pair p's values are ``d2[offsets[p]:offsets[p + 1]]`` in ascending order; ``offsets`` int64 [P + 1];
    ``target_count`` int64 [P], the target voxels.  Where the target part is empty in the whole volume the values are ``DIST_NONE``."""
    return _lists_volume(src, dst, pairs, src_part, dst_part, slice_step, scratch_bytes)[:3]


def build_volume_surface_metrics(d2, offsets, counts, classes, ratio=None, percentile=95):
    """The report of ``volume_surface_metrics`` from the integers.  Pure host, float64 numpy.  ``d2`` = ``(pred -> truth, truth -> pred)``, each
    the sorted squared distances of ``directed_distances_volume``; ``offsets`` = their two offset arrays [P + 1]; ``counts`` int [P, 3] =
    |pred & truth|, |pred|, |truth| set voxels; ``classes`` the P names.  Returns ``{name: {'n_pred', 'n_truth', 'hd', 'hd95', 'assd',
    'dice', 'iou'}}``, one scalar each: the definitions are those of ``build_surface_metrics`` (it is what computes them, on the volume as
    its one slice), taken over the volume's boundary voxels; the three distances are ``None`` when either side has no voxel."""
    counts = np.asarray(counts, np.int64)
    if counts.ndim != 2:
        raise ValueError(f'counts {counts.shape} must be [P, 3]')
    per_slice = build_surface_metrics(d2, offsets, counts[None], classes, ratio=ratio, percentile=percentile)
    return {name: {k: v[0] for k, v in col.items() if k != 'slice'} for name, col in per_slice.items()}


def _volume_surface_lists(pred, truth, pairs, slice_step=1, scratch_bytes=DEFAULT_SCRATCH):
    """``(d2, offsets, counts)`` for ``build_volume_surface_metrics``: the two directed boundary lists and the overlap counts."""
    d_ab, o_ab, _, overlap = _lists_volume(pred, truth, pairs, 'boundary', 'boundary', slice_step, scratch_bytes)
    d_ba, o_ba, _, _ = _lists_volume(truth, pred, pairs, 'boundary', 'boundary', slice_step, scratch_bytes)
    return (d_ab, d_ba), (o_ab, o_ba), overlap


def volume_surface_metrics(pred, truth, classes=None, slice_step=1, ratio=None, percentile=95, scratch_bytes=DEFAULT_SCRATCH):
    """Surface agreement of two mask volumes per class: the volumetric ``hd``, ``hd95``, ``assd`` over the 3-D boundary voxels next to ``dice`` and
    ``iou`` of the whole volume.  A lesion predicted one slice early or late is ``slice_step`` off here, where ``surface_metrics`` has ``None``
    on the slices only one side holds.  ``pred`` / ``truth`` float32 CUDA [N, H, W, channels]; ``classes`` as in ``surface_metrics``;
    ``slice_step`` the distance between slices in pixels (an integer).  Returns the dict of ``build_volume_surface_metrics``."""
    check_slice_step(slice_step, 1)
    sc, sc2 = _shape4(pred)[3], _shape4(truth)[3]
    if sc != sc2:
        raise ValueError(f'pred and truth must have equal channels, got {sc} and {sc2}')
    names = _names(classes, sc)
    d2, offsets, counts = _volume_surface_lists(pred, truth, [(ch, ch) for ch, _ in names], slice_step, scratch_bytes)
    return build_volume_surface_metrics(d2, offsets, counts, [name for _, name in names], ratio=ratio, percentile=percentile)


def pair_minimum_volume(src, dst, pairs=None, src_part='set', dst_part='set', slice_step=1, scratch_bytes=DEFAULT_SCRATCH):
    """uint64 numpy [P]: per pair the minimum over the source part's voxels of ``d2 << 32 | (z * H * W + y * W + x)`` -- the smallest squared
    distance to the target part anywhere in the volume and, among the voxels that attain it, the first in raster order; all ones without a
    source voxel, ``d2 == DIST_NONE`` without a target voxel."""
    sp, dp = _part(src_part, 'src_part'), _part(dst_part, 'dst_part')
    src, dst, pairs, (n, h, w, ca, cb), s = _check_volume_pair(src, dst, pairs, slice_step)
    npairs = len(pairs)
    with torch.cuda.device(src.device):
        pairs_dev = torch.tensor(pairs, dtype=torch.int32, device=src.device).reshape(npairs, 2)
        out = torch.empty((npairs,), dtype=torch.int64, device=src.device)
        nbytes = volume_bands(n, h, w, ca, cb, npairs, scratch_bytes)[2]
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=src.device)
        L.check(L.lib().octseg_volume_pair_distance_min(L.ptr(src), L.ptr(dst), n, h, w, ca, cb, L.ptr(pairs_dev), npairs, sp, dp, s, L.ptr(scratch), nbytes,
                                                        L.ptr(out), L.stream_ptr()))
    return out.cpu().numpy().view(np.uint64)


def build_cap_distance_volume(key, h, w, ratio=None):
    """``cap_distance_volume``'s dict from the packed minimum (``d2 << 32 | z * H * W + y * W + x``), ``None`` when it is all ones (no lipid
    voxel) or its ``d2`` is ``DIST_NONE`` (no lumen voxel).  Pure host."""
    if ratio is not None and not float(ratio) > 0:
        raise ValueError(f'ratio must be positive, got {ratio}')
    k = int(key)
    d2, vox = k >> 32, k & 0xffffffff
    if k == 2 ** 64 - 1 or d2 == DIST_NONE:
        return None
    scale = 1.0 if ratio is None else 1.0 / float(ratio)
    return {'distance': float(np.sqrt(np.float64(d2)) * scale), 'at': (vox // (h * w), vox % (h * w) // w, vox % w), 'd2': d2}


def cap_distance_volume(stack, classes=None, lumen='Lumen', lipid='Lipid core', slice_step=1, ratio=None, scratch_bytes=DEFAULT_SCRATCH):
    """The shortest distance from a lipid-core voxel to a lumen voxel anywhere in the volume: the thinnest piece of cap need not lie inside one
    frame, and ``cap_distance`` overestimates it whenever the nearest lumen voxel is in a neighbouring frame.  Returns ``{'distance', 'at',
    'd2'}`` -- ``distance`` = sqrt(d2) voxel centre to voxel centre, divided by ``ratio`` when given; ``at`` = ``(z, y, x)`` of the lipid voxel
    that attains it, the first in raster order; ``d2`` the squared distance in pixels -- or ``None`` when either class is absent from the
    volume.  ``classes`` as in ``surface_metrics``."""
    n, h, w, channels = _shape4(stack)
    by_name = {name: ch for ch, name in _names(classes, channels)}
    for name in (lumen, lipid):
        if name not in by_name:
            raise ValueError(f'class {name!r} has no channel in a stack of {channels} (known: {sorted(by_name)})')
    keys = pair_minimum_volume(stack, stack, [(by_name[lipid], by_name[lumen])], 'set', 'set', slice_step, scratch_bytes)
    return build_cap_distance_volume(keys[0], h, w, ratio=ratio)


def read_mask_dirs(pred_dir, truth_dir):
    """The mask TIFFs both folders hold under the same file name, as ``(names, pred, truth)``: uint8-valued numpy stacks [N, H, W, channels]
    (``dataset.read_mask_tiff``; a 2-D mask is one channel).  All masks must share one shape."""
    from .dataset import read_mask_tiff

    def listing(d):
        return {os.path.basename(p): p for ext in ('*.tiff', '*.tif') for p in glob(os.path.join(d, ext))}
    a, b = listing(pred_dir), listing(truth_dir)
    names = sorted(set(a) & set(b))
    if not names:
        raise ValueError(f'no mask TIFF of the same name in {pred_dir} and {truth_dir}')

    def load(p):
        m = np.asarray(read_mask_tiff(p))
        return m[:, :, None] if m.ndim == 2 else m
    pred, truth = [load(a[k]) for k in names], [load(b[k]) for k in names]
    shapes = {m.shape for m in pred + truth}
    if len(shapes) != 1:
        raise ValueError(f'the masks must share one shape, got {sorted(shapes)}')
    return names, np.stack(pred), np.stack(truth)


def _host_surface_lists(pred, truth, pairs):
    """``_surface_lists`` for numpy stacks: one upload each."""
    dev = torch.device('cuda')
    up = [torch.from_numpy(np.ascontiguousarray(np.asarray(v) != 0).astype(np.float32)).to(dev) for v in (pred, truth)]
    return _surface_lists(up[0], up[1], pairs)


def _host_volume_surface_lists(pred, truth, pairs, slice_step):
    """``_volume_surface_lists`` for numpy stacks: one upload each."""
    dev = torch.device('cuda')
    up = [torch.from_numpy(np.ascontiguousarray(np.asarray(v) != 0).astype(np.float32)).to(dev) for v in (pred, truth)]
    return _volume_surface_lists(up[0], up[1], pairs, slice_step)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    usage = 'usage: python -m oct_segmentation_amd.distance pred_dir truth_dir [save_dir] [slice_step=K]'
    step = [a for a in argv if a.startswith('slice_step=')]
    argv = [a for a in argv if not a.startswith('slice_step=')]
    if len(argv) not in (2, 3) or len(step) > 1:
        raise SystemExit(usage)
    if step:
        try:
            step = [int(step[0].split('=', 1)[1])]
        except ValueError:
            raise SystemExit(f'slice_step must be an integer number of pixels, got {step[0]!r}')
    pred_dir, truth_dir = argv[:2]
    save_dir = argv[2] if len(argv) == 3 else pred_dir
    names, pred, truth = read_mask_dirs(pred_dir, truth_dir)
    n, h, w, sc = pred.shape
    check_extents(n, h, w, sc)
    if step:
        check_volume(n, h, w)
        check_slice_step(step[0], n)
    classes = _names(None, sc)
    pairs, cnames = [(ch, ch) for ch, _ in classes], [name for _, name in classes]
    d2, offsets, counts = _host_surface_lists(pred, truth, pairs)
    report = {'images': names, 'classes': cnames, 'percentile': 95, 'unit': 'pixel',
              'metrics': build_surface_metrics(d2, offsets, counts, cnames)}
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, 'surface_metrics.json')
    with open(path, 'w') as f:
        json.dump(report, f, indent=1)
    print(path)
    if step:                                                 # the files in sorted-name order are the slices of the volume
        d2, offsets, counts = _host_volume_surface_lists(pred, truth, pairs, step[0])
        volume = {'images': names, 'classes': cnames, 'percentile': 95, 'unit': 'pixel', 'slice_step': step[0],
                  'metrics': build_volume_surface_metrics(d2, offsets, counts, cnames)}
        path = os.path.join(save_dir, 'surface_metrics_3d.json')
        with open(path, 'w') as f:
            json.dump(volume, f, indent=1)
        print(path)
    return report


if __name__ == '__main__':
    main()
