"""Per-pullback measurements on the GPU -- what the reference's app computes segmentations FOR: host mirror of ``get_analysis``
(``src/app/tools/analysis.py:133-250``) and of its ray walker ``calculate_object_thickness`` (``analysis.py:60-130``).

For every class the app's dict lists the slices where the class is present, the area per slice, the grouping of consecutive slices into
numbered objects and a thickness per slice; its plots are drawn from exactly that dict, and upstream leaves the model call in that function
as ``TODO: inference``.  Here the mask stack is already on the device (``predict.segment_stack``): one call (``octseg_stack_measure``,
``csrc/measure.hip``) counts the set pixels per slice and class and walks the 360 rays per slice and class; about 6 KB per slice come back
and the rest is a few integers per slice on the host.

    counts, radii = measure_stack(stack)                       # int32 CUDA [N, 4], [N, 4, 360]; stack float32 CUDA [N, H, W, 4]
    data = analyze_stack(stack, image_names)                   # the app's dict: {'ratio', 'objects': {class: {...}}, 'images'}
"""
import base64
import math
from io import BytesIO

import numpy as np
import torch

from . import _lib as L
from .model import CLASS_IDS

ANGLES = 360
MAX_CHANNELS = 16

_consts = {}   # (h, w, device) -> (ray_pix, ray_len) device tensors


def ray_table(h, w):
    """The samples of ``calculate_object_thickness`` (analysis.py:74-76,81-107) for an ``h`` x ``w`` mask as tables: ``ray_pix`` int32
    [360, R], the linear pixel index ``y * w + x`` of step ``r = 1 .. R`` at every whole degree, and ``ray_len`` int32 [360], the number of
    leading steps inside the frame (the walk stops at the first step outside).  ``R = max(max_radius - 1, 0)`` with upstream's
    ``max_radius = int(sqrt(w ** 2 + h ** 2)) // 2``.  The arithmetic is Python's ``math`` and ``int()`` exactly as upstream writes it --
    truncation toward zero, so a coordinate in (-1, 0) becomes 0 and is inside the frame.  Entries past ``ray_len`` are 0 and never read."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f'frame size must be positive, got {h} x {w}')
    cx, cy = w // 2, h // 2
    max_radius = int(math.sqrt(w ** 2 + h ** 2)) // 2
    R = max(max_radius - 1, 0)
    pix = np.zeros((ANGLES, R), np.int32)
    length = np.zeros((ANGLES,), np.int32)
    for angle in range(ANGLES):
        rad = math.radians(angle)
        c, s = math.cos(rad), math.sin(rad)
        n = 0
        for r in range(1, max_radius):
            x = int(cx + r * c)
            y = int(cy + r * s)
            if not (0 <= x < w and 0 <= y < h):
                break
            pix[angle, n] = y * w + x
            n += 1
        length[angle] = n
    return pix, length


def _ray_table_dev(h, w, device):
    key = (int(h), int(w), str(device))
    if key not in _consts:
        pix, length = ray_table(h, w)
        _consts[key] = (torch.from_numpy(pix).to(device), torch.from_numpy(length).to(device))
    return _consts[key]


def measure_stack(stack):
    """``stack`` float32 CUDA [N, H, W, channels] (any value != 0 is set).  Returns ``(counts, radii)``: int32 CUDA [N, channels], the set
    pixels per slice and channel, and int32 CUDA [N, channels, 360], per degree the radius ``calculate_object_thickness`` appends for that
    ray, or 0 where it appends none (its radii are >= 1).  One call, no host synchronisation."""
    if not (torch.is_tensor(stack) and stack.is_cuda and stack.dtype == torch.float32 and stack.dim() == 4):
        raise ValueError('stack must be a float32 CUDA tensor [N, H, W, channels]')
    if 0 in stack.shape:
        raise ValueError('empty batch or frame')
    n, h, w, sc = (int(v) for v in stack.shape)
    if sc > MAX_CHANNELS:
        raise ValueError(f'at most {MAX_CHANNELS} channels, got {sc}')
    if h * w >= 2 ** 31:
        raise ValueError(f'frame {h} x {w} has 2^31 pixels or more')
    stack = stack.contiguous()
    pix, length = _ray_table_dev(h, w, stack.device)
    counts = torch.empty((n, sc), dtype=torch.int32, device=stack.device)
    radii = torch.empty((n, sc, ANGLES), dtype=torch.int32, device=stack.device)
    with torch.cuda.device(stack.device):
        L.check(L.lib().octseg_stack_measure(L.ptr(stack), n, h, w, sc, L.ptr(pix) if pix.numel() else None, L.ptr(length), int(pix.shape[1]),
                                             L.ptr(counts), L.ptr(radii), L.stream_ptr()))
    return counts, radii


def radial_thickness(radii_row):
    """The dict ``calculate_object_thickness`` returns (analysis.py:112-130) from one row of ``radii``: the measurements are the non-zero
    radii in angle order; ``median`` is numpy's (a float), ``min`` / ``max`` ints; the all-zero dict when no ray met the object."""
    row = np.asarray(radii_row).reshape(-1)
    meas = [int(v) for v in row if v != 0]
    if not meas:
        return {'median': 0, 'min': 0, 'max': 0, 'all_measurements': []}
    return {'median': float(np.median(meas)), 'min': int(min(meas)), 'max': int(max(meas)), 'all_measurements': meas}


def _mask_png_b64(mask_u8):
    from PIL import Image
    buff = BytesIO()
    Image.fromarray(mask_u8).save(buff, format='png')
    return base64.b64encode(buff.getvalue()).decode('utf-8')


def build_analysis(counts, radii, h, w, image_names, ratio=None, masks=None):
    """analysis.py:143-161,185-213 from the integers: ``counts`` [N, channels] and ``radii`` [N, channels, 360] (numpy or anything
    ``np.asarray`` takes), the frame size and one name per slice.  Pure host.

    ``ratio`` defaults to ``int(h * 150 // 1000)`` (upstream's ``dcm.shape[1]``).  For every class of ``CLASS_IDS`` in id order and every
    slice in order the class is present iff ``0 < count < h * w`` -- upstream's ``np.unique(...).shape[0] == 2``: a completely FULL mask
    counts as absent, and that quirk is kept.  A present slice appends ``slice``, ``area = pow(count // ratio, 0.5)``, ``object_id`` (first
    0; the same id if this slice is the previous present slice + 1, else the previous id + 1), ``thickness_mean = median / ratio``,
    ``thickness_min = min / ratio``, ``thickness_max = max / ratio`` (not in upstream's dict) of ``radial_thickness`` and ``img_name``.
    ``masks``: optional callable ``(slice, channel) -> str`` filling upstream's ``masks`` lists; without it they stay empty.
    Values are plain Python floats and ints: the dict goes through ``json.dump``."""
    counts, radii = np.asarray(counts), np.asarray(radii)
    h, w = int(h), int(w)
    if counts.ndim != 2 or radii.shape != counts.shape + (ANGLES,):
        raise ValueError(f'counts {counts.shape} and radii {radii.shape} must be [N, channels] and [N, channels, {ANGLES}]')
    image_names = [str(s) for s in image_names]
    if len(image_names) != counts.shape[0]:
        raise ValueError(f'{len(image_names)} names for {counts.shape[0]} slices')
    ratio = int(h * 150 // 1000) if ratio is None else int(ratio)
    if ratio < 1:
        raise ValueError(f'ratio must be at least 1, got {ratio} (the default int(h * 150 // 1000) is 0 for frames below 7 rows)')
    keys = ('area', 'thickness_mean', 'thickness_min', 'thickness_max', 'slice', 'object_id', 'masks', 'img_name')
    objects = {name: {k: [] for k in keys} for name in CLASS_IDS}
    data = {'ratio': ratio, 'objects': objects, 'images': []}
    by_id = sorted((cid, name) for name, cid in CLASS_IDS.items())
    for idx, img_name in enumerate(image_names):
        for cid, name in by_id:
            ch = cid - 1
            if ch >= counts.shape[1]:
                continue
            count = int(counts[idx, ch])
            if not 0 < count < h * w:
                continue
            obj = objects[name]
            if not obj['object_id']:
                obj['object_id'].append(0)
            elif idx == obj['slice'][-1] + 1:
                obj['object_id'].append(obj['object_id'][-1])
            else:
                obj['object_id'].append(obj['object_id'][-1] + 1)
            obj['slice'].append(idx)
            obj['area'].append(float(pow(count // ratio, 0.5)))
            t = radial_thickness(radii[idx, ch])
            obj['thickness_mean'].append(float(t['median'] / ratio))
            obj['thickness_min'].append(float(t['min'] / ratio))
            obj['thickness_max'].append(float(t['max'] / ratio))
            if masks is not None:
                obj['masks'].append(masks(idx, ch))
            obj['img_name'].append(img_name)
        data['images'].append(img_name)
    return data


def analyze_stack(stack, image_names=None, ratio=None, thickness='radial', with_masks=False, clean=None, with_contours=False):
    """The app's ``get_analysis`` dict for a mask stack on the device.  NOTE: ``thickness_mean`` / ``thickness_min`` carry the median / min of
    upstream's RADIAL thickness function, ``calculate_object_thickness`` -- not of ``calculate_thickness_contour``, the call ``get_analysis``
    actually makes (analysis.py:202-207), whose result depends on ``cv2.findContours``' border-following order and vertex compression and has
    no independent implementation here to be held to.  ``thickness='contour'`` raises ``NotImplementedError``.

    ``stack`` float32 CUDA [N, H, W, channels]; ``image_names`` one per slice (default ``'0', '1', ...``), the slices in pullback order.
    Runs ``measure_stack``, makes ONE device-to-host copy of counts and radii (about 6 KB per slice) and calls ``build_analysis``.
    ``with_masks=True`` also fills upstream's ``masks`` lists (base64 PNG of the 0 / 255 uint8 mask, analysis.py:208-211), which copies the
    present masks to the host; the default leaves the lists empty and the masks on the device.
    ``clean``: None (default, the stack is measured as it is), True or a dict of ``cleanup.clean_stack`` keywords: the stack goes through
    ``clean_stack`` first (smoothing, keep-largest, hole fill) and the cleaned stack is what is measured and what ``with_masks`` encodes.
    ``with_contours=True`` adds a ``contours`` list beside every class's ``masks``: per present slice the polygons of the mask
    (``contours.Contours.polygons``: integer vertices on the pixel lattice, holes as ``interior`` rings), so that a viewer can draw outlines
    without decoding a PNG; the dict gains ``contour_convention``.  Off by default: every other key is unchanged."""
    if thickness == 'contour':
        raise NotImplementedError("thickness='contour' (calculate_thickness_contour) needs cv2.findContours / contourArea / moments: its "
                                  'result depends on OpenCV\'s border-following order, tie-breaking among equal areas and '
                                  'CHAIN_APPROX_SIMPLE vertex compression, and there is no independent implementation to hold a restatement '
                                  "to; use thickness='radial' (calculate_object_thickness)")
    if thickness != 'radial':
        raise ValueError(f"thickness must be 'radial' or 'contour', got {thickness!r}")
    from .cleanup import clean_kwargs, clean_stack
    kw = clean_kwargs(clean)
    if kw is not None:
        stack = clean_stack(stack, **kw)
    counts, radii = measure_stack(stack)
    n, h, w, sc = (int(v) for v in stack.shape)
    if image_names is None:
        image_names = [str(i) for i in range(n)]
    host = torch.cat([counts.reshape(n, sc, 1), radii], dim=2).cpu().numpy()
    masks = None
    if with_masks:
        def masks(idx, ch):
            return _mask_png_b64(((stack[idx, :, :, ch] != 0).to(torch.uint8) * 255).cpu().numpy())
    data = build_analysis(host[:, :, 0], host[:, :, 1:], h, w, image_names, ratio=ratio, masks=masks)
    if with_contours:
        from .contours import CONVENTION, trace_stack
        polys = trace_stack(stack).polygons()
        data['contour_convention'] = CONVENTION
        for name, cid in CLASS_IDS.items():
            obj = data['objects'][name]
            obj['contours'] = [polys[idx][cid - 1] for idx in obj['slice']]
    return data
