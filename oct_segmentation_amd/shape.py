"""Lumen geometry: what a reader of an intravascular OCT pullback asks first -- lumen area per frame, the smallest and largest lumen diameter
through the lumen's OWN centre of mass, eccentricity, the minimal-lumen-area (MLA) frame and the percent area stenosis against the reference
frames on either side.  No reference counterpart: ``analysis.measure_stack`` and ``polar.polar_profile`` walk their rays
from the frame centre, the A-lines of a catheter-centred frame, and the catheter is almost never at the lumen's centre.

Three device calls (``csrc/shape.hip``, rules in ``include/octseg.h``), everything integer and pinned exactly by ``tests/shape_ref.py``:

    mom = moments_stack(stack)                                 # int64 CUDA [N, C, 12]: M00 M10 M01 M20 M11 M02, box, crack perimeter
    org = origins(stack, mom, ref='Lumen')                     # int32 CUDA [N, C, 3]: the centroid as a pixel, and whether the plane is set there
    prof, length, org = centred_profile(stack, 'Lumen')        # polar.polar_profile's five integers per ray, walked from that pixel
    table = shape_table(mom)                                   # area, centroid, box, central moments, axes, orientation, perimeter, compactness
    report = lumen_report(stack, image_names)                  # per-frame lumen area and diameters, MLA, reference, area stenosis; json.dump-able

``stack`` is float32 CUDA [N, H, W, channels] (any value != 0 is set); nothing synchronises with the host before a report copies its integers.
"""
import math

import numpy as np
import torch

from . import _lib as L
from .analysis import ANGLES
from .model import CLASS_IDS
from .polar import FIELDS, IN, OUT

MOMENT_FIELDS = 12
M00, M10, M01, M20, M11, M02, XMIN, XMAX, YMIN, YMAX, EDGES = range(11)
MAX_CHANNELS = 16                      # moments_stack, origins
MAX_WALK_CHANNELS = 8                  # centred_profile, as polar.polar_profile
MAX_EXTENT = 32768                     # H and W; with MAX_PIXELS every int64 sum stays below MAX_PIXELS * (MAX_EXTENT - 1) ** 2 < 2 ** 61
MAX_PIXELS = 2 ** 31                   # H * W must stay below

_offsets = {}   # (h, w, device) -> ray_off device tensor


def _check_stack(stack, max_channels):
    if not (torch.is_tensor(stack) and stack.dtype == torch.float32 and stack.dim() == 4):
        raise ValueError('stack must be a float32 CUDA tensor [N, H, W, channels]')
    if 0 in stack.shape:
        raise ValueError('empty batch or frame')
    n, h, w, sc = (int(v) for v in stack.shape)
    if sc > max_channels:
        raise ValueError(f'at most {max_channels} channels, got {sc}')
    if h > MAX_EXTENT or w > MAX_EXTENT or h * w >= MAX_PIXELS:
        raise ValueError(f'frame {h} x {w}: at most {MAX_EXTENT} rows and columns and fewer than 2^31 pixels')
    if not stack.is_cuda:
        raise ValueError('stack must be a float32 CUDA tensor [N, H, W, channels]: it is on the host, and there is no CPU path')
    return n, h, w, sc


def _channel(ref, sc):
    """None -> -1 (own); a class name or a channel index -> the channel, checked against ``sc``."""
    if ref is None:
        return -1
    if isinstance(ref, str):
        if ref not in CLASS_IDS:
            raise ValueError(f'unknown class {ref!r}')
        ch = CLASS_IDS[ref] - 1
    else:
        ch = int(ref)
    if not 0 <= ch < sc:
        raise ValueError(f'reference {ref!r} is channel {ch} of a stack with {sc}')
    return ch


def moments_stack(stack):
    """``stack`` float32 CUDA [N, H, W, channels <= 16] -> int64 CUDA [N, channels, 12]: per plane M00, M10, M01, M20, M11, M02 over the set
    pixels (x the column, y the row), XMIN, XMAX, YMIN, YMAX (``W, -1, H, -1`` on an empty plane), EDGES (the crack perimeter: the sides of set
    pixels that face a clear pixel or the frame's border) and a zero.  ``octseg_stack_moments``: one streaming pass, no host synchronisation."""
    n, h, w, sc = _check_stack(stack, MAX_CHANNELS)
    stack = stack.contiguous()
    mom = torch.empty((n, sc, MOMENT_FIELDS), dtype=torch.int64, device=stack.device)
    with torch.cuda.device(stack.device):
        L.check(L.lib().octseg_stack_moments(L.ptr(stack), n, h, w, sc, L.ptr(mom), L.stream_ptr()))
    return mom


def origins(stack, mom, ref=None):
    """int32 CUDA [N, channels, 3] = x, y, AT: the centroid rounded to the nearest pixel, ``(2 * M10 + M00) // (2 * M00)`` and likewise y, of
    the plane's own moments (``ref=None``) or of the class / channel ``ref`` of the same slice for every channel; AT = 1 where THIS channel is
    set at that pixel; ``(-1, -1, 0)`` where the source plane is empty.  ``mom`` is ``moments_stack(stack)``.  One tiny launch."""
    n, h, w, sc = _check_stack(stack, MAX_CHANNELS)
    ch = _channel(ref, sc)
    if not (torch.is_tensor(mom) and mom.dtype == torch.int64 and tuple(mom.shape) == (n, sc, MOMENT_FIELDS) and mom.device == stack.device):
        raise ValueError(f'mom must be the int64 tensor [{n}, {sc}, {MOMENT_FIELDS}] of moments_stack on the stack\'s device')
    stack, mom = stack.contiguous(), mom.contiguous()
    out = torch.empty((n, sc, 3), dtype=torch.int32, device=stack.device)
    with torch.cuda.device(stack.device):
        L.check(L.lib().octseg_moment_origins(L.ptr(stack), L.ptr(mom), n, h, w, sc, ch, L.ptr(out), L.stream_ptr()))
    return out


def ray_offsets(h, w):
    """int32 [360, R, 2], ``R = int(hypot(h, w))``: entry ``[a, r - 1]`` is ``(floor(r * cos(a) + 0.5), floor(r * sin(a) + 0.5))`` for whole
    degrees ``a`` in CPython's double arithmetic -- the (dx, dy) of step ``r`` as the NEAREST pixel.  ``analysis.ray_table`` truncates
    ``cx + r * cos`` as the reference does; that pattern depends on the centre, so it cannot serve an origin that is data.  R reaches across
    the frame's diagonal: a ray from any pixel leaves the frame within the table."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f'frame size must be positive, got {h} x {w}')
    R = int(math.hypot(h, w))
    r = np.arange(1, R + 1, dtype=np.float64)
    off = np.zeros((ANGLES, R, 2), np.int32)
    for a in range(ANGLES):
        rad = math.radians(a)
        off[a, :, 0] = np.floor(r * math.cos(rad) + 0.5)       # IEEE double multiply and add, element by element: CPython's values
        off[a, :, 1] = np.floor(r * math.sin(rad) + 0.5)
    return off


def _ray_offsets_dev(h, w, device):
    key = (int(h), int(w), str(device))
    if key not in _offsets:
        _offsets[key] = torch.from_numpy(ray_offsets(h, w)).to(device)
    return _offsets[key]


def centred_profile(stack, origin='own'):
    """The polar profile walked from an origin that is data.  ``stack`` float32 CUDA [N, H, W, channels <= 8]; ``origin``: ``'own'`` (every
    plane from its own centroid), a class name or channel index (every channel of a slice from that class's centroid: one gather serves them
    all), or an int32 CUDA tensor [N, channels, 2 or 3] of (x, y[, anything]) pixels.  Returns ``(prof, length, origins)``: int32 CUDA
    [N, channels, 360, 5] = IN, OUT, LAST, HITS, RUNS as ``polar.polar_profile`` defines them, so ``polar.summarize``, ``overlap``,
    ``build_report`` and ``carpet_view`` take it unchanged; int32 [N, channels, 360], the steps inside the frame (``OUT == length``: the
    frame cut the run); and the int32 [N, channels, 3] origins used.  An origin outside the frame -- the (-1, -1) of an empty plane -- gives a
    zero profile and length 0.  Two or three launches, no host synchronisation."""
    n, h, w, sc = _check_stack(stack, MAX_WALK_CHANNELS)
    stack = stack.contiguous()
    if torch.is_tensor(origin):
        if not (origin.dtype == torch.int32 and origin.dim() == 3 and tuple(origin.shape[:2]) == (n, sc) and origin.shape[2] in (2, 3)
                and origin.device == stack.device):
            raise ValueError(f'origin must be an int32 tensor [{n}, {sc}, 2 or 3] on the stack\'s device')
        org = origin if origin.shape[2] == 3 else torch.nn.functional.pad(origin, (0, 1))
        org = org.contiguous()
    else:
        ref = None if isinstance(origin, str) and origin == 'own' else origin
        _channel(ref, sc)                                      # refused before any launch
        org = origins(stack, moments_stack(stack), ref)
    off = _ray_offsets_dev(h, w, stack.device)
    R = int(off.shape[1])
    prof = torch.empty((n, sc, ANGLES, FIELDS), dtype=torch.int32, device=stack.device)
    length = torch.empty((n, sc, ANGLES), dtype=torch.int32, device=stack.device)
    with torch.cuda.device(stack.device):
        L.check(L.lib().octseg_stack_polar_at(L.ptr(stack), n, h, w, sc, L.ptr(org), L.ptr(off), R, L.ptr(prof), L.ptr(length), L.stream_ptr()))
    return prof, length, org


def shape_table(mom):
    """Per (slice, channel) from ``mom`` [N, channels, 12] (CUDA tensor: one device-to-host copy; or numpy).  Pure host, float64 from the
    integers; the central moments are formed in exact integer arithmetic first (``M20 * M00 - M10 ** 2``), so nothing cancels.  A dict of
    numpy arrays [N, channels]: ``area`` (M00), ``cx`` / ``cy`` (M10 / M00, M01 / M00), ``xmin`` / ``xmax`` / ``ymin`` / ``ymax``, the central
    second moments per pixel ``mu20`` / ``mu11`` / ``mu02`` (the covariance of the set pixels' coordinates), ``major`` / ``minor`` = 4 *
    sqrt(eigenvalue) (the full axes of the ellipse with that covariance), ``orientation`` = 0.5 * atan2(2 * mu11, mu20 - mu02) (radians, the
    major axis against +x with y pointing down the rows), ``perimeter`` (EDGES) and ``compactness`` = 4 * pi * area / EDGES ** 2.  An empty
    plane has area 0, the box ``(W, -1, H, -1)`` the kernel leaves, and zeros elsewhere."""
    if torch.is_tensor(mom):
        mom = mom.cpu().numpy()
    mom = np.asarray(mom)
    if mom.ndim != 3 or mom.shape[2] != MOMENT_FIELDS:
        raise ValueError(f'mom {mom.shape} must be [N, channels, {MOMENT_FIELDS}]')
    n, sc = mom.shape[:2]
    out = {k: np.zeros((n, sc), np.float64) for k in ('cx', 'cy', 'mu20', 'mu11', 'mu02', 'major', 'minor', 'orientation', 'compactness')}
    out['area'] = mom[:, :, M00].astype(np.int64)
    out['perimeter'] = mom[:, :, EDGES].astype(np.int64)
    for k, f in (('xmin', XMIN), ('xmax', XMAX), ('ymin', YMIN), ('ymax', YMAX)):
        out[k] = mom[:, :, f].astype(np.int64)
    for i in range(n):
        for c in range(sc):
            m = [int(v) for v in mom[i, c]]
            a = m[M00]
            if a == 0:
                continue
            out['cx'][i, c], out['cy'][i, c] = m[M10] / a, m[M01] / a
            mu20 = (m[M20] * a - m[M10] ** 2) / (a * a)        # exact integers above the line
            mu11 = (m[M11] * a - m[M10] * m[M01]) / (a * a)
            mu02 = (m[M02] * a - m[M01] ** 2) / (a * a)
            out['mu20'][i, c], out['mu11'][i, c], out['mu02'][i, c] = mu20, mu11, mu02
            half, root = (mu20 + mu02) / 2.0, math.hypot((mu20 - mu02) / 2.0, mu11)
            out['major'][i, c] = 4.0 * math.sqrt(max(half + root, 0.0))
            out['minor'][i, c] = 4.0 * math.sqrt(max(half - root, 0.0))
            out['orientation'][i, c] = 0.5 * math.atan2(2.0 * mu11, mu20 - mu02)
            out['compactness'][i, c] = 4.0 * math.pi * a / (m[EDGES] ** 2)
    return out


def centroid_thickness(prof_row):
    """Median, min and max of OUT over the rays that meet the object (``IN > 0``), from one [360, 5] row of ``centred_profile(stack, 'own')``:
    how far the first run on each ray from the object's own centroid reaches.  The dict of ``analysis.radial_thickness``.

    This is NOT the reference's ``calculate_thickness_contour`` (``src/app/tools/analysis.py:21-57``).  That function also measures from the
    object's centroid, but along the vertices ``cv2.findContours`` returns, in its traversal order and after its vertex compression, and
    nothing here can pin a restatement of that; ``analysis.analyze_stack(thickness='contour')`` keeps refusing.  The rays here step to the
    nearest pixel of ``ray_offsets`` and are defined without OpenCV."""
    row = np.asarray(prof_row.cpu().numpy() if torch.is_tensor(prof_row) else prof_row)
    if row.shape != (ANGLES, FIELDS):
        raise ValueError(f'prof_row {row.shape} must be [{ANGLES}, {FIELDS}]')
    meas = [int(v) for v in row[row[:, IN] > 0, OUT]]
    if not meas:
        return {'median': 0, 'min': 0, 'max': 0, 'all_measurements': []}
    return {'median': float(np.median(meas)), 'min': int(min(meas)), 'max': int(max(meas)), 'all_measurements': meas}


LUMEN_KEYS = ('slice', 'area_px', 'area', 'centroid', 'catheter_offset', 'inside', 'd_min', 'd_max', 'd_mean', 'd_argmin', 'eccentricity',
              'd_equivalent', 'cut')


def build_lumen_report(mom, org, prof, length, h, w, image_names=None, ratio=None, ref_window=None):
    """``lumen_report`` from the integers of ONE channel: ``mom`` [N, 12], ``org`` [N, 3], ``prof`` [N, 360, 5], ``length`` [N, 360] (numpy or
    tensors), the profile walked from ``org``, and the frame size.  Pure host."""
    mom, org, prof, length = (np.asarray(v.cpu().numpy() if torch.is_tensor(v) else v).astype(np.int64) for v in (mom, org, prof, length))
    n = mom.shape[0]
    if mom.shape != (n, MOMENT_FIELDS) or org.shape != (n, 3) or prof.shape != (n, ANGLES, FIELDS) or length.shape != (n, ANGLES):
        raise ValueError(f'mom {mom.shape}, org {org.shape}, prof {prof.shape}, length {length.shape} must be [N, {MOMENT_FIELDS}], [N, 3], '
                         f'[N, {ANGLES}, {FIELDS}], [N, {ANGLES}]')
    h, w = int(h), int(w)
    ratio = int(h * 150 // 1000) if ratio is None else int(ratio)
    if ratio < 1:
        raise ValueError(f'ratio must be at least 1, got {ratio} (the default int(h * 150 // 1000) is 0 for frames below 7 rows)')
    if ref_window is not None:
        ref_window = int(ref_window)
        if ref_window < 1:
            raise ValueError(f'ref_window must be at least 1 slice, got {ref_window}')
    image_names = [str(i) for i in range(n)] if image_names is None else [str(s) for s in image_names]
    if len(image_names) != n:
        raise ValueError(f'{len(image_names)} names for {n} slices')
    lum = {k: [] for k in LUMEN_KEYS}
    for i in range(n):
        area = int(mom[i, M00])
        if not 0 < area < h * w:                               # analyze_stack's presence rule: a completely full mask is absent
            continue
        cx, cy = int(mom[i, M10]) / area, int(mom[i, M01]) / area
        lum['slice'].append(i)
        lum['area_px'].append(area)
        lum['area'].append(float(area / (ratio * ratio)))
        lum['centroid'].append([float(cx), float(cy)])
        lum['catheter_offset'].append(float(math.hypot(cx - w // 2, cy - h // 2) / ratio))
        inside = int(org[i, 2])
        lum['inside'].append(inside)
        if inside:
            e = np.where(prof[i, :, IN] == 1, prof[i, :, OUT], 0)
            d = e[:ANGLES // 2] + e[ANGLES // 2:] + 1
            k = int(np.argmin(d))                              # the first minimum
            lo, hi = int(d[k]), int(d.max())
            lum['d_min'].append(float(lo / ratio))
            lum['d_max'].append(float(hi / ratio))
            lum['d_mean'].append(float(int(d.sum()) / (ANGLES // 2) / ratio))
            lum['d_argmin'].append(k)
            lum['eccentricity'].append(float((hi - lo) / hi))
        else:
            for k in ('d_min', 'd_max', 'd_mean', 'd_argmin', 'eccentricity'):
                lum[k].append(None)
        lum['d_equivalent'].append(float(2.0 * math.sqrt(area / math.pi) / ratio))
        lum['cut'].append(bool((prof[i, :, OUT] == length[i]).any()))
    out = {'ratio': ratio, 'images': image_names, 'lumen': lum, 'mla': None, 'reference': None, 'area_stenosis': None}
    if lum['slice']:
        areas = lum['area_px']
        j = min(range(len(areas)), key=lambda q: (areas[q], q))    # the smallest present lumen, the first on ties
        at = lum['slice'][j]
        out['mla'] = {'slice': at, 'area_px': areas[j], 'area': lum['area'][j]}

        def side(cands):
            if not cands:
                return None
            q = max(cands, key=lambda q: (areas[q], -q))       # the largest, the first on ties
            return {'slice': lum['slice'][q], 'area_px': areas[q], 'area': lum['area'][q]}
        near = (lambda s: True) if ref_window is None else (lambda s: abs(s - at) <= ref_window)
        prox = side([q for q in range(len(areas)) if lum['slice'][q] < at and near(lum['slice'][q])])
        dist = side([q for q in range(len(areas)) if lum['slice'][q] > at and near(lum['slice'][q])])
        sides = [s['area_px'] for s in (prox, dist) if s is not None]
        ref_px = sum(sides) / len(sides) if sides else float(areas[j])
        out['reference'] = {'proximal': prox, 'distal': dist, 'area_px': float(ref_px), 'area': float(ref_px / (ratio * ratio))}
        out['area_stenosis'] = float(100.0 * (1.0 - areas[j] / ref_px))
    return out


def lumen_report(stack, image_names=None, ratio=None, clean=None, lumen='Lumen', ref_window=None):
    """The lumen reading of a mask stack on the device as a JSON-serialisable dict of plain Python ints, floats, bools and None.

    ``stack`` float32 CUDA [N, H, W, channels <= 8], channel ``CLASS_IDS[name] - 1`` per class; ``image_names`` one per slice (default ``'0',
    '1', ...``), the slices in pullback order; ``ratio`` defaults to ``int(h * 150 // 1000)`` and ``clean`` takes what
    ``analysis.analyze_stack`` takes, both as in ``polar.plaque_report``; ``lumen`` names the class.  Every channel is walked from the
    LUMEN's centroid (``centred_profile(stack, lumen)``); only the lumen channel's integers are copied to the host (its moments, and one int32 block of
    profile, lengths and origin).  Keys:

    ``ratio``, ``images``;
    ``lumen``: lists over the PRESENT slices (``0 < count < h * w``, ``analyze_stack``'s rule): ``slice``; ``area_px`` and ``area`` (``/
    ratio ** 2``); ``centroid`` [x, y] in pixels (M10 / M00, M01 / M00); ``catheter_offset``, centroid to the frame centre ``(w // 2, h // 2)``,
    ``/ ratio``; ``inside``, 1 where the lumen is set at its rounded centroid; over the 180 diameters ``d(t) = e(t) + e(t + 180) + 1`` with
    ``e(a) = OUT[a] if IN[a] == 1 else 0`` -- the two half-chords that leave the centroid pixel plus that pixel -- ``d_min``, ``d_max``,
    ``d_mean`` (``/ ratio``), ``d_argmin`` (the first degree attaining the minimum) and ``eccentricity = (d_max - d_min) / d_max``, all None
    where ``inside`` is 0 (a crescent: no chord through the centroid is a lumen diameter); ``d_equivalent = 2 * sqrt(area_px / pi) / ratio``;
    ``cut``, true where a ray's OUT equals its length: the frame ended the lumen, the diameters are lower bounds;
    ``mla``: ``{'slice', 'area_px', 'area'}`` of the smallest present lumen, the first on ties; None without a present slice;
    ``reference``: ``proximal`` = the largest present lumen BEFORE the MLA slice (lower index; the first on ties), ``distal`` the same after
    it, each ``{'slice', 'area_px', 'area'}`` or None, only slices within ``ref_window`` of the MLA slice when that is given; ``area_px`` /
    ``area`` = the mean of the sides that exist, the MLA's own area with none;
    ``area_stenosis = 100 * (1 - mla / reference)``.

    The calibration is the reference's ``ratio`` (``dcm.shape[1] * 150 // 1000`` steps per unit) and is NOT validated against a physical
    scale here.  The stenosis rule -- largest lumen on either side, mean of the two -- is this project's, not an implementation of a consensus
    document; which slices are proximal depends on the pullback's direction, which the stack does not carry.  Steps are nearest pixels
    (``ray_offsets``), not the reference's truncated ones, and none of this is ``calculate_thickness_contour``."""
    from .cleanup import clean_kwargs, clean_stack
    if lumen not in CLASS_IDS:
        raise ValueError(f'unknown class {lumen!r}')
    n, h, w, sc = _check_stack(stack, MAX_WALK_CHANNELS)
    ch = _channel(lumen, sc)
    if (int(h * 150 // 1000) if ratio is None else int(ratio)) < 1:
        raise ValueError(f'ratio must be at least 1, got {int(h * 150 // 1000) if ratio is None else int(ratio)} (the default int(h * 150 // '
                         '1000) is 0 for frames below 7 rows)')
    kw = clean_kwargs(clean)
    if kw is not None:
        stack = clean_stack(stack, **kw)
    mom = moments_stack(stack)
    prof, length, org = centred_profile(stack, origins(stack, mom, ch))
    host = torch.cat([prof[:, ch].reshape(n, -1), length[:, ch], org[:, ch]], dim=1).cpu().numpy()    # the one copy of the int32 results
    prof_h, length_h, org_h = host[:, :ANGLES * FIELDS].reshape(n, ANGLES, FIELDS), host[:, ANGLES * FIELDS:ANGLES * (FIELDS + 1)], host[:, -3:]
    return build_lumen_report(mom[:, ch].cpu().numpy(), org_h, prof_h, length_h, h, w, image_names, ratio=ratio, ref_window=ref_window)
