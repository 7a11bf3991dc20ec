"""Raw pullback volumes on the GPU -- the two steps in front of ``segment_stack`` that the reference runs on the host, frame by frame.

1. ``cv2.normalize(slice, None, 0, 255, NORM_MINMAX, CV_8U)`` + ``cvtColor(BGR2RGB)`` of every slice of a DICOM's ``pixel_array``
   (reference ``src/data/convert_dicoms.py:71-81``, again in ``src/app/tools/analysis.py:167-177``): ``normalize_volume``.
2. ``Image.open(p).resize(output_size)`` of ``data_processing`` (``src/data/utils.py:187``), Pillow's default BICUBIC: ``resize_pil_u8``.

Both are kernels of ``csrc/volume.hip``.  The resize is Pillow's own 8-bit integer arithmetic (``Resample.c``) driven by the tables
``pil_resample_table`` makes, and EQUALS ``Image.resize`` byte for byte.  The normalisation restates OpenCV 4.8.1's ``normalize`` /
``convertTo`` in its unfused baseline form (``x * a`` and ``+ b`` each rounded to float32); cv2 is not installed where this project runs
and its AVX2 build fuses the two, so parity with cv2 itself is unpinned.  Reading DICOM files stays outside: a caller hands
over ``pydicom.dcmread(f).pixel_array``.

    frames = normalize_volume(pixel_array)                              # [S,H,W,3] | [S,H,W] uint8 | uint16 -> uint8 CUDA [S,H,W,3] RGB
    frames = resize_pil_u8(frames, (1000, 1000))                        # uint8 CUDA [S,oh,ow,C], every frame = Image.resize((ow, oh))
    result = analyze_pullback(pixel_array, models_dir, classes)         # .data: the app's get_analysis dict; .stack, .frames on the device
"""
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L

PRECISION_BITS = 32 - 8 - 2           # Resample.c: coefficients of the 8-bit path carry 22 fractional bits
BICUBIC_SUPPORT = 2.0

_tables = {}   # (in, out, device) -> (bounds, kk, ksize) device int32 tensors

Pullback = namedtuple('Pullback', 'data stack frames overlay color_mask plaque lumen', defaults=(None, None))


def _bicubic(x):
    """Resample.c ``bicubic_filter`` with ``a = -0.5``, the operations in its order."""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_resample_table(in_size, out_size):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` (``src/libImaging/Resample.c``) for BICUBIC over the whole axis
    (box = (0, in_size)): ``bounds`` int32 [out_size, 2], first source index and tap count of every output index, and ``kk`` int32
    [out_size, ksize], the coefficients at 22 fractional bits, zero behind the count.  ``filterscale = max(in / out, 1)``,
    ``support = 2.0 * filterscale``, ``ksize = 2 * ceil(support) + 1``; per output ``center = (i + 0.5) * in / out``, taps
    ``int(center - support + 0.5)`` (at least 0) up to ``int(center + support + 0.5)`` (at most in_size), weights
    ``bicubic((x - center + 0.5) / filterscale)`` normalised by their sum in double, then ``int(w * 2 ** 22 +- 0.5)`` by sign."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f'sizes must be positive, got {in_size} -> {out_size}')
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = BICUBIC_SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            kk[xx, x] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _table_dev(in_size, out_size, device):
    key = (int(in_size), int(out_size), str(device))
    if key not in _tables:
        bounds, kk = pil_resample_table(in_size, out_size)
        _tables[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), int(kk.shape[1]))
    return _tables[key]


def resize_pil_u8(frames_u8, size):
    """``Image.fromarray(frame).resize((ow, oh))`` (Pillow's default BICUBIC) of every frame: uint8 CUDA [S,H,W,C], C = 1 (mode L) or 3 (RGB)
    -> uint8 CUDA [S,oh,ow,C], equal to Pillow byte for byte.  ``size``: an int (square) or ``(oh, ow)``.  Two launches through a uint8
    intermediate [S,H,ow,C]; an axis that keeps its length is skipped, as Pillow skips it.  No host synchronisation."""
    from .ingest import _check_u8, _size2
    _check_u8(frames_u8, 'frames_u8')
    oh, ow = _size2(size)
    x = frames_u8.contiguous()
    S, H, W, C = (int(v) for v in x.shape)
    if C not in (1, 3):
        raise ValueError(f'frames_u8 must have 1 or 3 channels, got {tuple(x.shape)}')
    if H < 1 or W < 1:
        raise ValueError('empty frame')
    if max(H * W, H * ow, oh * ow) * C >= 2 ** 31:
        raise ValueError('a frame must stay below 2^31 bytes')
    dev = x.device
    out = torch.empty((S, oh, ow, C), dtype=torch.uint8, device=dev)
    xb = xk = yb = yk = tmp = None
    xks = yks = 0
    if ow != W:
        xb, xk, xks = _table_dev(W, ow, dev)
    if oh != H:
        yb, yk, yks = _table_dev(H, oh, dev)
    if ow != W and oh != H:
        tmp = torch.empty((S, H, ow, C), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().octseg_resize_pil_u8(L.ptr(x), S, H, W, C, L.ptr(tmp), L.ptr(out), oh, ow, L.ptr(xb), L.ptr(xk), xks, L.ptr(yb), L.ptr(yk),
                                             yks, L.stream_ptr()))
    return out


def _volume_bytes(volume, device):
    """``volume`` as (device tensor holding its bytes, dtype code, shape).  torch may lack uint16 arithmetic and numpy has no device form: the
    bytes go up as they are and the kernel gets the pointer."""
    if isinstance(volume, np.ndarray):
        if volume.dtype not in (np.uint8, np.uint16):
            raise ValueError(f'volume must be uint8 or uint16, got {volume.dtype} (signed and float volumes are out of scope)')
        host = np.ascontiguousarray(volume)
        code = 1 if host.dtype == np.uint16 else 0
        return torch.from_numpy(host.reshape(-1).view(np.uint8)).to(device), code, tuple(host.shape)
    if torch.is_tensor(volume):
        if not volume.is_cuda:
            raise ValueError('a tensor volume must be on the GPU (pass host data as a numpy array)')
        u16 = getattr(torch, 'uint16', None)
        if volume.dtype != torch.uint8 and (u16 is None or volume.dtype != u16):
            raise ValueError(f'volume must be uint8 or uint16, got {volume.dtype} (signed and float volumes are out of scope)')
        return volume.contiguous(), 0 if volume.dtype == torch.uint8 else 1, tuple(volume.shape)
    raise ValueError('volume must be a numpy array or a CUDA tensor')


def normalize_volume(volume, swap_rb=True, device='cuda', return_minmax=False):
    """``cv2.normalize(slice, None, 0, 255, NORM_MINMAX, CV_8U)`` (+ ``cvtColor(BGR2RGB)`` with ``swap_rb``) of every slice:
    ``volume`` a numpy array or CUDA tensor [S,H,W,3] or [S,H,W], uint8 or uint16 -> uint8 CUDA [S,H,W,3] (a grey volume is written to three
    equal channels).  Minimum and maximum are taken per slice over all channels, on the device; nothing comes back to the host.
    ``return_minmax=True`` also returns them, int64 CUDA [S, 2].  ``device`` places a numpy volume; a tensor stays where it is."""
    data, code, shape = _volume_bytes(volume, device)
    if len(shape) == 3:
        shape = shape + (1,)
    if len(shape) != 4 or shape[3] not in (1, 3):
        raise ValueError(f'volume must be [S, H, W, 3] or [S, H, W], got {shape}')
    S, H, W, C = (int(v) for v in shape)
    if S < 1 or H < 1 or W < 1:
        raise ValueError('empty volume or frame')
    if H * W * max(3, C * (2 if code else 1)) >= 2 ** 31:
        raise ValueError('a frame must stay below 2^31 bytes')
    dev = data.device
    minmax = torch.empty((S, 2), dtype=torch.int32, device=dev)       # the kernel's uint32 pairs; values stay below 2^16
    out = torch.empty((S, H, W, 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().octseg_volume_normalize(L.ptr(data), code, S, H, W, C, int(bool(swap_rb)), L.ptr(minmax), L.ptr(out), L.stream_ptr()))
    return (out, minmax.to(torch.int64)) if return_minmax else out


def analyze_pullback(volume, models_dir, classes, output_size=(1000, 1000), names=None, render=False, swap_rb=True, close_iterations=1,
                     clean=None, plaque=None, lumen=None, **segment_kwargs):
    """From a raw volume to the app's dict in one call: ``normalize_volume`` -> ``resize_pil_u8`` -> ``predict.segment_stack`` ->
    ``analysis.analyze_stack``; with ``render=True`` also ``postprocess.render_results``.  The frames go up once, at source size, and nothing
    comes back but the results.

    ``volume``: [S,H,W,3] or [S,H,W], uint8 or uint16 (``pixel_array``).  ``output_size`` as in ``configs/predict.yaml``: the frames are
    resized as ``Image.resize(tuple(output_size))`` does, the mask stack is [S, output_size[0], output_size[1], 4] (square sizes, as
    upstream).  ``ratio = int(volume.shape[1] * 150 // 1000)``: the SOURCE height, upstream's ``dcm.shape[1]``, not the output size.
    ``names`` default to ``'001', '002', ...`` (the ``slice+1:03d`` of convert_dicoms).  ``segment_kwargs`` go to ``segment_stack``
    (``batch_size``, ``compute_dtype``, ``use_graph``, ``device``).  ``clean``: None (default), True or a dict of ``cleanup.clean_stack``
    keywords: the mask stack is cleaned once (smoothing, keep-largest, hole fill) and the cleaned stack is measured, rendered and returned.
    ``plaque``: None (default), True or a dict of ``polar.plaque_report`` keywords (``cap``, ``lipid``, ``thin_cap``, ``wide_arc``, ``ratio``):
    the polar plaque report of the stack that is measured (after ``clean``), with the same names and, unless given, the same ``ratio``.
    ``lumen``: None (default), True or a dict of ``shape.lumen_report`` keywords (``lumen``, ``ref_window``, ``ratio``): the lumen report of the
    same stack, with the same names and, unless given, the same ``ratio``.

    Returns ``Pullback(data, stack, frames, overlay, color_mask, plaque, lumen)``: the dict, the float32 mask stack and the uint8 RGB frames at
    output size on the device; overlay and colour mask (uint8 CUDA [S,oh,ow,3]) with ``render=True``, else None; ``plaque`` and ``lumen`` the
    reports or None."""
    from .analysis import analyze_stack
    from .postprocess import render_results
    from .predict import segment_stack
    pk = None                                                                        # refused before any work is done
    if plaque is not None and plaque is not False:
        if plaque is not True and not isinstance(plaque, dict):
            raise ValueError(f'plaque must be None, a bool or a dict of plaque_report keywords, got {plaque!r}')
        pk = {} if plaque is True else dict(plaque)
        bad = set(pk) - {'ratio', 'cap', 'lipid', 'thin_cap', 'wide_arc'}
        if bad:
            raise ValueError(f'unknown plaque_report keywords: {sorted(bad)}')
    lk = None
    if lumen is not None and lumen is not False:
        if lumen is not True and not isinstance(lumen, dict):
            raise ValueError(f'lumen must be None, a bool or a dict of lumen_report keywords, got {lumen!r}')
        lk = {} if lumen is True else dict(lumen)
        bad = set(lk) - {'ratio', 'lumen', 'ref_window'}
        if bad:
            raise ValueError(f'unknown lumen_report keywords: {sorted(bad)}')
    frames = normalize_volume(volume, swap_rb=swap_rb, device=segment_kwargs.get('device', 'cuda'))
    S, H = int(frames.shape[0]), int(frames.shape[1])
    frames = resize_pil_u8(frames, (int(output_size[1]), int(output_size[0])))       # PIL sizes are (width, height)
    if names is None:
        names = [f'{i + 1:03d}' for i in range(S)]
    stack = segment_stack(frames, output_size, classes, models_dir, **segment_kwargs)
    from .cleanup import clean_kwargs, clean_stack
    kw = clean_kwargs(clean)
    if kw is not None:
        stack = clean_stack(stack, **kw)
    data = analyze_stack(stack, names, ratio=int(H * 150 // 1000))
    overlay = color_mask = None
    if render:
        overlay, color_mask = render_results(frames, stack, classes, close_iterations)
    report = None
    if pk is not None:
        from .polar import plaque_report
        pk.setdefault('ratio', int(H * 150 // 1000))
        report = plaque_report(stack, names, **pk)
    lumen_rep = None
    if lk is not None:
        from .shape import lumen_report
        lk.setdefault('ratio', int(H * 150 // 1000))
        lumen_rep = lumen_report(stack, names, **lk)
    return Pullback(data, stack, frames, overlay, color_mask, report, lumen_rep)
