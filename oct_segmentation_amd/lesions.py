"""Lesions in 3-D on the GPU: the connected components of a mask stack ACROSS its slices (``csrc/lesions.hip``, ``octseg_volume_components`` /
``octseg_volume_cleanup``; no reference counterpart).

Everything else the package measures on a stack is per slice: ``cleanup.label_stack`` labels every plane on its own and ``analysis.analyze_stack``
groups slices into "objects" by class presence alone, as upstream's ``get_analysis`` does.  A pullback is a volume.  Here a VOLUME is one channel
of the stack, slices along N in the order given; voxels are 8-connected inside a slice and connect between adjacent slices either through the
same pixel only (``across='overlap'``, the default: the frame pitch is an order of magnitude above the pixel pitch) or through the 3 x 3
(``across='full'``, 26-connected).

    labels = label_volume(stack)                               # int32 CUDA [channels, N, H, W]: 1 + n*H*W + y*W + x of the first voxel, 0 background
    nles, top, profile = lesion_table(stack, profile=True)     # int32 CUDA [channels], [channels, 32, 8], [channels, 32, N]
    stack = clean_volume(stack, min_slices=2)                  # the flicker filter: what shows in one slice only goes
    report = lesion_report(stack, image_names)                 # per class: lesions with length, voxels, bounding box, area profile, peak

``stack`` is float32 CUDA [N, H, W, channels], any value != 0 set.  Everything is integer: results EQUAL ``scipy.ndimage.label``'s with the
explicit 3 x 3 x 3 structure, no tolerance.  Nothing synchronises with the host before ``lesion_report``'s one copy of the tables; scratch comes
from torch's allocator, sized by the library.
"""
import numpy as np
import torch

from . import _lib as L

MAX_CHANNELS = 16
TOPL = 32
TOP_COLUMNS = ('voxels', 'first_voxel', 'z0', 'z1', 'y0', 'y1', 'x0', 'x1')
ACROSS = {'overlap': 0, 'full': 1}
DEFAULT_SCRATCH = 8 << 30      # about 13.3 bytes per voxel and channel: a 186 x 750 x 750 x 4 pullback needs 5.6 GB and goes in one call


def _check(stack, across):
    if across not in ACROSS:
        raise ValueError(f"across must be 'overlap' or 'full', got {across!r}")
    if not (torch.is_tensor(stack) and stack.is_cuda and stack.dtype == torch.float32 and stack.dim() == 4):
        raise ValueError('stack must be a float32 CUDA tensor [N, H, W, channels]')
    if 0 in stack.shape:
        raise ValueError('empty stack or frame')
    n, h, w, sc = (int(v) for v in stack.shape)
    if sc > MAX_CHANNELS:
        raise ValueError(f'at most {MAX_CHANNELS} channels, got {sc}')
    if n * h * w >= 2 ** 31 - 1:
        raise ValueError(f'volume {n} x {h} x {w} has 2^31 - 1 voxels or more')
    return stack.contiguous(), n, h, w, sc, ACROSS[across]


def _chunks(stack, n, h, w, sc, scratch_bytes):
    """``(channels per call, scratch tensor, its bytes)``: all channels in one call when their scratch fits the budget, else one at a time."""
    lib = L.lib()
    for per in (sc, 1):
        need = int(lib.octseg_lesions_scratch_bytes(per, n, h, w))
        if need <= int(scratch_bytes):
            return per, torch.empty((need,), dtype=torch.uint8, device=stack.device), need
    raise ValueError(f'one channel of a {n} x {h} x {w} volume needs {need} bytes of scratch, scratch_bytes is {int(scratch_bytes)}')


def _pieces(stack, sc, per):
    """The stack itself (all channels in one call) or one contiguous single-channel copy per channel: ``(first channel, channels, tensor)``."""
    if per == sc:
        yield 0, sc, stack
    else:
        for c in range(sc):
            yield c, 1, stack[:, :, :, c:c + 1].contiguous()


def _components(stack, across, want_labels, want_table, want_profile, scratch_bytes=DEFAULT_SCRATCH):
    stack, n, h, w, sc, ac = _check(stack, across)
    dev = stack.device
    labels = torch.empty((sc, n, h, w), dtype=torch.int32, device=dev) if want_labels else None
    nles = torch.empty((sc,), dtype=torch.int32, device=dev) if want_table else None
    top = torch.empty((sc, TOPL, len(TOP_COLUMNS)), dtype=torch.int32, device=dev) if want_table else None
    prof = torch.empty((sc, TOPL, n), dtype=torch.int32, device=dev) if want_profile else None
    with torch.cuda.device(dev):
        per, scratch, nbytes = _chunks(stack, n, h, w, sc, scratch_bytes)
        for c, m, src in _pieces(stack, sc, per):
            L.check(L.lib().octseg_volume_components(L.ptr(src), n, h, w, m, ac, L.ptr(scratch), nbytes,
                                                     L.ptr(labels[c:c + m]) if want_labels else None,
                                                     L.ptr(nles[c:c + m]) if want_table else None,
                                                     L.ptr(top[c:c + m]) if want_table else None,
                                                     L.ptr(prof[c:c + m]) if want_profile else None, L.stream_ptr()))
    return labels, nles, top, prof


def label_volume(stack, across='overlap', scratch_bytes=DEFAULT_SCRATCH):
    """The components of every channel's volume: int32 CUDA [channels, N, H, W], the label of a lesion is ``1 + n * H * W + y * W + x`` of its
    first voxel in raster order, background 0 (``scipy.ndimage.label`` with the 3 x 3 x 3 structure of ``across``, relabelled).  For N = 1 this is
    ``cleanup.label_stack``."""
    return _components(stack, across, True, False, False, scratch_bytes)[0]


def lesion_table(stack, across='overlap', profile=False, scratch_bytes=DEFAULT_SCRATCH):
    """``(nles, top)`` or, with ``profile``, ``(nles, top, profile)``: int32 CUDA [channels], the number of lesions; int32 CUDA [channels, 32, 8],
    the 32 largest by voxels descending then first voxel ascending, columns ``TOP_COLUMNS`` (inclusive bounds), rows beyond ``nles`` zero; int32
    CUDA [channels, 32, N], the set pixels of ranked lesion r in slice n."""
    _, nles, top, prof = _components(stack, across, False, True, bool(profile), scratch_bytes)
    return (nles, top, prof) if profile else (nles, top)


def clean_volume(stack, min_slices=2, min_voxels=0, keep=0, across='overlap', return_table=False, scratch_bytes=DEFAULT_SCRATCH):
    """The stack with only the lesions for which all three hold: at least ``min_slices`` slices from first to last (2 = the flicker filter), at
    least ``min_voxels`` voxels, and voxels >= t, the ``keep``-th largest voxel count of the channel (ties at t all stay; ``keep=0``: no rank
    filter).  Returns float32 0.0 / 1.0 in the input's layout (the input is not modified); with ``return_table`` also ``(nles, top)`` of the kept
    lesions.  All channels go in one call when their scratch fits ``scratch_bytes``, one channel at a time when not; the result does not depend
    on the chunking."""
    min_slices, min_voxels, keep = int(min_slices), int(min_voxels), int(keep)
    if keep < 0 or min_voxels < 0:
        raise ValueError('keep and min_voxels must not be negative')
    if min_slices < 1:
        raise ValueError(f'min_slices must be at least 1, got {min_slices}')
    stack, n, h, w, sc, ac = _check(stack, across)
    dev = stack.device
    out = torch.empty_like(stack)
    nles = torch.empty((sc,), dtype=torch.int32, device=dev) if return_table else None
    top = torch.empty((sc, TOPL, len(TOP_COLUMNS)), dtype=torch.int32, device=dev) if return_table else None
    with torch.cuda.device(dev):
        per, scratch, nbytes = _chunks(stack, n, h, w, sc, scratch_bytes)
        for c, m, src in _pieces(stack, sc, per):
            dst = out if per == sc else torch.empty_like(src)
            L.check(L.lib().octseg_volume_cleanup(L.ptr(src), n, h, w, m, ac, keep, min_voxels, min_slices, L.ptr(scratch), nbytes, L.ptr(dst),
                                                  L.ptr(nles[c:c + m]) if return_table else None,
                                                  L.ptr(top[c:c + m]) if return_table else None, L.stream_ptr()))
            if per != sc:
                out[:, :, :, c:c + 1] = dst
    return (out, (nles, top)) if return_table else out


def clean_kwargs(clean):
    """The ``clean`` argument of ``lesion_report``: None / False = off, True = ``clean_volume``'s defaults, a dict = its keywords."""
    if clean is None or clean is False:
        return None
    if clean is True:
        return {}
    if isinstance(clean, dict):
        bad = set(clean) - {'min_slices', 'min_voxels', 'keep', 'scratch_bytes'}
        if bad:
            raise ValueError(f'unknown clean_volume keywords: {sorted(bad)}')
        return dict(clean)
    raise ValueError(f'clean must be None, a bool or a dict of clean_volume keywords, got {clean!r}')


def default_classes(channels):
    """One name per channel: the names of ``model.CLASS_IDS`` in id order, then ``channel_<i>``."""
    from .model import CLASS_IDS
    names = [name for _, name in sorted((cid, name) for name, cid in CLASS_IDS.items())]
    return [names[c] if c < len(names) else f'channel_{c}' for c in range(int(channels))]


def build_report(nles, top, profile, h, w, image_names=None, classes=None, ratio=None):
    """The lesion report from the integers: ``nles`` [channels], ``top`` [channels, 32, 8] and ``profile`` [channels, 32, N] (numpy or anything
    ``np.asarray`` takes), the frame size, optionally one name per slice, one name per channel (default ``default_classes``) and upstream's
    ``ratio``.  Pure host.  Returns ``{class: {'n_lesions', 'truncated', 'lesions': [...]}}``; ``truncated`` says that the class has more than
    the 32 lesions listed.  A lesion: ``id`` (its rank, 0 the largest), ``first_slice`` / ``last_slice`` (indices; ``first_image`` /
    ``last_image`` with names), ``length`` in slices, ``voxels``, ``first_voxel`` [n, y, x], ``bbox`` {z0, z1, y0, y1, x0, x1} (inclusive),
    ``area`` (set pixels per slice over first..last), ``peak_area`` and ``peak_slice`` (the first slice of the largest area).  With ``ratio``
    also ``area_ratio`` and ``peak_area_ratio``: upstream's ``pow(count // ratio, 0.5)`` as in ``analysis.build_analysis``.  Values are plain
    Python ints and floats: the dict goes through ``json.dump``."""
    nles, top, profile = np.asarray(nles), np.asarray(top), np.asarray(profile)
    h, w = int(h), int(w)
    if nles.ndim != 1 or top.shape != nles.shape + (TOPL, len(TOP_COLUMNS)) or profile.ndim != 3 or profile.shape[:2] != nles.shape + (TOPL,):
        raise ValueError(f'nles {nles.shape}, top {top.shape} and profile {profile.shape} must be [channels], [channels, {TOPL}, '
                         f'{len(TOP_COLUMNS)}] and [channels, {TOPL}, N]')
    n = int(profile.shape[2])
    if h < 1 or w < 1:
        raise ValueError(f'frame size must be positive, got {h} x {w}')
    if image_names is not None:
        image_names = [str(s) for s in image_names]
        if len(image_names) != n:
            raise ValueError(f'{len(image_names)} names for {n} slices')
    classes = default_classes(nles.shape[0]) if classes is None else [str(s) for s in classes]
    if len(classes) != nles.shape[0] or len(set(classes)) != len(classes):
        raise ValueError(f'{len(classes)} class names for {nles.shape[0]} channels, or a name twice')
    if ratio is not None:
        ratio = int(ratio)
        if ratio < 1:
            raise ValueError(f'ratio must be at least 1, got {ratio}')
    report = {}
    for c, name in enumerate(classes):
        count = int(nles[c])
        lesions = []
        for r in range(min(count, TOPL)):
            voxels, first, z0, z1, y0, y1, x0, x1 = (int(v) for v in top[c, r])
            area = [int(v) for v in profile[c, r, z0:z1 + 1]]
            peak = int(np.argmax(area))
            les = {'id': r, 'first_slice': z0, 'last_slice': z1, 'length': z1 - z0 + 1, 'voxels': voxels,
                   'first_voxel': [first // (h * w), first % (h * w) // w, first % w],
                   'bbox': {'z0': z0, 'z1': z1, 'y0': y0, 'y1': y1, 'x0': x0, 'x1': x1},
                   'area': area, 'peak_area': area[peak], 'peak_slice': z0 + peak}
            if image_names is not None:
                les['first_image'], les['last_image'] = image_names[z0], image_names[z1]
            if ratio is not None:
                les['area_ratio'] = [float(pow(a // ratio, 0.5)) for a in area]
                les['peak_area_ratio'] = float(pow(area[peak] // ratio, 0.5))
            lesions.append(les)
        report[name] = {'n_lesions': count, 'truncated': count > TOPL, 'lesions': lesions}
    return report


def lesion_report(stack, image_names=None, classes=None, ratio=None, across='overlap', clean=None):
    """``build_report`` for a mask stack on the device: ``lesion_table`` with the profile, ONE device-to-host copy of the three tables (about
    (33 + N) * 128 bytes per class), the rest on the host.  ``clean``: None (default, the stack as it is), True or a dict of ``clean_volume``
    keywords: the stack goes through ``clean_volume`` (with the same ``across``) first."""
    kw = clean_kwargs(clean)
    if kw is not None:
        stack = clean_volume(stack, across=across, **kw)
    nles, top, prof = lesion_table(stack, across=across, profile=True)
    sc, n = int(top.shape[0]), int(prof.shape[2])
    host = torch.cat([nles.reshape(sc, 1), top.reshape(sc, -1), prof.reshape(sc, -1)], dim=1).cpu().numpy()
    k = TOPL * len(TOP_COLUMNS)
    return build_report(host[:, 0], host[:, 1:1 + k].reshape(sc, TOPL, len(TOP_COLUMNS)), host[:, 1 + k:].reshape(sc, TOPL, n),
                        int(stack.shape[1]), int(stack.shape[2]), image_names=image_names, classes=classes, ratio=ratio)
