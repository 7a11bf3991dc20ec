"""The polar plaque profile: what a Lumen / Fibrous cap / Lipid core segmentation of an OCT pullback is read for.  The reference's
``calculate_object_thickness`` (``src/app/tools/analysis.py:60-130``) returns, per ray, the radius at which the first run on the ray ENDS: a
radius for the lumen, the distance of the far edge for anything else.  Here the same 360 rays (``analysis.ray_table``; from the frame centre, the
A-lines of a catheter-centred frame) are walked to their end (``octseg_stack_polar``, ``csrc/polar.hip``) and five integers per slice, class and
degree come back: ``IN`` first set step, ``OUT`` last step of the first run (``measure_stack``'s radius), ``LAST`` last set step, ``HITS`` set
steps, ``RUNS`` runs.  Arcs, thicknesses and the cap-over-lipid report are host numpy over those integers (28.8 KB per slice at four classes).

    prof = polar_profile(stack)                                # int32 CUDA [N, C, 360, 5]; stack float32 CUDA [N, H, W, C], C <= 8
    prof, labels = polar_profile(stack, want_map=True)         # + uint8 CUDA [N, 360, R], bit c = class c set at that step
    view = unwrap_frames(frames_u8)                            # uint8 CUDA [N, 360, R, C]: the frames in the same polar layout
    report = plaque_report(stack, image_names)                 # lipid arc, cap thickness over lipid, per slice; json.dump-able
"""
import numpy as np
import torch

from . import _lib as L
from .analysis import ANGLES, _ray_table_dev
from .model import CLASS_IDS

MAX_CHANNELS = 8                       # the label map keeps one bit per class in a byte
IN, OUT, LAST, HITS, RUNS = range(5)
FIELDS = 5


def polar_profile(stack, want_map=False):
    """``stack`` float32 CUDA [N, H, W, channels <= 8] (any value != 0 is set).  Returns ``prof`` int32 CUDA [N, channels, 360, 5] = IN, OUT,
    LAST, HITS, RUNS per ray (``include/octseg.h``, octseg_stack_polar); with ``want_map=True`` ``(prof, map)``, map uint8 CUDA [N, 360, R]
    with bit ``c`` set where channel ``c`` is set at step ``r = index + 1``, 0 past the ray's end.  One call, no host synchronisation."""
    if not (torch.is_tensor(stack) and stack.dtype == torch.float32 and stack.dim() == 4):
        raise ValueError('stack must be a float32 CUDA tensor [N, H, W, channels]')
    if 0 in stack.shape:
        raise ValueError('empty batch or frame')
    n, h, w, sc = (int(v) for v in stack.shape)
    if sc > MAX_CHANNELS:
        raise ValueError(f'at most {MAX_CHANNELS} channels, got {sc}')
    if h * w >= 2 ** 31:
        raise ValueError(f'frame {h} x {w} has 2^31 pixels or more')
    if not stack.is_cuda:
        raise ValueError('stack must be a float32 CUDA tensor [N, H, W, channels]: it is on the host, and there is no CPU path')
    stack = stack.contiguous()
    pix, length = _ray_table_dev(h, w, stack.device)
    R = int(pix.shape[1])
    prof = torch.empty((n, sc, ANGLES, FIELDS), dtype=torch.int32, device=stack.device)
    labels = torch.empty((n, ANGLES, R), dtype=torch.uint8, device=stack.device) if want_map else None
    with torch.cuda.device(stack.device):
        L.check(L.lib().octseg_stack_polar(L.ptr(stack), n, h, w, sc, L.ptr(pix) if R else None, L.ptr(length), R, L.ptr(prof),
                                           L.ptr(labels) if want_map and R else None, L.stream_ptr()))
    return (prof, labels) if want_map else prof


def unwrap_frames(frames_u8):
    """``frames_u8`` uint8 CUDA [N, H, W, C], C = 1 or 3 -> uint8 CUDA [N, 360, R, C]: sample ``r`` of degree ``a`` is the pixel the ray table
    names for step ``r + 1``, 0 past the ray's end -- the polar view of the frame that ``polar_profile``'s label map lines up with."""
    if not (torch.is_tensor(frames_u8) and frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4):
        raise ValueError('frames must be a uint8 CUDA tensor [N, H, W, C]')
    if 0 in frames_u8.shape:
        raise ValueError('empty batch or frame')
    n, h, w, c = (int(v) for v in frames_u8.shape)
    if c not in (1, 3):
        raise ValueError(f'1 or 3 channels, got {c}')
    if h * w >= 2 ** 31:
        raise ValueError(f'frame {h} x {w} has 2^31 pixels or more')
    if not frames_u8.is_cuda:
        raise ValueError('frames must be a uint8 CUDA tensor [N, H, W, C]: they are on the host, and there is no CPU path')
    frames_u8 = frames_u8.contiguous()
    pix, length = _ray_table_dev(h, w, frames_u8.device)
    R = int(pix.shape[1])
    out = torch.empty((n, ANGLES, R, c), dtype=torch.uint8, device=frames_u8.device)
    if R == 0:                                                                 # a 1 x 1 frame has no steps: nothing to gather
        return out
    with torch.cuda.device(frames_u8.device):
        L.check(L.lib().octseg_frames_unwrap(L.ptr(frames_u8), n, h, w, c, L.ptr(pix), L.ptr(length), R, L.ptr(out),
                                             L.stream_ptr()))
    return out


def _host(prof):
    if torch.is_tensor(prof):
        prof = prof.cpu().numpy()                                              # the one device-to-host copy
    prof = np.asarray(prof)
    if prof.ndim != 4 or prof.shape[2:] != (ANGLES, FIELDS):
        raise ValueError(f'prof {prof.shape} must be [N, channels, {ANGLES}, {FIELDS}]')
    return prof.astype(np.int64, copy=False)


def circular_run(flags):
    """``(arc, arc_max, arc_start)`` of a boolean vector read as a circle: the number of set entries, and length and start of the longest
    run of set entries, wrapping from the last entry to entry 0; ties go to the smallest start; all set: (n, n, 0); none: (0, 0, -1)."""
    flags = np.asarray(flags, bool)
    n = flags.size
    arc = int(flags.sum())
    if arc == 0:
        return 0, 0, -1
    if arc == n:
        return n, n, 0
    idx = np.flatnonzero(flags)
    starts = idx[~flags[idx - 1]]                                              # set with a clear predecessor (index -1 wraps)
    clear = np.flatnonzero(~flags)
    nxt = clear[np.searchsorted(clear, starts) % clear.size]                   # the first clear entry after each start, circularly
    lengths = (nxt - starts) % n
    best = int(np.argmax(lengths))                                             # the first maximum: starts ascend
    return arc, int(lengths[best]), int(starts[best])


def summarize(prof):
    """Per (slice, channel) from ``prof`` [N, channels, 360, 5] (CUDA tensor: one device-to-host copy; or numpy).  With ``met[a] = IN > 0``
    and ``t[a] = OUT - IN + 1``: ``arc`` met degrees; ``arc_max`` / ``arc_start`` the longest circular run of met degrees (``circular_run``);
    over met degrees ``thick_min`` / ``thick_max`` (ints), ``thick_median`` (numpy's median, a float) and ``depth_min`` = the smallest IN,
    the closest approach to the catheter; zeros where nothing is met.  Returns a dict of numpy arrays [N, channels]."""
    prof = _host(prof)
    n, sc = prof.shape[:2]
    out = {k: np.zeros((n, sc), np.int64) for k in ('arc', 'arc_max', 'arc_start', 'thick_min', 'thick_max', 'depth_min')}
    out['thick_median'] = np.zeros((n, sc), np.float64)
    out['arc_start'][:] = -1
    for i in range(n):
        for c in range(sc):
            met = prof[i, c, :, IN] > 0
            out['arc'][i, c], out['arc_max'][i, c], out['arc_start'][i, c] = circular_run(met)
            if met.any():
                t = (prof[i, c, :, OUT] - prof[i, c, :, IN] + 1)[met]
                out['thick_min'][i, c], out['thick_max'][i, c] = t.min(), t.max()
                out['thick_median'][i, c] = float(np.median(t))
                out['depth_min'][i, c] = prof[i, c, :, IN][met].min()
    return out


def overlap(prof, front, behind):
    """Channel ``front`` lying over channel ``behind``: ``ov[a] = met_front[a] and LAST_behind[a] > OUT_front[a]`` -- the ray leaves the first
    run of ``front`` and meets ``behind`` further out.  Per slice: ``arc`` / ``arc_max`` / ``arc_start`` of ``ov`` (``circular_run``), and over
    ``ov`` of ``t_front = OUT - IN + 1``: ``cover_min`` (int), ``cover_median`` (float) and ``cover_argmin``, the smallest degree attaining
    the minimum; 0 / 0.0 / -1 where ``ov`` is empty.  Returns a dict of numpy arrays [N]."""
    prof = _host(prof)
    n, sc = prof.shape[:2]
    front, behind = int(front), int(behind)
    if not (0 <= front < sc and 0 <= behind < sc):
        raise ValueError(f'channels {front} and {behind} of a profile with {sc}')
    out = {k: np.zeros((n,), np.int64) for k in ('arc', 'arc_max', 'arc_start', 'cover_min', 'cover_argmin')}
    out['cover_median'] = np.zeros((n,), np.float64)
    out['arc_start'][:] = -1
    out['cover_argmin'][:] = -1
    for i in range(n):
        f, b = prof[i, front], prof[i, behind]
        ov = (f[:, IN] > 0) & (b[:, LAST] > f[:, OUT])
        out['arc'][i], out['arc_max'][i], out['arc_start'][i] = circular_run(ov)
        if ov.any():
            t = np.where(ov, f[:, OUT] - f[:, IN] + 1, np.iinfo(np.int64).max)
            out['cover_argmin'][i] = int(np.argmin(t))                         # the first minimum
            out['cover_min'][i] = t[out['cover_argmin'][i]]
            out['cover_median'][i] = float(np.median(t[ov]))
    return out


def build_report(prof, h, image_names=None, ratio=None, cap='Fibrous cap', lipid='Lipid core', thin_cap=0.065, wide_arc=90):
    """``plaque_report`` from the integers (numpy or tensor [N, channels, 360, 5]) and the frame height.  Pure host."""
    prof = _host(prof)
    n, sc = prof.shape[:2]
    ratio = int(int(h) * 150 // 1000) if ratio is None else int(ratio)
    if ratio < 1:
        raise ValueError(f'ratio must be at least 1, got {ratio} (the default int(h * 150 // 1000) is 0 for frames below 7 rows)')
    for name in (cap, lipid):
        if name not in CLASS_IDS:
            raise ValueError(f'unknown class {name!r}')
    image_names = [str(i) for i in range(n)] if image_names is None else [str(s) for s in image_names]
    if len(image_names) != n:
        raise ValueError(f'{len(image_names)} names for {n} slices')
    s = summarize(prof)
    keys = ('slice', 'arc', 'arc_max', 'arc_start', 'depth_min', 'thickness_min', 'thickness_median', 'thickness_max')
    classes = {name: {k: [] for k in keys} for name in CLASS_IDS}
    for cid, name in sorted((cid, name) for name, cid in CLASS_IDS.items()):
        ch = cid - 1
        if ch >= sc:
            continue
        obj = classes[name]
        for i in range(n):
            if s['arc'][i, ch] == 0:
                continue
            obj['slice'].append(i)
            for k in ('arc', 'arc_max', 'arc_start'):
                obj[k].append(int(s[k][i, ch]))
            obj['depth_min'].append(float(s['depth_min'][i, ch] / ratio))
            obj['thickness_min'].append(float(s['thick_min'][i, ch] / ratio))
            obj['thickness_median'].append(float(s['thick_median'][i, ch] / ratio))
            obj['thickness_max'].append(float(s['thick_max'][i, ch] / ratio))
    col = {k: [] for k in ('slice', 'arc', 'arc_max', 'arc_start', 'cap_min', 'cap_median', 'cap_argmin')}
    flagged = []
    if CLASS_IDS[cap] <= sc and CLASS_IDS[lipid] <= sc:
        o = overlap(prof, CLASS_IDS[cap] - 1, CLASS_IDS[lipid] - 1)
        for i in range(n):
            if o['arc'][i] == 0:
                continue
            col['slice'].append(i)
            for k in ('arc', 'arc_max', 'arc_start'):
                col[k].append(int(o[k][i]))
            col['cap_min'].append(float(o['cover_min'][i] / ratio))
            col['cap_median'].append(float(o['cover_median'][i] / ratio))
            col['cap_argmin'].append(int(o['cover_argmin'][i]))
            if col['cap_min'][-1] < thin_cap and col['arc_max'][-1] > wide_arc:
                flagged.append(i)
    return {'ratio': ratio, 'images': image_names, 'classes': classes, 'cap_over_lipid': col,
            'thin_cap': {'max_cap': float(thin_cap), 'min_arc': int(wide_arc), 'slice': flagged}}


def plaque_report(stack, image_names=None, ratio=None, clean=None, cap='Fibrous cap', lipid='Lipid core', thin_cap=0.065, wide_arc=90):
    """The polar reading of a mask stack on the device as a JSON-serialisable dict of plain Python ints and floats.

    ``stack`` float32 CUDA [N, H, W, channels <= 8], channel ``CLASS_IDS[name] - 1`` per class; ``image_names`` one per slice (default
    ``'0', '1', ...``); ``ratio`` defaults to ``int(h * 150 // 1000)`` as in ``analysis.build_analysis``; ``clean`` takes what
    ``analysis.analyze_stack`` takes (None, True or a dict of ``cleanup.clean_stack`` keywords) and the cleaned stack is what is profiled.
    One ``polar_profile`` call, ONE device-to-host copy of the profile, the rest is host numpy.  Keys:

    ``ratio``, ``images``;
    ``classes[name]``: for every slice where the class is met by at least one ray, ``slice``, ``arc`` (met degrees), ``arc_max`` /
    ``arc_start`` (the longest circular run of met degrees, wrapping 359 -> 0), ``depth_min`` (closest approach to the centre) and
    ``thickness_min`` / ``thickness_median`` / ``thickness_max`` of ``OUT - IN + 1``, the radial extent of the first run on the ray;
    ``cap_over_lipid``: for every slice with a degree where the ray leaves ``cap``'s first run and meets ``lipid`` further out, ``slice``,
    ``arc`` / ``arc_max`` / ``arc_start`` of those degrees and ``cap_min`` / ``cap_median`` / ``cap_argmin`` of the cap's thickness there;
    ``thin_cap = {'max_cap': thin_cap, 'min_arc': wide_arc, 'slice': [...]}``: the slices with ``cap_min < thin_cap`` and the overlap's
    ``arc_max > wide_arc``.  Lengths are step counts divided by ``ratio``; arcs are whole degrees.

    The two thresholds ``thin_cap`` and ``wide_arc`` are parameters, ``thin_cap`` in the reference's own ``ratio`` units (``dcm.shape[1] *
    150 // 1000`` steps per unit).  That calibration is the reference's and is NOT validated against a physical scale here: the flag is a
    convenience for sorting slices, not a diagnosis.
    Presence here is "met by a ray": a class enters ``classes`` when at least one of the 360 rays meets it.  That is not
    ``analyze_stack``'s rule (``0 < count < h * w`` over all pixels): an object no ray samples is absent here, a completely full mask is
    present here."""
    from .cleanup import clean_kwargs, clean_stack
    kw = clean_kwargs(clean)
    if kw is not None:
        stack = clean_stack(stack, **kw)
    prof = polar_profile(stack)
    return build_report(prof, int(stack.shape[1]), image_names, ratio=ratio, cap=cap, lipid=lipid, thin_cap=thin_cap, wide_arc=wide_arc)


def carpet_view(prof, classes):
    """The en-face map of a pullback: uint8 RGB [360, N, 3], rows are degrees, columns are slices; background (128, 128, 128), then
    ``postprocess.CLASS_COLORS_RGB`` painted in class-id order wherever the class is met (``IN > 0``): the colour-mask rule, a later id
    paints over an earlier one.  ``classes``: names from ``CLASS_IDS`` whose channel ``id - 1`` exists in ``prof``."""
    from .postprocess import CLASS_COLORS_RGB
    prof = _host(prof)
    n, sc = prof.shape[:2]
    out = np.full((ANGLES, n, 3), 128, np.uint8)
    for cl in classes:
        if cl not in CLASS_IDS or cl not in CLASS_COLORS_RGB:
            raise ValueError(f'unknown class {cl!r}')
        if CLASS_IDS[cl] > sc:
            raise ValueError(f'class {cl!r} is channel {CLASS_IDS[cl] - 1} of a profile with {sc}')
    for cl in sorted(classes, key=lambda c: CLASS_IDS[c]):
        out[(prof[:, CLASS_IDS[cl] - 1, :, IN] > 0).T] = CLASS_COLORS_RGB[cl]
    return out
