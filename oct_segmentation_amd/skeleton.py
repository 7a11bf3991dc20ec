"""Local thickness on the GPU: the centreline of every mask plane by parallel thinning, and the width of the mask across it
(``csrc/skeleton.hip`` behind ``octseg_stack_skeleton``; the width is ``distance.directed_distances`` at the skeleton's pixels).  The reference
measures thickness along rays from the frame centre, an oblique cut wherever the object is not perpendicular to the ray; this has no counterpart
there.

    skel = skeleton_stack(stack)                               # float32 0 / 1, the input's layout
    skel, census = skeleton_stack(stack, with_census=True)     # int32 CUDA [N, channels, 6]: CENSUS_COLUMNS
    d2, offsets, counts = width_lists(stack)                   # the squared distance to the nearest clear pixel at the skeleton's pixels
    report = thickness_report(stack, names=image_names)        # per class and slice: centreline, ends, junctions, passes, width statistics
    pruned = prune_stack(skel, spur=10, trim=20)               # side branches of at most 10 pixels removed, 20 pixels off every end that is left
    pruned, pc = prune_stack(skel, 10, 20, with_census=True)   # int32 CUDA [N, channels, 9]: PRUNE_COLUMNS
    length = centreline_length(pc)                             # float64 [N, channels]: orth + sqrt(2) * diag links, the length along the centreline
    report = thickness_report(stack, spur=10, trim=20)         # the widths at the pruned centreline; adds tips, length, removed, restored

``stack`` is float32 CUDA [N, H, W, channels], any value != 0 set; a plane is one (slice, channel) pair and every pixel outside the frame is
clear.  Definitions (``include/octseg.h`` states the pixel rule in full):

* The SKELETON of a plane is Guo and Hall's two-sub-iteration parallel thinning (1989, algorithm A1): passes of sub-iteration 0 then 1, every
  deletion of a sub-iteration decided on the plane as it stood when the sub-iteration began, until a pass deletes nothing.  It keeps the number
  of 8-connected components and of holes (Zhang and Suen's rule does not: a 2 x 2 square vanishes under it and thins to one pixel here).  The
  result is unique and boolean: it EQUALS the numpy restatement of ``tests/skeleton_ref.py``.  ``passes`` counts the passes that deleted
  something.
* The CENSUS of a plane: set pixels, skeleton pixels, END points (skeleton pixels with exactly one of their 8 neighbours on the skeleton),
  JUNCTION pixels (three or more), ISOLATED pixels (none), passes.  The length along the centreline and the pruning of spurs: PRUNING below.
* The WIDTH at a skeleton pixel is ``2 * sqrt(d2) - 1`` in float64 on the host, ``d2`` the squared distance from the pixel to the nearest clear
  pixel of the same plane INSIDE the frame (``distance`` with ``dst_part='clear'``, int32).  It is exact for a straight band of odd width and
  ONE SHORT for an even width: the centreline is a row of pixels, not the line between two rows, so a band of width 4 has ``d2 = 4`` on one
  side's row and reads 3.  A plane without a clear pixel has ``DIST_NONE`` and reports ``None``.
* An object that touches the frame edge is measured as if it continued beyond the edge: pixels outside the frame are no target of the distance,
  although the thinning does peel the object from the edge (outside is clear for it).  A frame-edge-aware distance is out of scope.
* With ``ratio`` given, widths are divided by it as ``analysis.py`` divides its lengths; without it they are pixels.

* PRUNING (``csrc/prune.hip`` behind ``octseg_stack_prune``; DESIGN.md section 5r, ``include/octseg.h`` states every rule in full).  A TIP is a
  set pixel that matches one of the eight end-point structuring elements of morphological pruning: the neighbour at an orthogonal direction
  d is set and the five neighbours other than d and d's two adjacent diagonals are clear, or no orthogonal neighbour is set and exactly one
  diagonal one is.  ``erode(X, n)`` removes the tips n times (all of a pass decided at once, stopping at a pass without a tip),
  ``grow(D, n, A)`` dilates D by 3 x 3 inside A n times.  For a plane A: ``X = erode(A, spur)``, ``Y = X | grow(tips(X), spur, A)`` (A itself
  for ``spur == 0``), ``Z = erode(Y, trim)``, R = the 8-connected components of A that meet Z, and the result is ``Z | (A & ~R)``: side
  branches of at most ``spur`` pixels go away, longer branches and the main ends keep their full length, ``trim`` pixels then come off every
  end that is left, and a component that this would erase is returned whole -- a centreline is never lost.  The result is a subset of A with
  the same components and holes and EQUALS the numpy restatement of ``tests/prune_ref.py``.  The width at the last pixel thinning leaves in
  the taper of an object's end measures the thinning rule, not the object; ``trim`` takes those pixels out of the statistics.
* The LENGTH along a centreline is ``orth + sqrt(2) * diag``: ``orth`` the pairs of 4-adjacent pixels, ``diag`` the pairs of diagonally
  adjacent pixels whose two common 4-neighbours are clear (float64 on the host, divided by ``ratio`` when given).

Planes whose padded bit image fits the 160 KiB of LDS (1024 x 1024 and somewhat beyond) are thinned there, larger ones (up to 4096 x 4096) by
the same loop over images in scratch; ``path='global'`` forces the latter at any size, the results are equal.

    python -m oct_segmentation_amd.skeleton mask_dir [save_dir]      # mask TIFFs -> save_dir/medial_thickness.json
    python -m oct_segmentation_amd.skeleton mask_dir [save_dir] spur=10 trim=20      # the same at the pruned centreline
"""
import json
import os
import re
import sys
from glob import glob

import numpy as np
import torch

from . import _lib as L
from . import distance
from .distance import DIST_NONE, check_extents

CENSUS_COLUMNS = ('pixels', 'skeleton', 'ends', 'junctions', 'isolated', 'passes')
PRUNE_COLUMNS = ('pixels', 'pruned', 'tips', 'ends', 'junctions', 'isolated', 'orth', 'diag', 'restored')
PATHS = {'auto': 0, 'global': 1}                 # OCTSEG_SKEL_GLOBAL, OCTSEG_PRUNE_GLOBAL
MAX_STEPS = 8192                                 # the interface bound of spur and trim
DEFAULT_SCRATCH = 512 << 20
STATS = ('median', 'mean', 'min', 'p5', 'max')


LDS_WORDS = (160 * 1024 - 16) // 8


def fits_lds(h, w):
    """Whether ``path='auto'`` thins an ``h`` x ``w`` plane from LDS: its padded bit image, ``(h + 2) * (ceil(w / 64) + 1) + 1`` 64-bit words,
    within the 160 KiB less the flags (``csrc/planepass.h``, ``lds_image_words``)."""
    return (int(h) + 2) * ((int(w) + 63) // 64 + 1) + 1 <= LDS_WORDS


def _flags(path):
    if path not in PATHS:
        raise ValueError(f"path must be one of {sorted(PATHS)}, got {path!r}")
    return PATHS[path]


def _chunked(size_fn, n, h, w, sc, scratch_bytes, device, call):
    """``call(i, m, scratch, need)`` for every chunk of ``m`` slices from slice ``i``: as many slices as ``scratch_bytes`` holds by ``size_fn(slices,
    h, w, sc)``, one at least; the scratch block of ``need`` bytes is allocated once."""
    with torch.cuda.device(device):
        per_slice = int(size_fn(1, h, w, sc))
        step = max(min(n, int(scratch_bytes) // per_slice), 1)
        need = int(size_fn(step, h, w, sc))
        scratch = torch.empty((need,), dtype=torch.uint8, device=device)
        for i in range(0, n, step):
            call(i, min(step, n - i), scratch, need)


def _run(stack, want_out, want_census, path, scratch_bytes):
    flags = _flags(path)
    stack, n, h, w, sc = distance._check(stack)
    out = torch.empty_like(stack) if want_out else None
    census = torch.empty((n, sc, 6), dtype=torch.int32, device=stack.device) if want_census else None
    lib = L.lib()

    def call(i, m, scratch, need):
        L.check(lib.octseg_stack_skeleton(L.ptr(stack[i:i + m]), m, h, w, sc, flags, L.ptr(scratch), need,
                                          L.ptr(out[i:i + m]) if want_out else None, L.ptr(census[i:i + m]) if want_census else None,
                                          L.stream_ptr()))
    _chunked(lib.octseg_skeleton_scratch_bytes, n, h, w, sc, scratch_bytes, stack.device, call)
    return out, census


def skeleton_stack(stack, with_census=False, path='auto', scratch_bytes=DEFAULT_SCRATCH):
    """The skeleton of every plane (module docstring): float32 0.0 / 1.0 in the input's layout, and with ``with_census`` also the census, int32
    CUDA [N, channels, 6] in the order of ``CENSUS_COLUMNS``.  The input is not modified.  ``path``: ``'auto'`` thins from LDS where the plane
    fits, ``'global'`` forces the scratch path.  Processed in chunks of slices under ``scratch_bytes`` (one slice is the smallest chunk); the
    result does not depend on the chunking."""
    out, census = _run(stack, True, bool(with_census), path, scratch_bytes)
    return (out, census) if with_census else out


def census_stack(stack, path='auto', scratch_bytes=DEFAULT_SCRATCH):
    """The census alone, int32 CUDA [N, channels, 6]: the skeleton stays in scratch as bits and is never unpacked."""
    return _run(stack, False, True, path, scratch_bytes)[1]


def _steps(spur, trim):
    out = []
    for name, v in (('spur', spur), ('trim', trim)):
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= MAX_STEPS:
            raise ValueError(f'{name} must be an integer in 0..{MAX_STEPS}, got {v!r}')
        out.append(int(v))
    return out


def prune_stack(skel, spur=0, trim=0, with_census=False, path='auto', scratch_bytes=DEFAULT_SCRATCH):
    """Every plane of ``skel`` (float32 CUDA [N, H, W, channels], meant to be ``skeleton_stack``'s result; any plane is legal) pruned (module
    docstring): float32 0.0 / 1.0 in the input's layout, and with ``with_census`` also int32 CUDA [N, channels, 9] in the order of
    ``PRUNE_COLUMNS``: input pixels, output pixels, tips, END, JUNCTION and ISOLATED points of the output, orthogonal and diagonal links,
    restored pixels (those of the components returned whole).  ``spur`` / ``trim``: 0..8192; (0, 0) returns the input's planes.  The input is
    not modified.  ``path`` as for ``skeleton_stack``.  Processed in chunks of slices under ``scratch_bytes`` (one slice is the smallest chunk);
    the result does not depend on the chunking."""
    flags = _flags(path)
    spur, trim = _steps(spur, trim)
    skel, n, h, w, sc = distance._check(skel)
    out = torch.empty_like(skel)
    census = torch.empty((n, sc, 9), dtype=torch.int32, device=skel.device) if with_census else None
    lib = L.lib()

    def call(i, m, scratch, need):
        L.check(lib.octseg_stack_prune(L.ptr(skel[i:i + m]), m, h, w, sc, spur, trim, flags, L.ptr(scratch), need, L.ptr(out[i:i + m]),
                                       L.ptr(census[i:i + m]) if with_census else None, L.stream_ptr()))
    _chunked(lib.octseg_prune_scratch_bytes, n, h, w, sc, scratch_bytes, skel.device, call)
    return (out, census) if with_census else out


def centreline_length(census):
    """``orth + sqrt(2) * diag`` of a prune census [..., 9] (tensor or array), float64 numpy [...]: the length along the centreline in pixels."""
    cen = census.cpu().numpy() if torch.is_tensor(census) else np.asarray(census)
    if cen.ndim < 1 or cen.shape[-1] != len(PRUNE_COLUMNS):
        raise ValueError(f'census {cen.shape} must end in {len(PRUNE_COLUMNS)} columns')
    return cen[..., 6].astype(np.float64) + np.sqrt(2.0) * cen[..., 7].astype(np.float64)


def width_lists(stack, skeleton=None, scratch_bytes=DEFAULT_SCRATCH):
    """``(d2, offsets, counts)`` per (slice, channel): ``d2`` int64 numpy, the SQUARED distances from the skeleton's pixels to the nearest clear
    pixel of the same plane, segment ``s = slice * channels + channel`` = ``d2[offsets[s]:offsets[s + 1]]`` in ascending order; ``offsets``
    int64 [N * channels + 1]; ``counts`` int32 [N, channels], the clear pixels of each plane (0: the values are ``DIST_NONE``).  ``skeleton``:
    the result of ``skeleton_stack(stack)`` when the caller already has it.  This is ``distance.directed_distances(skeleton, stack, src_part=
    'set', dst_part='clear')``: no distance code of its own."""
    if skeleton is None:
        skeleton = skeleton_stack(stack, scratch_bytes=scratch_bytes)
    sc = int(distance._check(stack)[4])
    return distance.directed_distances(skeleton, stack, pairs=[(c, c) for c in range(sc)], src_part='set', dst_part='clear',
                                       scratch_bytes=scratch_bytes)


def build_thickness(d2, offsets, census, classes, names=None, ratio=None):
    """The report of ``thickness_report`` from the integers.  Pure host, float64 numpy.  ``d2`` / ``offsets``: the sorted lists of ``width_lists``
    restricted to the P channels reported, segment ``slice * P + k``; ``census`` int [N, P, 6]; ``classes`` the P names; ``names`` the N image
    names (optional).  Returns ``{name: {'slice', ['image',] 'centreline', 'ends', 'junctions', 'passes', 'median', 'mean', 'min', 'p5',
    'max'}}``, every value a list with one entry per slice WHERE THE CLASS IS PRESENT: ``centreline`` the skeleton pixels, the five statistics
    of the width ``2 * sqrt(d2) - 1`` over them (``p5`` = ``np.percentile(., 5)``, linear interpolation), divided by ``ratio`` when given and
    ``None`` on a plane without a clear pixel (module docstring)."""
    d2 = np.asarray(d2, np.int64)
    offsets = np.asarray(offsets, np.int64)
    census = np.asarray(census, np.int64)
    classes = [str(c) for c in classes]
    if census.ndim != 3 or census.shape[1:] != (len(classes), 6):
        raise ValueError(f'census {census.shape} must be [N, {len(classes)}, 6]')
    n, p = census.shape[:2]
    if offsets.shape != (n * p + 1,) or offsets[-1] != d2.size:
        raise ValueError('offsets must be [N * P + 1] and end at the length of the list')
    if not np.array_equal(np.diff(offsets), census[:, :, 1].reshape(-1)):
        raise ValueError('the segments of the list must hold one value per skeleton pixel of the census')
    if names is not None and len(names) != n:
        raise ValueError(f'{len(names)} names for {n} slices')
    if ratio is not None and not float(ratio) > 0:
        raise ValueError(f'ratio must be positive, got {ratio}')
    scale = 1.0 if ratio is None else 1.0 / float(ratio)
    keys = ('slice',) + (('image',) if names is not None else ()) + ('centreline', 'ends', 'junctions', 'passes') + STATS
    out = {name: {k: [] for k in keys} for name in classes}
    for i in range(n):
        for k, name in enumerate(classes):
            pixels, skel, ends, junctions, _, passes = (int(v) for v in census[i, k])
            if pixels == 0:
                continue
            col = out[name]
            col['slice'].append(i)
            if names is not None:
                col['image'].append(str(names[i]))
            col['centreline'].append(skel)
            col['ends'].append(ends)
            col['junctions'].append(junctions)
            col['passes'].append(passes)
            seg = d2[offsets[i * p + k]:offsets[i * p + k + 1]]
            if seg.size == 0 or seg[-1] >= DIST_NONE:
                for s in STATS:
                    col[s].append(None)
                continue
            wd = (2.0 * np.sqrt(seg.astype(np.float64)) - 1.0) * scale
            for s, v in zip(STATS, (np.median(wd), wd.mean(), wd.min(), np.percentile(wd, 5), wd.max())):
                col[s].append(float(v))
    return out


def build_pruned_thickness(d2, offsets, census, pruned, classes, names=None, ratio=None):
    """The report of ``thickness_report(spur=, trim=)`` from the integers.  Pure host.  ``d2`` / ``offsets``: the sorted lists of the squared
    distances at the PRUNED centreline's pixels, segment ``slice * P + k``; ``census`` int [N, P, 6] the skeleton's (``CENSUS_COLUMNS``);
    ``pruned`` int [N, P, 9] the pruned centreline's (``PRUNE_COLUMNS``), its input the skeleton.  Returns ``build_thickness``'s dict with
    ``centreline``, ``ends`` and ``junctions`` describing the pruned centreline, plus, per slice where the class is present: ``tips``,
    ``length`` (``orth + sqrt(2) * diag``, divided by ``ratio`` when given), ``removed`` (skeleton pixels pruned away) and ``restored``
    (pixels of components returned whole because pruning would have erased them)."""
    census = np.asarray(census, np.int64)
    pruned = np.asarray(pruned, np.int64)
    if census.ndim != 3 or census.shape[2] != 6 or pruned.shape != census.shape[:2] + (len(PRUNE_COLUMNS),):
        raise ValueError(f'census {census.shape} must be [N, P, 6] and the pruned census {pruned.shape} [N, P, {len(PRUNE_COLUMNS)}]')
    if not np.array_equal(pruned[:, :, 0], census[:, :, 1]):
        raise ValueError("the pruned census must count the skeleton's pixels as its input")
    both = census.copy()
    both[:, :, 1:5] = pruned[:, :, [1, 3, 4, 5]]               # pixels, ends, junctions, isolated of the pruned centreline
    out = build_thickness(d2, offsets, both, classes, names=names, ratio=ratio)
    scale = 1.0 if ratio is None else 1.0 / float(ratio)
    length = centreline_length(pruned) * scale
    for k, col in enumerate(out.values()):
        rows = col['slice']
        col['tips'] = [int(pruned[i, k, 2]) for i in rows]
        col['length'] = [float(length[i, k]) for i in rows]
        col['removed'] = [int(pruned[i, k, 0] - pruned[i, k, 1]) for i in rows]
        col['restored'] = [int(pruned[i, k, 8]) for i in rows]
    return out


def _lists(stack, channels, scratch_bytes=DEFAULT_SCRATCH):
    """``(d2, offsets, census)`` of the channels listed, as ``build_thickness`` takes them."""
    skel, census = skeleton_stack(stack, with_census=True, scratch_bytes=scratch_bytes)
    d2, offsets, _ = distance.directed_distances(skel, stack, pairs=[(c, c) for c in channels], src_part='set', dst_part='clear',
                                                 scratch_bytes=scratch_bytes)
    return d2, offsets, census.cpu().numpy()[:, list(channels)]


def _pruned_lists(stack, channels, spur, trim, scratch_bytes=DEFAULT_SCRATCH):
    """``(d2, offsets, census, pruned)`` of the channels listed, as ``build_pruned_thickness`` takes them: the skeleton goes from the thinning to
    the pruning to the distances without leaving the device."""
    skel, census = skeleton_stack(stack, with_census=True, scratch_bytes=scratch_bytes)
    cut, pruned = prune_stack(skel, spur, trim, with_census=True, scratch_bytes=scratch_bytes)
    d2, offsets, _ = distance.directed_distances(cut, stack, pairs=[(c, c) for c in channels], src_part='set', dst_part='clear',
                                                 scratch_bytes=scratch_bytes)
    return d2, offsets, census.cpu().numpy()[:, list(channels)], pruned.cpu().numpy()[:, list(channels)]


def thickness_report(stack, classes=None, names=None, ratio=None, scratch_bytes=DEFAULT_SCRATCH, spur=0, trim=0):
    """Direction-free thickness per class and slice: the width of the mask across its own centreline at every centreline pixel, with the
    centreline's length in pixels and its end and junction points.  ``classes``: None = the pipeline's layout (channel ``CLASS_IDS[name] - 1``),
    or the names of the channels in order; ``names``: the image names of the slices.  Returns the dict of ``build_thickness``.  With ``spur``
    or ``trim`` above 0 the centreline is pruned first (``prune_stack``) and the dict is ``build_pruned_thickness``'s: the widths are taken at
    the pruned centreline's pixels, ``centreline``, ``ends`` and ``junctions`` describe it, and ``tips``, ``length``, ``removed`` and
    ``restored`` are added."""
    spur, trim = _steps(spur, trim)
    sc = int(distance._check(stack)[4])
    named = distance._names(classes, sc)
    if spur or trim:
        d2, offsets, census, pruned = _pruned_lists(stack, [ch for ch, _ in named], spur, trim, scratch_bytes)
        return build_pruned_thickness(d2, offsets, census, pruned, [name for _, name in named], names=names, ratio=ratio)
    d2, offsets, census = _lists(stack, [ch for ch, _ in named], scratch_bytes)
    return build_thickness(d2, offsets, census, [name for _, name in named], names=names, ratio=ratio)


def read_mask_dir(mask_dir):
    """The mask TIFFs of a folder in sorted file-name order, as ``(names, masks)``: a uint8-valued numpy stack [N, H, W, channels]
    (``dataset.read_mask_tiff``; a 2-D mask is one channel).  All masks must share one shape."""
    from .dataset import read_mask_tiff
    paths = {os.path.basename(p): p for ext in ('*.tiff', '*.tif') for p in glob(os.path.join(mask_dir, ext))}
    if not paths:
        raise ValueError(f'no mask TIFF in {mask_dir}')
    names = sorted(paths)
    masks = []
    for k in names:
        m = np.asarray(read_mask_tiff(paths[k]))
        masks.append(m[:, :, None] if m.ndim == 2 else m)
    shapes = {m.shape for m in masks}
    if len(shapes) != 1:
        raise ValueError(f'the masks must share one shape, got {sorted(shapes)}')
    return names, np.stack(masks)


def _host_lists(masks, channels):
    """``_lists`` for a numpy stack: one upload."""
    up = torch.from_numpy(np.ascontiguousarray(np.asarray(masks) != 0).astype(np.float32)).to(torch.device('cuda'))
    return _lists(up, channels)


def _host_pruned_lists(masks, channels, spur, trim):
    """``_pruned_lists`` for a numpy stack: one upload."""
    up = torch.from_numpy(np.ascontiguousarray(np.asarray(masks) != 0).astype(np.float32)).to(torch.device('cuda'))
    return _pruned_lists(up, channels, spur, trim)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    steps = {'spur': 0, 'trim': 0}
    for word in [a for a in argv if re.fullmatch(r'(spur|trim)=\d+', str(a))]:
        argv.remove(word)
        steps[word.split('=')[0]] = int(word.split('=')[1])
    if len(argv) not in (1, 2):
        raise SystemExit('usage: python -m oct_segmentation_amd.skeleton mask_dir [save_dir] [spur=K] [trim=K]')
    spur, trim = _steps(steps['spur'], steps['trim'])
    mask_dir = argv[0]
    save_dir = argv[1] if len(argv) == 2 else mask_dir
    names, masks = read_mask_dir(mask_dir)
    n, h, w, sc = masks.shape
    check_extents(n, h, w, sc)
    named = distance._names(None, sc)
    cnames = [name for _, name in named]
    if spur or trim:
        d2, offsets, census, pruned = _host_pruned_lists(masks, [ch for ch, _ in named], spur, trim)
        report = {'images': names, 'classes': cnames, 'unit': 'pixel', 'width': '2 * sqrt(d2) - 1', 'spur': spur, 'trim': trim,
                  'thickness': build_pruned_thickness(d2, offsets, census, pruned, cnames, names=names)}
    else:
        d2, offsets, census = _host_lists(masks, [ch for ch, _ in named])
        report = {'images': names, 'classes': cnames, 'unit': 'pixel', 'width': '2 * sqrt(d2) - 1',
                  'thickness': build_thickness(d2, offsets, census, cnames, names=names)}
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, 'medial_thickness.json')
    with open(path, 'w') as f:
        json.dump(report, f, indent=1)
    print(path)
    return report


if __name__ == '__main__':
    main()
