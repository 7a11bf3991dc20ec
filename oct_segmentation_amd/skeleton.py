"""Local thickness on the GPU: the centreline of every mask plane by parallel thinning, and the width of the mask across it
(``csrc/skeleton.hip`` behind ``octseg_stack_skeleton``; the width is ``distance.directed_distances`` at the skeleton's pixels).  The reference
measures thickness along rays from the frame centre, an oblique cut wherever the object is not perpendicular to the ray; this has no counterpart
there.

    skel = skeleton_stack(stack)                               # float32 0 / 1, the input's layout
    skel, census = skeleton_stack(stack, with_census=True)     # int32 CUDA [N, channels, 6]: CENSUS_COLUMNS
    d2, offsets, counts = width_lists(stack)                   # the squared distance to the nearest clear pixel at the skeleton's pixels
    report = thickness_report(stack, names=image_names)        # per class and slice: centreline, ends, junctions, passes, width statistics

``stack`` is float32 CUDA [N, H, W, channels], any value != 0 set; a plane is one (slice, channel) pair and every pixel outside the frame is
clear.  Definitions (``include/octseg.h`` states the pixel rule in full):

* The SKELETON of a plane is Guo and Hall's two-sub-iteration parallel thinning (1989, algorithm A1): passes of sub-iteration 0 then 1, every
  deletion of a sub-iteration decided on the plane as it stood when the sub-iteration began, until a pass deletes nothing.  It keeps the number
  of 8-connected components and of holes (Zhang and Suen's rule does not: a 2 x 2 square vanishes under it and thins to one pixel here).  The
  result is unique and boolean: it EQUALS the numpy restatement of ``tests/skeleton_ref.py``.  ``passes`` counts the passes that deleted
  something.
* The CENSUS of a plane: set pixels, skeleton pixels, END points (skeleton pixels with exactly one of their 8 neighbours on the skeleton),
  JUNCTION pixels (three or more), ISOLATED pixels (none), passes.  The skeleton's pixel count stands in for the centreline length; a geodesic
  length and the pruning of spurs are out of scope.
* The WIDTH at a skeleton pixel is ``2 * sqrt(d2) - 1`` in float64 on the host, ``d2`` the squared distance from the pixel to the nearest clear
  pixel of the same plane INSIDE the frame (``distance`` with ``dst_part='clear'``, int32).  It is exact for a straight band of odd width and
  ONE SHORT for an even width: the centreline is a row of pixels, not the line between two rows, so a band of width 4 has ``d2 = 4`` on one
  side's row and reads 3.  A plane without a clear pixel has ``DIST_NONE`` and reports ``None``.
* An object that touches the frame edge is measured as if it continued beyond the edge: pixels outside the frame are no target of the distance,
  although the thinning does peel the object from the edge (outside is clear for it).  A frame-edge-aware distance is out of scope.
* With ``ratio`` given, widths are divided by it as ``analysis.py`` divides its lengths; without it they are pixels.

Planes whose padded bit image fits the 160 KiB of LDS (1024 x 1024 and somewhat beyond) are thinned there, larger ones (up to 4096 x 4096) by
the same loop over images in scratch; ``path='global'`` forces the latter at any size, the results are equal.

    python -m oct_segmentation_amd.skeleton mask_dir [save_dir]      # mask TIFFs -> save_dir/medial_thickness.json
"""
import json
import os
import sys
from glob import glob

import numpy as np
import torch

from . import _lib as L
from . import distance
from .distance import DIST_NONE, check_extents

CENSUS_COLUMNS = ('pixels', 'skeleton', 'ends', 'junctions', 'isolated', 'passes')
PATHS = {'auto': 0, 'global': 1}                 # OCTSEG_SKEL_GLOBAL
DEFAULT_SCRATCH = 512 << 20
STATS = ('median', 'mean', 'min', 'p5', 'max')


LDS_WORDS = (160 * 1024 - 16) // 8


def fits_lds(h, w):
    """Whether ``path='auto'`` thins an ``h`` x ``w`` plane from LDS: its padded bit image, ``(h + 2) * (ceil(w / 64) + 1) + 1`` 64-bit words,
    within the 160 KiB less the flags (``csrc/skeleton.hip``, ``lds_image_words``)."""
    return (int(h) + 2) * ((int(w) + 63) // 64 + 1) + 1 <= LDS_WORDS


def _flags(path):
    if path not in PATHS:
        raise ValueError(f"path must be one of {sorted(PATHS)}, got {path!r}")
    return PATHS[path]


def _run(stack, want_out, want_census, path, scratch_bytes):
    flags = _flags(path)
    stack, n, h, w, sc = distance._check(stack)
    out = torch.empty_like(stack) if want_out else None
    census = torch.empty((n, sc, 6), dtype=torch.int32, device=stack.device) if want_census else None
    lib = L.lib()
    with torch.cuda.device(stack.device):
        per_slice = int(lib.octseg_skeleton_scratch_bytes(1, h, w, sc))
        step = max(min(n, int(scratch_bytes) // per_slice), 1)
        need = int(lib.octseg_skeleton_scratch_bytes(step, h, w, sc))
        scratch = torch.empty((need,), dtype=torch.uint8, device=stack.device)
        for i in range(0, n, step):
            m = min(step, n - i)
            L.check(lib.octseg_stack_skeleton(L.ptr(stack[i:i + m]), m, h, w, sc, flags, L.ptr(scratch), need,
                                              L.ptr(out[i:i + m]) if want_out else None, L.ptr(census[i:i + m]) if want_census else None,
                                              L.stream_ptr()))
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


def _lists(stack, channels, scratch_bytes=DEFAULT_SCRATCH):
    """``(d2, offsets, census)`` of the channels listed, as ``build_thickness`` takes them."""
    skel, census = skeleton_stack(stack, with_census=True, scratch_bytes=scratch_bytes)
    d2, offsets, _ = distance.directed_distances(skel, stack, pairs=[(c, c) for c in channels], src_part='set', dst_part='clear',
                                                 scratch_bytes=scratch_bytes)
    return d2, offsets, census.cpu().numpy()[:, list(channels)]


def thickness_report(stack, classes=None, names=None, ratio=None, scratch_bytes=DEFAULT_SCRATCH):
    """Direction-free thickness per class and slice: the width of the mask across its own centreline at every centreline pixel, with the
    centreline's length in pixels and its end and junction points.  ``classes``: None = the pipeline's layout (channel ``CLASS_IDS[name] - 1``),
    or the names of the channels in order; ``names``: the image names of the slices.  Returns the dict of ``build_thickness``."""
    sc = int(distance._check(stack)[4])
    named = distance._names(classes, sc)
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


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if len(argv) not in (1, 2):
        raise SystemExit('usage: python -m oct_segmentation_amd.skeleton mask_dir [save_dir]')
    mask_dir = argv[0]
    save_dir = argv[1] if len(argv) == 2 else mask_dir
    names, masks = read_mask_dir(mask_dir)
    n, h, w, sc = masks.shape
    check_extents(n, h, w, sc)
    named = distance._names(None, sc)
    cnames = [name for _, name in named]
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
