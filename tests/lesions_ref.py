"""Host reference of the 3-D lesion feature (``oct_segmentation_amd/lesions.py``, ``csrc/lesions.hip``) for the tests: scipy and numpy only, independent
of the package's wrappers and of the kernels.

Stacks are [N, H, W, channels] as the pipeline carries them, any value != 0 set; a volume is one channel, [N, H, W].

  labels      scipy.ndimage.label with an explicit 3 x 3 x 3 structure, relabelled to 1 + n * H * W + y * W + x of the lesion's first voxel.  scipy numbers
              its labels in raster order of first encounter, so np.unique(..., return_index=True) on the flat labels gives the first voxel
  table       np.bincount for the voxels, ndimage.find_objects for the bounds, ranked by voxels descending then first voxel ascending
  profile     per-slice counts of the ranked lesions
  keep rule   t = the keep-th largest voxel count (0 with fewer lesions); a lesion stays iff voxels >= max(t, min_voxels) and its slice span
              z1 - z0 + 1 >= min_slices
"""
import os

import numpy as np
from scipy import ndimage

TOPL = 32


def structure(across):
    """overlap: 8-connected inside a slice, the same pixel between slices; full: 26-connected."""
    if across == 'full':
        return np.ones((3, 3, 3), np.int32)
    assert across == 'overlap', across
    s = np.zeros((3, 3, 3), np.int32)
    s[1] = 1
    s[0, 1, 1] = s[2, 1, 1] = 1
    return s


def _scipy_labels(vol, across):
    """(scipy's labels [N, H, W], the first voxel (flat index) of label i at [i - 1])."""
    m = np.asarray(vol) != 0
    lab, n = ndimage.label(m, structure=structure(across))
    ids, first = np.unique(lab.reshape(-1), return_index=True)
    first = first[ids > 0]
    assert first.size == n and np.all(np.diff(first) > 0)          # raster order of first encounter
    return lab, first.astype(np.int64)


def canonical_labels(vol, across='overlap'):
    """int32 [N, H, W]: 1 + the flat index of the first voxel of the voxel's lesion, 0 for background."""
    lab, first = _scipy_labels(vol, across)
    lut = np.concatenate([[0], first + 1]).astype(np.int32)
    return lut[lab]


def _rows(lab, first):
    counts = np.bincount(lab.reshape(-1), minlength=first.size + 1)
    rows = []
    for i, sl in enumerate(ndimage.find_objects(lab)):
        rows.append((int(counts[i + 1]), int(first[i]), sl[0].start, sl[0].stop - 1, sl[1].start, sl[1].stop - 1, sl[2].start, sl[2].stop - 1))
    rows.sort(key=lambda r: (-r[0], r[1]))
    return rows


def lesions(vol, across='overlap'):
    """All lesions of a volume as rows (voxels, first_voxel, z0, z1, y0, y1, x0, x1), voxels descending then first voxel ascending."""
    return _rows(*_scipy_labels(vol, across))


def threshold(voxels, keep, min_voxels=0):
    voxels = sorted((int(a) for a in voxels), reverse=True)
    t = voxels[keep - 1] if (keep > 0 and len(voxels) >= keep) else 0
    return max(t, int(min_voxels), 0)


def clean(vol, min_slices=2, min_voxels=0, keep=0, across='overlap'):
    """uint8 0 / 1 volume of the kept lesions."""
    lab = canonical_labels(vol, across)
    rows = lesions(vol, across)
    thr = threshold([r[0] for r in rows], keep, min_voxels)
    ok = [r[1] + 1 for r in rows if r[0] >= thr and r[3] - r[2] + 1 >= min_slices]
    return np.isin(lab, ok).astype(np.uint8)


def analyse(vol, across='overlap'):
    """(canonical labels, nles, top int32 [32, 8], profile int32 [32, N]) of a volume from one scipy labelling."""
    vol = np.asarray(vol)
    n = vol.shape[0]
    lab, first = _scipy_labels(vol, across)
    rows = _rows(lab, first)
    top = np.zeros((TOPL, 8), np.int32)
    rank = np.full(first.size + 1, TOPL, np.int64)                 # scipy label -> rank; TOPL = background or not ranked
    for i, r in enumerate(rows[:TOPL]):
        top[i] = r
        rank[1 + int(np.searchsorted(first, r[1]))] = i
    cell = rank[lab] * n + np.arange(n).reshape(n, 1, 1)           # (rank, slice) of every voxel
    prof = np.bincount(cell.reshape(-1), minlength=(TOPL + 1) * n)[:TOPL * n].reshape(TOPL, n).astype(np.int32)
    return np.concatenate([[0], first + 1]).astype(np.int32)[lab], len(rows), top, prof


def table(vol, across='overlap'):
    """(nles, top int32 [32, 8], profile int32 [32, N]) of a volume."""
    return analyse(vol, across)[1:]


def label_stack(stack, across='overlap'):
    """int32 [channels, N, H, W]."""
    stack = np.asarray(stack)
    return np.stack([canonical_labels(stack[..., c], across) for c in range(stack.shape[3])])


def table_stack(stack, across='overlap'):
    """(nles [channels], top [channels, 32, 8], profile [channels, 32, N])."""
    stack = np.asarray(stack)
    parts = [table(stack[..., c], across) for c in range(stack.shape[3])]
    return (np.array([p[0] for p in parts], np.int32), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]))


def clean_stack(stack, min_slices=2, min_voxels=0, keep=0, across='overlap'):
    """float32 [N, H, W, channels] of the kept lesions."""
    stack = np.asarray(stack)
    return np.stack([clean(stack[..., c], min_slices, min_voxels, keep, across) for c in range(stack.shape[3])], axis=-1).astype(np.float32)


_golden = {}


def golden_stack():
    """The demo excerpt tests/golden/pullback_demo_excerpt.npz: (bool [48, 750, 750, 4], names, the recorded get_analysis dict).  Read-only."""
    if not _golden:
        import json
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pullback_demo_excerpt.npz'))
        shape = tuple(int(v) for v in z['shape'])
        stack = np.unpackbits(z['packed'])[:int(np.prod(shape))].reshape(shape).astype(bool)
        stack.setflags(write=False)
        _golden['v'] = (stack, [str(s) for s in z['names']], json.loads(str(z['objects_json'])))
    return _golden['v']


_golden_tables = {}


def golden_table(across):
    """``table_stack`` of the demo excerpt, computed once per process and rule."""
    if across not in _golden_tables:
        _golden_tables[across] = table_stack(golden_stack()[0], across)
    return _golden_tables[across]
