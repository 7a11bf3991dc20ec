"""Host reference of the mask clean-up (``oct_segmentation_amd/cleanup.py``, ``csrc/components.hip``) for the tests: scipy and numpy only,
independent of the package's wrappers and of the kernels.

Planes are 2-D arrays, any value != 0 set; stacks are [N, H, W, channels] as the pipeline carries them.

  labels      scipy.ndimage.label with the full 3 x 3 structure, relabelled to the canonical form 1 + y * W + x of the component's first pixel
  areas       np.bincount
  filter      t = the keep-th largest area (0 with fewer components), components with area >= t stay (ties all stay), min_area drops below it
  fill        scipy.ndimage.binary_fill_holes (default structure: background 4-connected to the border stays)
  smoothing   written from the definition: loop over the footprint's offsets, anchor k // 2, no reflection, neutral value outside the frame
"""
import os

import numpy as np
from scipy import ndimage

FULL = np.ones((3, 3), np.int32)
TOPK = 8


def ellipse(n):
    """cv2.getStructuringElement(MORPH_ELLIPSE, (n, n)) restated (OpenCV 4.8.1): row i is set on [c - dx, c + dx], dx = cvRound(c * sqrt((r^2 -
    dy^2) / r^2)), r = c = n // 2, dy = i - r; written here again so that the reference does not lean on the package."""
    n = int(n)
    r = c = n // 2
    out = np.zeros((n, n), np.uint8)
    for i in range(n):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) / (r * r)))) if r else 0
            out[i, max(c - dx, 0):min(c + dx + 1, n)] = 1
    return out


def canonical_labels(plane, structure=FULL):
    """int32 [H, W]: 1 + y * W + x of the first pixel (raster order) of the pixel's component, 0 for background."""
    m = np.asarray(plane) != 0
    lab, n = ndimage.label(m, structure=structure)
    out = np.zeros(m.shape, np.int32)
    if n:
        flat = lab.reshape(-1)
        idx = np.nonzero(flat)[0]
        first = np.full(n + 1, flat.size, np.int64)
        np.minimum.at(first, flat[idx], idx)
        out.reshape(-1)[idx] = (first[flat[idx]] + 1).astype(np.int32)
    return out


def components(plane):
    """List of (area, first_pixel, x0, y0, x1, y1), area descending then first pixel ascending; all components of the plane."""
    lab = canonical_labels(plane)
    ids = np.unique(lab[lab > 0])
    rows = []
    for v in ids:
        ys, xs = np.nonzero(lab == v)
        rows.append((int(ys.size), int(v) - 1, int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())))
    rows.sort(key=lambda r: (-r[0], r[1]))
    return rows


def table(plane):
    """(ncomp, top int32 [8, 6]) of a plane."""
    rows = components(plane)
    top = np.zeros((TOPK, 6), np.int32)
    for i, r in enumerate(rows[:TOPK]):
        top[i] = r
    return len(rows), top


def threshold(areas, keep, min_area=0):
    areas = sorted((int(a) for a in areas), reverse=True)
    t = areas[keep - 1] if (keep > 0 and len(areas) >= keep) else 0
    return max(t, int(min_area), 0)


def keep_largest(plane, keep=3, min_area=0, fill_holes=True):
    """uint8 0 / 1 plane: the components with area >= threshold, then (optionally) filled."""
    lab = canonical_labels(plane)
    flat = lab.reshape(-1)
    counts = np.bincount(flat)
    ids = np.nonzero(counts)[0]
    ids = ids[ids > 0]
    thr = threshold(counts[ids], keep, min_area)
    ok = np.zeros(counts.size, bool)
    ok[ids] = counts[ids] >= thr
    out = ok[flat].reshape(lab.shape)
    if fill_holes:
        out = ndimage.binary_fill_holes(out)
    return out.astype(np.uint8)


def kept_table(plane, keep=3, min_area=0):
    """(ncomp, top) of the kept components, before the fill."""
    return table(keep_largest(plane, keep, min_area, fill_holes=False))


def _morph(plane, fp, erode):
    """One stage from the definition: out(y, x) = AND (erode) / OR (dilate) over the set footprint cells (i, j) of src(y + i - a, x + j - a),
    a = k // 2; positions outside the frame do not take part (they read as 1 for an erosion, 0 for a dilation)."""
    m = np.asarray(plane) != 0
    h, w = m.shape
    k = fp.shape[0]
    a = k // 2
    pad = np.full((h + 2 * k, w + 2 * k), bool(erode))
    pad[k:k + h, k:k + w] = m
    out = np.full((h, w), bool(erode))
    for i in range(k):
        for j in range(k):
            if fp[i, j]:
                sh = pad[k + i - a:k + i - a + h, k + j - a:k + j - a + w]
                out = (out & sh) if erode else (out | sh)
    return out


def smooth_size(h, w):
    return max(int(0.005 * min(h, w)), 1)


def smooth(plane, k=None):
    """MaskProcessor.smooth_mask: open, close, dilate = erode, dilate, dilate, erode, dilate with ellipse(k); uint8 0 / 1."""
    m = np.asarray(plane) != 0
    k = smooth_size(*m.shape) if k is None else int(k)
    if k > 1:
        fp = ellipse(k)
        for erode in (True, False, False, True, False):
            m = _morph(m, fp, erode)
    return m.astype(np.uint8)


def smooth_scipy(plane, k):
    """The same chain through scipy's rank filters (cross-check of the definition above)."""
    m = (np.asarray(plane) != 0).astype(np.uint8)
    if k > 1:
        fp = ellipse(k)
        for erode in (True, False, False, True, False):
            if erode:
                m = ndimage.minimum_filter(m, footprint=fp, mode='constant', cval=1)
            else:
                m = ndimage.maximum_filter(m, footprint=fp, mode='constant', cval=0)
    return m


def clean(plane, smooth_k=None, keep=3, min_area=0, fill_holes=True, do_smooth=True):
    m = smooth(plane, smooth_k) if do_smooth else (np.asarray(plane) != 0).astype(np.uint8)
    if keep > 0 or min_area > 1 or fill_holes:
        m = keep_largest(m, keep, min_area, fill_holes)
    return m


def per_plane(stack, fn, dtype=np.float32):
    """Apply ``fn(plane) -> [H, W]`` to every (slice, channel) plane of a stack [N, H, W, channels]; result in the stack's layout."""
    stack = np.asarray(stack)
    out = np.zeros(stack.shape, dtype)
    for n in range(stack.shape[0]):
        for c in range(stack.shape[3]):
            out[n, :, :, c] = fn(stack[n, :, :, c])
    return out


def label_stack(stack):
    """int32 [N, channels, H, W]."""
    stack = np.asarray(stack)
    return np.stack([np.stack([canonical_labels(stack[n, :, :, c]) for c in range(stack.shape[3])]) for n in range(stack.shape[0])])


def table_stack(stack, fn=table):
    stack = np.asarray(stack)
    n, _, _, ch = stack.shape
    ncomp = np.zeros((n, ch), np.int32)
    top = np.zeros((n, ch, TOPK, 6), np.int32)
    for i in range(n):
        for c in range(ch):
            ncomp[i, c], top[i, c] = fn(stack[i, :, :, c])
    return ncomp, top


def golden_planes():
    """The demo planes of tests/golden/cleanup_demo_masks.npz: (bool [P, 750, 750], 1-based file numbers, channels, components, hole pixels)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cleanup_demo_masks.npz'))
    shape = tuple(int(v) for v in z['shape'])
    planes = np.unpackbits(z['packed'])[:int(np.prod(shape))].reshape(shape).astype(bool)
    return planes, z['slices'], z['channels'], z['ncomp'], z['holes']


def salt(shape, seed, p=0.002):
    """Seeded salt noise: bool array, True with probability p."""
    return np.random.RandomState(seed).rand(*shape) < p
