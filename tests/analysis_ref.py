"""Host restatement of the measurements of csrc/measure.hip, written from the semantics stated in include/octseg.h (the role
tests/postprocess_ref.py has for the rendering kernel).  numpy only; nothing here is shared with oct_segmentation_amd/analysis.py: the ray
coordinates are recomputed from the formula, and the walk is a per-ray scan of a boolean vector.

    counts, radii = measure(masks)           # masks: [N, H, W, C], anything != 0 is set  ->  int32 [N, C], int32 [N, C, 360]
"""
import math

import numpy as np

ANGLES = 360


def ray_coords(h, w):
    """Per degree the in-frame steps of the ray as (ys, xs) index arrays: step r = 1, 2, ... at (int(cx + r cos), int(cy + r sin)) while
    r < int(sqrt(w^2 + h^2)) // 2 and the sample is inside the frame."""
    cx, cy = w // 2, h // 2
    rmax = int(math.sqrt(w ** 2 + h ** 2)) // 2
    rays = []
    for angle in range(ANGLES):
        a = math.radians(angle)
        ys, xs = [], []
        r = 1
        while r < rmax:
            x, y = int(cx + r * math.cos(a)), int(cy + r * math.sin(a))
            if x < 0 or x >= w or y < 0 or y >= h:
                break
            ys.append(y); xs.append(x)
            r += 1
        rays.append((np.array(ys, np.int64), np.array(xs, np.int64)))
    return rays


def walk(v):
    """v: boolean samples of steps 1 .. len(v).  0 when none is set; else g - 1 for the first clear step g after the first set one, or
    len(v) when the object reaches the end of the ray."""
    on = np.flatnonzero(v)
    if on.size == 0:
        return 0
    f = on[0]                                   # step f + 1
    off = np.flatnonzero(~v[f + 1:])
    return int(f + 1 + off[0]) if off.size else int(v.size)     # g = f + 2 + off[0]; g - 1


def radii_of(mask, rays=None):
    """int32 [360] for one boolean [H, W] mask."""
    mask = np.asarray(mask) != 0
    rays = ray_coords(*mask.shape) if rays is None else rays
    return np.array([walk(mask[ys, xs]) for ys, xs in rays], np.int32)


def measure(masks):
    masks = np.asarray(masks) != 0
    n, h, w, c = masks.shape
    rays = ray_coords(h, w)
    counts = masks.reshape(n, h * w, c).sum(axis=1).astype(np.int32)
    radii = np.zeros((n, c, ANGLES), np.int32)
    for i in range(n):
        for k in range(c):
            if counts[i, k]:
                radii[i, k] = radii_of(masks[i, :, :, k], rays)
    return counts, radii


def ray_lengths(h, w):
    return np.array([len(ys) for ys, _ in ray_coords(h, w)], np.int32)


_fixtures = {}


def load_fixture(path):
    """tests/golden/pullback_demo_excerpt.npz (made by tests/golden/make_pullback_fixture.py) -> dict with the boolean stack [48, 750, 750, 4],
    the names, the recorded dict of the reference's get_analysis and, per present (slice, channel), what its calculate_object_thickness
    returned.  Loaded once per process; callers must not modify it."""
    if path not in _fixtures:
        import json
        z = np.load(path)
        shape = tuple(int(v) for v in z['shape'])
        stack = np.unpackbits(z['packed'])[:int(np.prod(shape))].reshape(shape).astype(bool)
        ends = np.cumsum(z['thick_len'])
        thick = {}
        for i, (s, c) in enumerate(zip(z['thick_slice'], z['thick_channel'])):
            thick[(int(s), int(c))] = {'median': float(z['thick_median'][i]), 'min': int(z['thick_min'][i]), 'max': int(z['thick_max'][i]),
                                       'all_measurements': [int(v) for v in z['thick_all'][ends[i] - z['thick_len'][i]:ends[i]]]}
        _fixtures[path] = {'stack': stack, 'names': [str(s) for s in z['names']], 'recorded': json.loads(str(z['objects_json'])),
                           'thickness': thick}
    return _fixtures[path]
