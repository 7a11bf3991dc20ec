"""Host restatement of csrc/polar.hip and of the statistics of oct_segmentation_amd/polar.py, written from the table in include/octseg.h
(octseg_stack_polar).  numpy only; the ray coordinates come from analysis_ref.ray_coords, nothing is shared with oct_segmentation_amd/polar.py:
the five fields are a per-ray scan of a boolean vector, circular runs, medians and the overlap are plain loops.

    prof, labels = profile(masks)            # masks [N, H, W, C], anything != 0 is set -> int32 [N, C, 360, 5], uint8 [N, 360, R]
"""
import math

import numpy as np

from analysis_ref import ANGLES, ray_coords

IN, OUT, LAST, HITS, RUNS = range(5)


def table_width(h, w):
    return max(int(math.sqrt(w ** 2 + h ** 2)) // 2 - 1, 0)


def scan(v):
    """v: boolean samples of steps 1 .. len(v) -> (IN, OUT, LAST, HITS, RUNS)."""
    on = np.flatnonzero(v)                      # step = index + 1
    if on.size == 0:
        return 0, 0, 0, 0, 0
    first = int(on[0]) + 1
    off = np.flatnonzero(~v[first:])            # clear steps after step `first`: step = first + 1 + index
    out = first + int(off[0]) if off.size else int(v.size)
    runs = 1 + int(np.count_nonzero(np.diff(on) > 1))
    return first, out, int(on[-1]) + 1, int(on.size), runs


def profile(masks, rays=None):
    masks = np.asarray(masks) != 0
    n, h, w, c = masks.shape
    rays = ray_coords(h, w) if rays is None else rays
    R = table_width(h, w)
    prof = np.zeros((n, c, ANGLES, 5), np.int32)
    labels = np.zeros((n, ANGLES, R), np.uint8)
    for i in range(n):
        for k in range(c):
            plane = masks[i, :, :, k]
            if not plane.any():
                continue
            for a, (ys, xs) in enumerate(rays):
                v = plane[ys, xs]
                if v.any():
                    prof[i, k, a] = scan(v)
                    labels[i, a, :v.size] |= (v.astype(np.uint8) << k).astype(np.uint8)
    return prof, labels


def unwrap(frames, rays=None):
    """uint8 [N, H, W, C] -> [N, 360, R, C] by fancy indexing, zeros past the ray's end."""
    frames = np.asarray(frames)
    n, h, w, c = frames.shape
    rays = ray_coords(h, w) if rays is None else rays
    out = np.zeros((n, ANGLES, table_width(h, w), c), frames.dtype)
    for a, (ys, xs) in enumerate(rays):
        out[:, a, :ys.size] = frames[:, ys, xs]
    return out


def circular(flags):
    """(arc, arc_max, arc_start) of a circle of booleans: ties to the smallest start, all set (n, n, 0), none (0, 0, -1)."""
    flags = [bool(f) for f in flags]
    n = len(flags)
    arc = sum(flags)
    if arc == 0:
        return 0, 0, -1
    if arc == n:
        return n, n, 0
    best, start = 0, -1
    for s in range(n):
        if flags[s] and not flags[s - 1]:
            k = 0
            while flags[(s + k) % n]:
                k += 1
            if k > best:
                best, start = k, s
    return arc, best, start


def median(values):
    v = sorted(values)
    m = len(v) // 2
    return float(v[m]) if len(v) % 2 else (v[m - 1] + v[m]) / 2.0


def summary(prof_nc):
    """One [360, 5] profile -> dict."""
    met = [a for a in range(ANGLES) if prof_nc[a][IN] > 0]
    arc, arc_max, arc_start = circular([prof_nc[a][IN] > 0 for a in range(ANGLES)])
    d = {'arc': arc, 'arc_max': arc_max, 'arc_start': arc_start, 'thick_min': 0, 'thick_max': 0, 'thick_median': 0.0, 'depth_min': 0}
    if met:
        t = [int(prof_nc[a][OUT]) - int(prof_nc[a][IN]) + 1 for a in met]
        d.update(thick_min=min(t), thick_max=max(t), thick_median=median(t), depth_min=min(int(prof_nc[a][IN]) for a in met))
    return d


def cover(front, behind):
    """Two [360, 5] profiles -> dict of the overlap 'front lying over behind'."""
    ov = [front[a][IN] > 0 and behind[a][LAST] > front[a][OUT] for a in range(ANGLES)]
    arc, arc_max, arc_start = circular(ov)
    d = {'arc': arc, 'arc_max': arc_max, 'arc_start': arc_start, 'cover_min': 0, 'cover_median': 0.0, 'cover_argmin': -1}
    if arc:
        t = {a: int(front[a][OUT]) - int(front[a][IN]) + 1 for a in range(ANGLES) if ov[a]}
        lo = min(t.values())
        d.update(cover_min=lo, cover_median=median(t.values()), cover_argmin=min(a for a in t if t[a] == lo))
    return d
