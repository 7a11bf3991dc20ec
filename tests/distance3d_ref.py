"""Host restatement of the volume distance calls (csrc/distance.hip, ``octseg_volume_*``), written from the header comments of include/octseg.h.
numpy only; nothing here is shared with oct_segmentation_amd/distance.py.  Only the per-slice map comes from ``distance_ref.edt2``.
tests/test_distance3d.py holds it to scipy.ndimage by equality (``rint(distance_transform_edt(~T, sampling=(s, 1, 1)) ** 2)`` and
``binary_erosion`` with the 6-neighbour cross and ``border_value=0``).

    b = boundary(m)                                        # m [N, H, W]: m & ~erode(m), outside the volume clear
    d2 = edt2(target, s)                                   # int32 [N, H, W], squared; NONE everywhere when the target is empty in the volume
    d2, offsets, target_count = directed(src, dst, pairs, 'boundary', 'boundary', s)
    keys = pair_min(src, dst, pairs, 'set', 'set', s)      # uint64 [P]: d2 << 32 | (z * H * W + y * W + x), all ones without a query voxel
    counts = overlap(src, dst, pairs)                      # int64 [P, 3]: |a & b|, |a|, |b|
    m = blob_volume(n, h, w, seed)                         # the test volumes both test files share: unions of ellipsoids

Stacks are [N, H, W, C], anything != 0 set; a channel is a volume [N, H, W]; ``s`` is the integer distance between slices in pixels.
"""
import numpy as np

from distance_ref import NONE
from distance_ref import edt2 as edt2_slice

_FAR = 1 << 40                       # "no target in this slice": stays above every real squared distance after (s k)^2 is added


def blob_volume(n, h, w, seed, count=3, size=1.0):
    """A seeded boolean volume [n, h, w]: the union of ``count`` random ellipsoids whose half-axes are a good part of the frame (``size`` scales
    the in-slice ones) and about the stack's depth, so that from three slices on a sizeable share of the set voxels has all six neighbours
    set.  An i.i.d. mask is nearly all boundary and would not show an erosion error."""
    rng = np.random.RandomState(seed + 7919 * n + 31 * h + w)
    zz, yy, xx = np.mgrid[:n, :h, :w].astype(np.float64)
    m = np.zeros((n, h, w), bool)
    for _ in range(count):
        cz, cy, cx = rng.uniform(0, n - 1), rng.uniform(0.25, 0.75) * (h - 1), rng.uniform(0.2, 0.8) * (w - 1)
        rz = rng.uniform(max(1.5, 0.6 * n), n + 1.0)
        ry, rx = size * rng.uniform(0.3, 0.5) * h + 1.0, size * rng.uniform(0.15, 0.3) * w + 1.0
        m |= ((zz - cz) / rz) ** 2 + ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return m


def boundary(m):
    """A set voxel is boundary unless its six neighbours are all set; a neighbour outside the volume is clear."""
    m = np.asarray(m) != 0
    p = np.pad(m, 1, constant_values=False)
    inner = (p[1:-1, 1:-1, 1:-1] & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1]
             & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return m & ~inner


def part(m, name):
    m = np.asarray(m) != 0
    if name == 'set':
        return m
    if name == 'clear':
        return ~m
    if name == 'boundary':
        return boundary(m)
    raise ValueError(name)


def edt2(t, s=1):
    """The exact squared distance ``(s dz)^2 + dy^2 + dx^2`` of every voxel to the nearest voxel of ``t``, int32 [N, H, W]: the per-slice
    map, then ``min over z' of d2_slice[z'] + (s (z - z')) ** 2`` taken offset by offset, a slice without target never added to; ``NONE``
    everywhere when ``t`` is empty."""
    t = np.asarray(t, bool)
    n = t.shape[0]
    if not t.any():
        return np.full(t.shape, NONE, np.int32)
    per = np.stack([edt2_slice(t[z]).astype(np.int64) for z in range(n)])
    per[per == NONE] = _FAR
    best = per.copy()
    for k in range(1, n):
        k2 = (s * k) ** 2
        best[k:] = np.minimum(best[k:], per[:-k] + k2)
        best[:-k] = np.minimum(best[:-k], per[k:] + k2)
    assert best.max() < NONE
    return best.astype(np.int32)


def distance_volume(stack, to, s=1):
    """int32 [N, C, H, W]."""
    stack = np.asarray(stack) != 0
    n, h, w, c = stack.shape
    out = np.empty((n, c, h, w), np.int32)
    for k in range(c):
        out[:, k] = edt2(part(stack[..., k], to), s)
    return out


def boundary_volume(stack):
    stack = np.asarray(stack) != 0
    out = np.zeros(stack.shape, np.float32)
    for k in range(stack.shape[3]):
        out[..., k] = boundary(stack[..., k])
    return out


def _volumes(src, dst, pairs, src_part, dst_part):
    src, dst = np.asarray(src) != 0, np.asarray(dst) != 0
    for a, b in pairs:
        yield part(src[..., a], src_part), part(dst[..., b], dst_part)


def directed(src, dst, pairs, src_part='boundary', dst_part='boundary', s=1):
    """``(d2, offsets, target_count)``: int64, sorted within each pair's segment; int64 [P + 1]; int64 [P]."""
    lists, tcount = [], []
    for q, t in _volumes(src, dst, pairs, src_part, dst_part):
        lists.append(np.sort(edt2(t, s)[q].astype(np.int64)))
        tcount.append(int(t.sum()))
    offsets = np.zeros((len(lists) + 1,), np.int64)
    np.cumsum([v.size for v in lists], out=offsets[1:])
    return np.concatenate(lists).astype(np.int64), offsets, np.array(tcount, np.int64)


def pair_min(src, dst, pairs, src_part='set', dst_part='set', s=1):
    """uint64 [P]: the smallest ``d2 << 32 | (z * H * W + y * W + x)`` over the query voxels; all ones without one."""
    out = []
    for q, t in _volumes(src, dst, pairs, src_part, dst_part):
        idx = np.flatnonzero(q)                                # raster order
        if idx.size == 0:
            out.append(2 ** 64 - 1)
            continue
        d = edt2(t, s).reshape(-1)[idx].astype(np.int64)
        i = int(np.flatnonzero(d == d.min())[0])               # the first voxel that attains the minimum
        out.append((int(d[i]) << 32) | int(idx[i]))
    return np.array(out, np.uint64)


def overlap(src, dst, pairs):
    """int64 [P, 3]: |a & b|, |a|, |b| of the set voxels."""
    out = [(int((a & b).sum()), int(a.sum()), int(b.sum())) for a, b in _volumes(src, dst, pairs, 'set', 'set')]
    return np.array(out, np.int64).reshape(len(pairs), 3)
