"""Host restatement of the boundary-distance kernels (csrc/distance.hip), written from the header comments of include/octseg.h.  numpy only;
nothing here is shared with oct_segmentation_amd/distance.py.  tests/test_distance.py holds it to scipy.ndimage by equality
(``rint(distance_transform_edt(~target) ** 2)`` and ``binary_erosion`` with the 4-neighbour cross and ``border_value=0``).

    b = boundary(m)                                  # m & ~erode(m), outside the frame clear
    d2 = edt2(target)                                # int32 [H, W], squared; NONE everywhere when the target is empty
    d2, offsets, target_count = directed(src, dst, pairs, 'boundary', 'boundary')
    keys = pair_min(src, dst, pairs, 'set', 'set')   # uint64 [N, P]: d2 << 32 | (y * W + x), all ones without a query pixel
    counts = overlap(src, dst, pairs)                # int32 [N, P, 3]: |a & b|, |a|, |b|

Stacks are [N, H, W, C], anything != 0 set.
"""
import numpy as np

NONE = 0x7fffffff
_FAR = 1 << 40                       # "no target in this column": stays above every real squared distance after k^2 is added


def boundary(m):
    """``m & ~erode(m)``: a set pixel is boundary unless its four neighbours are all set; a neighbour outside the frame is clear."""
    m = np.asarray(m) != 0
    p = np.pad(m, 1, constant_values=False)
    inner = p[1:-1, 1:-1] & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
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


def column_pass(t):
    """int64 [H, W]: the vertical distance to the nearest target pixel of the same column, ``_FAR`` where the column holds none."""
    t = np.asarray(t, bool)
    h, w = t.shape
    g = np.full((h, w), _FAR, np.int64)
    d = np.full((w,), _FAR, np.int64)
    for y in range(h):                                      # down
        d = np.where(t[y], 0, np.where(d >= _FAR, _FAR, d + 1))
        g[y] = d
    d = np.full((w,), _FAR, np.int64)
    for y in range(h - 1, -1, -1):                          # up
        d = np.where(t[y], 0, np.where(d >= _FAR, _FAR, d + 1))
        g[y] = np.minimum(g[y], d)
    return g


def edt2(t):
    """The exact squared Euclidean distance of every pixel to the nearest pixel of ``t``, int32 [H, W]: the column pass, then per row
    ``min over x' of (x - x') ** 2 + g[y, x'] ** 2`` taken offset by offset; ``NONE`` everywhere when ``t`` is empty."""
    t = np.asarray(t, bool)
    h, w = t.shape
    if not t.any():
        return np.full((h, w), NONE, np.int32)
    g = column_pass(t)
    g2 = np.where(g >= _FAR, _FAR, g * g)
    best = g2.copy()
    for k in range(1, w):
        if k * k >= best.max():                             # no offset from here on can improve any pixel
            break
        best[:, k:] = np.minimum(best[:, k:], g2[:, :-k] + k * k)
        best[:, :-k] = np.minimum(best[:, :-k], g2[:, k:] + k * k)
    assert best.max() < _FAR
    return best.astype(np.int32)


def distance_stack(stack, to):
    """int32 [N, C, H, W]."""
    stack = np.asarray(stack) != 0
    n, h, w, c = stack.shape
    out = np.empty((n, c, h, w), np.int32)
    for i in range(n):
        for k in range(c):
            out[i, k] = edt2(part(stack[i, :, :, k], to))
    return out


def boundary_stack(stack):
    stack = np.asarray(stack) != 0
    out = np.zeros(stack.shape, np.float32)
    for i in range(stack.shape[0]):
        for k in range(stack.shape[3]):
            out[i, :, :, k] = boundary(stack[i, :, :, k])
    return out


def d2_at(query, target):
    """(ys, xs, d2) of the query pixels in raster order.  Every query and target pixel lies in their joint bounding box, and so does every
    column and row the two passes read for them: the transform is taken on that box only."""
    ys, xs = np.nonzero(query)
    if ys.size == 0:
        return ys, xs, np.zeros((0,), np.int64)
    if not target.any():
        return ys, xs, np.full(ys.shape, NONE, np.int64)
    ty, tx = np.nonzero(target)
    y0, y1 = min(ys.min(), ty.min()), max(ys.max(), ty.max()) + 1
    x0, x1 = min(xs.min(), tx.min()), max(xs.max(), tx.max()) + 1
    d = edt2(target[y0:y1, x0:x1])
    return ys, xs, d[ys - y0, xs - x0].astype(np.int64)


def _planes(src, dst, pairs, src_part, dst_part):
    src, dst = np.asarray(src) != 0, np.asarray(dst) != 0
    for i in range(src.shape[0]):
        for a, b in pairs:
            yield part(src[i, :, :, a], src_part), part(dst[i, :, :, b], dst_part)


def directed(src, dst, pairs, src_part='boundary', dst_part='boundary'):
    """``(d2, offsets, target_count)``: int64, sorted within each (slice, pair) segment; int64 [N * P + 1]; int32 [N, P]."""
    lists, tcount = [], []
    for q, t in _planes(src, dst, pairs, src_part, dst_part):
        lists.append(np.sort(d2_at(q, t)[2]))
        tcount.append(int(t.sum()))
    offsets = np.zeros((len(lists) + 1,), np.int64)
    np.cumsum([v.size for v in lists], out=offsets[1:])
    d2 = np.concatenate(lists) if lists else np.zeros((0,), np.int64)
    return d2.astype(np.int64), offsets, np.array(tcount, np.int32).reshape(np.asarray(src).shape[0], len(pairs))


def pair_min(src, dst, pairs, src_part='set', dst_part='set'):
    """uint64 [N, P]: the smallest ``d2 << 32 | (y * W + x)`` over the query pixels; all ones without one."""
    w = np.asarray(src).shape[2]
    out = []
    for q, t in _planes(src, dst, pairs, src_part, dst_part):
        ys, xs, d = d2_at(q, t)
        if ys.size == 0:
            out.append(2 ** 64 - 1)
            continue
        i = int(np.flatnonzero(d == d.min())[0])           # nonzero is in raster order: the first pixel that attains the minimum
        out.append((int(d[i]) << 32) | (int(ys[i]) * w + int(xs[i])))
    return np.array(out, np.uint64).reshape(np.asarray(src).shape[0], len(pairs))


def overlap(src, dst, pairs):
    """int32 [N, P, 3]: |a & b|, |a|, |b| of the set pixels."""
    out = [(int((a & b).sum()), int(a.sum()), int(b.sum())) for a, b in _planes(src, dst, pairs, 'set', 'set')]
    return np.array(out, np.int32).reshape(np.asarray(src).shape[0], len(pairs), 3)
