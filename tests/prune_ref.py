"""Host restatement of the centreline pruning kernels (csrc/prune.hip), written from the header comments of include/octseg.h.  numpy only, every
rule applied to whole arrays; nothing here is shared with oct_segmentation_amd/skeleton.py.  tests/test_prune.py holds it to scipy.ndimage's
conditional dilation, propagation and component counts and to hand cases.

    t = tips(m)                                      # the eight end-point structuring elements of morphological pruning
    x = erode(m, n)                                  # n passes of m <- m \\ tips(m), stopping at the first pass without a tip
    d = grow(d, n, a)                                # n passes of d <- d | (dil8(d) & a)
    out, restored = prune(a, spur, trim)             # the pruned plane and the pixels returned because their component would have vanished
    row = census(a, spur, trim)                      # int32 [9]: COLUMNS
    out, cen = prune_stack(stack, spur, trim)        # float32 [N, H, W, C] 0 / 1 and int32 [N, C, 9]

Planes are [H, W], stacks [N, H, W, C], anything != 0 set, everything outside the frame clear.
"""
import numpy as np

COLUMNS = ('pixels', 'pruned', 'tips', 'ends', 'junctions', 'isolated', 'orth', 'diag', 'restored')


def neighbours(m):
    """P2 .. P9 of every pixel, clockwise from north: (y-1, x), (y-1, x+1), (y, x+1), (y+1, x+1), (y+1, x), (y+1, x-1), (y, x-1), (y-1, x-1)."""
    p = np.pad(np.asarray(m, bool), 1, constant_values=False)
    return (p[:-2, 1:-1], p[:-2, 2:], p[1:-1, 2:], p[2:, 2:], p[2:, 1:-1], p[2:, :-2], p[1:-1, :-2], p[:-2, :-2])


def tips(m):
    """The set pixels that are tips.  Orthogonal form, for each of the four orthogonal directions d: the neighbour at d is set and the five
    neighbours other than d and d's two adjacent diagonals are clear.  Diagonal form: no orthogonal neighbour and exactly one diagonal one."""
    m = np.asarray(m, bool)
    p2, p3, p4, p5, p6, p7, p8, p9 = neighbours(m)
    north = p2 & ~(p4 | p5 | p6 | p7 | p8)
    east = p4 & ~(p6 | p7 | p8 | p9 | p2)
    south = p6 & ~(p8 | p9 | p2 | p3 | p4)
    west = p8 & ~(p2 | p3 | p4 | p5 | p6)
    ndiag = p3.astype(np.int32) + p5 + p7 + p9
    diag = ~(p2 | p4 | p6 | p8) & (ndiag == 1)
    return m & (north | east | south | west | diag)


def erode(m, n):
    m = np.array(m, bool)
    for _ in range(int(n)):
        t = tips(m)
        if not t.any():
            break
        m &= ~t
    return m


def dil8(d):
    p = np.pad(np.asarray(d, bool), 1, constant_values=False)
    out = np.zeros(np.asarray(d).shape, bool)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + out.shape[0], dx:dx + out.shape[1]]
    return out


def grow(d, n, a):
    d = np.array(d, bool)
    a = np.asarray(a, bool)
    for _ in range(int(n)):
        more = dil8(d) & a & ~d
        if not more.any():                                   # a fixed point: the remaining passes add nothing either
            break
        d |= more
    return d


def reach(z, a):
    """The union of the 8-connected components of ``a`` that meet ``z`` (``z`` a subset of ``a``): ``grow`` until a pass adds nothing."""
    d = np.array(z, bool)
    a = np.asarray(a, bool)
    while True:
        more = dil8(d) & a & ~d
        if not more.any():
            return d
        d |= more


def stages(a, spur, trim):
    """``(x, y, z, r)`` of the definition: X = erode(A, spur), Y = X | grow(tips(X), spur, A) (A for spur == 0), Z = erode(Y, trim), R = the
    components of A that meet Z."""
    a = np.asarray(a) != 0
    if spur > 0:
        x = erode(a, spur)
        y = x | grow(tips(x), spur, a)
    else:
        x, y = a.copy(), a.copy()
    z = erode(y, trim)
    return x, y, z, reach(z, a)


def _prune_box(a, spur, trim):
    _, _, z, r = stages(a, spur, trim)
    restored = a & ~r
    return z | restored, restored


def prune(a, spur, trim):
    """``(out, restored)`` of one plane.  Everything outside the bounding box of the set pixels is clear and stays clear, so the work is done on
    that box: the padding of ``neighbours`` and ``dil8`` is the clear ring around it."""
    a = np.asarray(a) != 0
    out = np.zeros(a.shape, bool)
    rest = np.zeros(a.shape, bool)
    if a.any():
        ys, xs = np.nonzero(a)
        box = (slice(ys.min(), ys.max() + 1), slice(xs.min(), xs.max() + 1))
        out[box], rest[box] = _prune_box(a[box], int(spur), int(trim))
    return out, rest


def links(m):
    """``(orth, diag)``: the pairs of 4-adjacent set pixels; the pairs of diagonally adjacent set pixels whose two common 4-neighbours are clear."""
    m = np.asarray(m, bool)
    _, _, e, se, s, sw, w, _ = neighbours(m)
    orth = (m & e).sum() + (m & s).sum()
    diag = (m & se & ~e & ~s).sum() + (m & sw & ~w & ~s).sum()
    return int(orth), int(diag)


def neighbour_count(m):
    return sum(v.astype(np.int32) for v in neighbours(m))


def census(a, spur, trim, pruned=None):
    a = np.asarray(a) != 0
    out, rest = prune(a, spur, trim) if pruned is None else pruned
    k = neighbour_count(out)
    orth, diag = links(out)
    return np.array([a.sum(), out.sum(), tips(out).sum(), (out & (k == 1)).sum(), (out & (k >= 3)).sum(), (out & (k == 0)).sum(), orth, diag,
                     rest.sum()], np.int32)


def prune_stack(stack, spur, trim):
    """``(out, census)``: float32 [N, H, W, C] 0.0 / 1.0 and int32 [N, C, 9]."""
    stack = np.asarray(stack) != 0
    n, h, w, c = stack.shape
    out = np.zeros(stack.shape, np.float32)
    cen = np.zeros((n, c, 9), np.int32)
    for i in range(n):
        for k in range(c):
            p = prune(stack[i, :, :, k], spur, trim)
            out[i, :, :, k] = p[0]
            cen[i, k] = census(stack[i, :, :, k], spur, trim, p)
    return out, cen


def length(cen):
    """``orth + sqrt(2) * diag`` in float64."""
    cen = np.asarray(cen, np.int64)
    return cen[..., 6] + np.sqrt(2.0) * cen[..., 7]
