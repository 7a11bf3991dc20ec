"""The planes both pruning test files use, and their reference results computed once per process (tests/prune_ref.py).  Read-only.  The
skeletons come from tests/skeleton_cases.py, thinned by its cached reference."""
import numpy as np

import prune_ref as P
import skeleton_cases as K

PAIRS = [(1, 0), (3, 0), (8, 0), (0, 2), (0, 6), (4, 3), (20, 0)]       # (spur, trim) of the restatement test
SHAPES = K.SHAPES                                                       # 1 x 1 to 97 x 130, around the 64-pixel word

_cache = {}


def thinned(m):
    """The skeleton of one plane as bool [H, W], by the cached thinning reference."""
    return K.reference(np.asarray(m)[None, :, :, None])[0][0, :, :, 0] != 0


def skeletons():
    """(name, skeleton, kind): the skeletons of the blob planes (two seeds) and of the random planes (three densities) at every shape."""
    for h, w in SHAPES:
        for seed in (0, 1):
            yield f'{h}x{w}@blobs{seed}', thinned(K.blobs(h, w, seed)), 'blobs'
        for d in K.DENSITIES:
            yield f'{h}x{w}@{d}', thinned(K.drawn(h, w, d)), 'drawn'


def stub():
    """9 x 24: the row y = 4, x = 2 .. 21, and a 3-pixel stub above x = 10."""
    m = np.zeros((9, 24), bool)
    m[4, 2:22] = True
    m[1:4, 10] = True
    return m


def diagonal():
    """A 10-pixel diagonal."""
    m = np.zeros((12, 12), bool)
    m[np.arange(1, 11), np.arange(1, 11)] = True
    return m


def thin_ring():
    return thinned(K.hand_cases()['ring'][0])


# (plane, spur, trim) -> (output pixels, tips or None, (orth, diag), restored pixels): the values of the run made while the feature was specified
def hand_values():
    s, d = stub(), diagonal()
    return [('stub', s, 2, 0, 23, 3, (22, 0), 0), ('stub', s, 3, 0, 20, 2, (19, 0), 0), ('stub', s, 3, 2, 16, None, (15, 0), 0),
            ('stub', s, 0, 2, 17, 3, (16, 0), 0), ('stub', s, 12, 0, 23, None, (22, 0), 23), ('stub', s, 0, 12, 23, None, (22, 0), 23),
            ('diagonal', d, 2, 0, 10, None, (0, 9), 0), ('diagonal', d, 0, 2, 6, None, (0, 5), 0), ('diagonal', d, 0, 5, 10, None, (0, 9), 10)]


def seam_planes():
    """name -> plane: a stub and two row ends (one facing west, one east) on each of the columns 63 / 64 / 65, and rows and stubs on every frame
    edge.  The GPU test runs each also transposed, which puts them on the rows 63 / 64 / 65 and swaps the edges."""
    out = {}
    for c in (63, 64, 65):
        m = np.zeros((16, 140), bool)
        m[5, c - 20:c + 21] = True                                       # a row across the seam with a 3-pixel stub above column c
        m[2:5, c] = True
        m[9, c:c + 30] = True                                            # a row whose west end is on column c
        m[13, c - 30:c + 1] = True                                       # a row whose east end is on column c
        out[f'seam{c}'] = m
    m = np.zeros((20, 130), bool)
    m[0, :] = True                                                       # rows on the top and bottom edges, ends on the left and right edges
    m[1:4, 64] = True
    m[19, :] = True
    m[16:19, 65] = True
    out['edges_rows'] = m
    m = np.zeros((20, 130), bool)
    m[:, 0] = True
    m[10, 1:4] = True
    m[:, 129] = True
    m[10, 126:129] = True
    out['edges_columns'] = m
    m = np.zeros((8, 70), bool)                                          # diagonal tips into the four corners
    for i in range(4):
        m[i, i] = m[i, 69 - i] = m[7 - i, i] = m[7 - i, 69 - i] = True
    m[3, 3:67] = True                                                    # joined by a row across the word seam
    out['corners'] = m
    return out


def designed():
    """name -> (plane, [(spur, trim), ...]): the hand cases, the seam and edge planes, a raw (unthinned) blob plane, degenerate planes."""
    out = {'stub': (stub(), [(2, 0), (3, 0), (3, 2), (0, 2), (12, 0), (0, 12)]),
           'diagonal': (diagonal(), [(2, 0), (0, 2), (0, 5)]),
           'ring': (thin_ring(), [(10, 10)])}
    for name, m in seam_planes().items():
        out[name] = (m, [(3, 0), (2, 4), (0, 7), (40, 0)])
    out['raw_blobs'] = (K.blobs(70, 130, 3), [(3, 2), (0, 9)])
    out['empty'] = (np.zeros((20, 70), bool), [(3, 3)])
    out['full'] = (np.ones((20, 70), bool), [(2, 2)])
    one = np.zeros((20, 70), bool)
    one[7, 64] = True
    out['pixel'] = (one, [(1, 1)])
    pair = np.zeros((5, 130), bool)                                      # two adjacent tips across the word seam: a whole two-pixel component
    pair[2, 63:65] = True
    out['pair'] = (pair, [(1, 0), (0, 1)])
    return out


def reference(stack, spur, trim):
    """``P.prune_stack`` with the planes cached by content, so that a plane both paths or several tests use is pruned once."""
    stack = np.asarray(stack) != 0
    n, h, w, c = stack.shape
    out = np.zeros(stack.shape, np.float32)
    cen = np.zeros((n, c, 9), np.int32)
    for i in range(n):
        for k in range(c):
            m = stack[i, :, :, k]
            key = (m.shape, m.tobytes(), int(spur), int(trim))
            if key not in _cache:
                p = P.prune(m, spur, trim)
                _cache[key] = (p[0], P.census(m, spur, trim, p))
            out[i, :, :, k], cen[i, k] = _cache[key]
    return out, cen


def excerpt_skeleton():
    """float32 [3, 750, 750, 4]: the thinning reference's skeletons of ``skeleton_cases.excerpt_stack()``."""
    return K.excerpt_reference()[0]


def sparse_skeleton(side, seed):
    """The skeleton of ``skeleton_cases.sparse_large``: strokes and small blobs, so both references stay fast."""
    return thinned(K.sparse_large(side, seed=seed))


def ladder_skeleton(k):
    """The skeleton of ``skeleton_cases.ladder_plane`` at the shape that selects the register-tile size ``k``."""
    return thinned(K.ladder_plane(*K.LADDER_SHAPES[k]))
