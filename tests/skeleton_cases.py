"""The planes both skeleton test files use, and their reference results computed once per process (tests/skeleton_ref.py).  Read-only."""
import numpy as np
from scipy import ndimage

import skeleton_ref as R

SHAPES = [(1, 1), (1, 70), (70, 1), (33, 65), (64, 64), (97, 130)]      # around the 64-pixel word
DENSITIES = [0.3, 0.6, 0.9]


def drawn(h, w, density, seed=0):
    """A seeded boolean plane at the density."""
    rng = np.random.RandomState(seed + 7919 * h + 31 * w + int(density * 1e4))
    return rng.rand(h, w) < density


def blobs(h, w, seed=0, sigma=3.0):
    """Gaussian blobs: a smoothed seeded noise field cut at its 60th percentile -- thick objects with holes, unlike the speckle of ``drawn``."""
    rng = np.random.RandomState(seed + 104729 * h + 17 * w)
    f = ndimage.gaussian_filter(rng.rand(h, w), sigma, mode='constant')
    return f > np.percentile(f, 60)


def disc(size=97, radius=40):
    yy, xx = np.mgrid[:size, :size]
    c = size // 2
    return (yy - c) ** 2 + (xx - c) ** 2 <= radius * radius


def ring(h, w, cy, cx, r_out, r_in):
    yy, xx = np.mgrid[:h, :w]
    d = (yy - cy) ** 2 + (xx - cx) ** 2
    return (d <= r_out * r_out) & (d > r_in * r_in)


def hand_cases():
    """name -> (plane, skeleton pixels as a sorted list of (y, x) or None, passes or None): the values of the issue's run."""
    out = {}
    m = np.zeros((6, 6), bool)
    m[2:4, 2:4] = True
    out['square2'] = (m, None, None)                                     # one pixel; which one is the rule's business
    out['full9'] = (np.ones((9, 9), bool), [(4, 4)], 4)
    m = np.zeros((9, 24), bool)
    m[2:7, 2:22] = True
    out['bar5'] = (m, [(4, x) for x in range(4, 20)], 2)
    m = np.zeros((9, 24), bool)
    m[2:6, 2:22] = True
    out['bar4'] = (m, [(3, x) for x in range(4, 21)], None)
    out['row70'] = (np.ones((1, 70), bool), [(0, x) for x in range(70)], 0)
    out['full3x70'] = (np.ones((3, 70), bool), None, 1)                  # 68 pixels
    out['disc40'] = (disc(), [(48, 47), (48, 48), (48, 49)], 40)
    out['ring'] = (ring(40, 40, 20, 20, 15, 8), None, None)
    return out


def designed():
    """name -> plane: the hand cases, the degenerate planes, objects across the word seam at columns 63 / 64 / 65 and on every frame edge.  The GPU
    test runs each also transposed."""
    out = {k: v[0] for k, v in hand_cases().items()}
    out['empty'] = np.zeros((20, 70), bool)
    out['full'] = np.ones((20, 70), bool)
    one = np.zeros((20, 70), bool)
    one[7, 64] = True
    out['pixel'] = one
    bar = np.zeros((40, 140), bool)                                      # a 5-wide horizontal bar over two word seams
    bar[10:15, 3:137] = True
    bar[20:38, 62:67] = True                                             # and a 5-wide vertical one on the seam
    out['bars_on_seam'] = bar
    st = np.zeros((40, 140), bool)                                       # a one-pixel-wide diagonal staircase through columns 63 / 64 / 65
    for i in range(36):
        st[2 + i, 46 + i] = True
        st[2 + i, 47 + i] = True
    out['staircase'] = st
    for name, sl in (('edge_top', (slice(0, 6), slice(10, 120))), ('edge_bottom', (slice(24, 30), slice(10, 120))),
                     ('edge_left', (slice(3, 27), slice(0, 7))), ('edge_right', (slice(3, 27), slice(123, 130)))):
        e = np.zeros((30, 130), bool)
        e[sl] = True
        out[name] = e
    out['ring_on_seam'] = ring(60, 130, 30, 64, 25, 14)
    return out


def sparse_large(side=1280, seed=5):
    """Thin strokes and small blobs over a plane too large for LDS: a few passes only, so the reference stays fast."""
    rng = np.random.RandomState(seed)
    m = np.zeros((side, side), bool)
    for _ in range(60):
        y, x = rng.randint(8, side - 8, 2)
        r = rng.randint(1, 5)
        yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
        m[y - r:y + r + 1, x - r:x + r + 1] |= yy * yy + xx * xx <= r * r
    for _ in range(40):
        y, x = rng.randint(8, side - 300, 2)
        n, t = rng.randint(50, 280), rng.randint(1, 6)
        if rng.rand() < 0.5:
            m[y:y + t, x:x + n] = True
        else:
            m[y:y + n, x:x + t] = True
    m[0:3, 100:900] = True                                               # on the frame edge and over many words
    m[200:1100, side - 2:side] = True
    return m


# ---- one plane per register-tile size K of the LDS kernels: K -> (H, W).  owned = H * (ceil(W / 64) + 1) words over 1024 threads selects K, and
# the padded image stays within the LDS limit.  Tall and narrow: the smallest planes that reach the high K
LADDER = (1, 2, 4, 7, 10, 13, 17, 20)
LADDER_SHAPES = {2: (300, 130), 4: (800, 130), 7: (1500, 130), 10: (2300, 130), 13: (3000, 130), 17: (4000, 130), 20: (3700, 200)}


def ladder_k(h, w):
    """The K the dispatch selects for an ``h`` x ``w`` plane with more than 1024 owned words."""
    owned = h * ((w + 63) // 64 + 1)
    assert owned > 1024
    k = -(-owned // 1024)
    return min(v for v in LADDER if v >= k)


def ladder_plane(h, w, seed=3):
    """3-pixel bars along the first and the last rows (the words a thread owns first and last, next to the pad rows), two dozen strokes 1 to 5
    pixels thick, a 30 x 8 block across the column 63 / 64 seam: objects that thin in a few passes, so the reference stays fast."""
    rng = np.random.RandomState(seed + 31 * h + w)
    m = np.zeros((h, w), bool)
    m[0:3, 4:w - 4] = True
    m[h - 3:h, 4:w - 4] = True
    for _ in range(24):
        t = rng.randint(1, 6)
        if rng.rand() < 0.5:
            n = rng.randint(20, w - 20)
            y, x = rng.randint(8, h - 8 - t), rng.randint(2, w - n - 2)
            m[y:y + t, x:x + n] = True
        else:
            n = rng.randint(40, 250)
            y, x = rng.randint(8, h - 8 - n), rng.randint(2, w - t - 2)
            m[y:y + n, x:x + t] = True
    y = h // 2
    m[y:y + 30, 60:68] = True
    return m


# ---- the demo excerpt (tests/golden/pullback_demo_excerpt.npz): slices 28 - 30; channel = CLASS_IDS - 1
LUMEN, CAP, LIPID, VASA = 0, 1, 2, 3
EXCERPT_PLANES = [(28, CAP), (29, CAP), (30, CAP), (28, VASA), (29, VASA), (30, VASA), (29, LIPID), (29, LUMEN)]

_cache = {}


def excerpt_stack():
    """bool [3, 750, 750, 4]: slices 28 - 30 of the excerpt with only ``EXCERPT_PLANES`` kept (the other planes cleared: a lumen or lipid plane
    costs the numpy reference about a second each)."""
    if 'stack' not in _cache:
        import lesions_ref
        full = lesions_ref.golden_stack()[0]
        st = np.zeros((3,) + full.shape[1:], bool)
        for sl, ch in EXCERPT_PLANES:
            st[sl - 28, :, :, ch] = full[sl, :, :, ch]
        st.setflags(write=False)
        _cache['stack'] = st
    return _cache['stack']


def excerpt_reference():
    """``(out, census)`` of ``excerpt_stack()`` by the reference, once per process."""
    if 'ref' not in _cache:
        out, cen = R.skeleton_stack(excerpt_stack())
        out.setflags(write=False)
        cen.setflags(write=False)
        _cache['ref'] = (out, cen)
    return _cache['ref']


def reference(stack):
    """``R.skeleton_stack`` with the planes cached by content, so that a plane both paths or several tests use is thinned once."""
    stack = np.asarray(stack) != 0
    n, h, w, c = stack.shape
    out = np.zeros(stack.shape, np.float32)
    cen = np.zeros((n, c, 6), np.int32)
    for i in range(n):
        for k in range(c):
            m = stack[i, :, :, k]
            key = (m.shape, m.tobytes())
            if key not in _cache:
                t = R.thin(m)
                _cache[key] = (t[0], R.census(m, t))
            out[i, :, :, k], cen[i, k] = _cache[key]
    return out, cen
