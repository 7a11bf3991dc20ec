"""The restatement the contour kernels are held to: a plain sequential crack follower over the definitions of include/octseg.h
(octseg_stack_contour_counts, octseg_stack_contours).  numpy and Python loops; nothing is shared with oct_segmentation_amd.  tests/test_contours.py
proves it against scipy.ndimage.label and matplotlib.path on every case the GPU test uses."""
import numpy as np
from scipy import ndimage

FIELDS = ('plane', 'first_vertex', 'vertices', 'area', 'edges', 'x0', 'y0', 'x1', 'y1', 'label')
DX, DY = (1, 0, -1, 0), (0, 1, 0, -1)               # E, S, W, N on screen (y down)


def edge_map(mask):
    """bool [H + 1, W + 1, 4]: the directed crack edges by start vertex (y, x) and direction; its flat index is the edge id."""
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    p = np.zeros((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = mask
    ex = np.zeros((h + 1, w + 1, 4), bool)
    ex[:h, :w, 0] = mask & ~p[:-2, 1:-1]             # top side:    (x, y) -> (x + 1, y)
    ex[:h, 1:, 1] = mask & ~p[1:-1, 2:]              # right side:  (x + 1, y) -> (x + 1, y + 1)
    ex[1:, 1:, 2] = mask & ~p[2:, 1:-1]              # bottom side: (x + 1, y + 1) -> (x, y + 1)
    ex[1:, :w, 3] = mask & ~p[1:-1, :-2]             # left side:   (x, y + 1) -> (x, y)
    return ex


def first_pixel_labels(mask):
    """int64 [H, W]: 1 + y * W + x of the first raster pixel of the pixel's 8-connected component, background 0."""
    mask = np.asarray(mask) != 0
    lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))
    if n == 0:
        return np.zeros(mask.shape, np.int64)
    first = ndimage.minimum(np.arange(mask.size).reshape(mask.shape), lab, index=np.arange(1, n + 1)).astype(np.int64)
    return np.where(lab > 0, 1 + first[np.maximum(lab, 1) - 1], 0)


def trace_plane(mask):
    """The contours of one plane in leader order: a list of dicts with the table fields (without plane and first_vertex) and 'ring', the vertex
    list [[x, y], ...]."""
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    ex = edge_map(mask)
    flat = ex.ravel().tolist()
    labels = first_pixel_labels(mask)
    seen = bytearray(len(flat))
    out = []
    for lead in np.flatnonzero(ex.ravel()).tolist():               # ascending ids: the first unseen edge of a cycle is its leader
        if seen[lead]:
            continue
        cycle, e = [], lead
        while not seen[e]:
            seen[e] = 1
            cycle.append(e)
            d = e & 3
            x, y = (e >> 2) % (w + 1) + DX[d], (e >> 2) // (w + 1) + DY[d]
            base = (y * (w + 1) + x) * 4
            for nd in ((d + 3) & 3, d, (d + 1) & 3):               # the diagonal pixel's edge first: foreground 8-connected
                if flat[base + nd]:
                    e = base + nd
                    break
            else:
                raise AssertionError('an edge without a successor')
        assert e == lead, 'a cycle must close at its leader'
        ring, area2 = [], 0
        for k, e in enumerate(cycle):
            d, x, y = e & 3, (e >> 2) % (w + 1), (e >> 2) // (w + 1)
            if cycle[k - 1] & 3 != d:
                ring.append([x, y])
            area2 += x * DY[d] * 2
        xs, ys = [v[0] for v in ring], [v[1] for v in ring]
        d, x, y = lead & 3, (lead >> 2) % (w + 1), (lead >> 2) // (w + 1)
        assert d in (0, 1), 'a leader runs east (outer contour) or south (hole)'
        px, py = (x, y) if d == 0 else (x - 1, y)
        out.append({'ring': ring, 'vertices': len(ring), 'area': area2 // 2, 'edges': len(cycle), 'x0': min(xs), 'y0': min(ys), 'x1': max(xs),
                    'y1': max(ys), 'label': int(labels[py, px]), 'leader': lead})
    return out


def trace_stack(stack):
    """stack [N, H, W, C] -> (ncont int32 [N, C], table int32 [K, 10], vertices int32 [V, 2], counts int64 [N, C, 2])."""
    stack = np.asarray(stack)
    n, h, w, c = stack.shape
    ncont = np.zeros((n, c), np.int32)
    counts = np.zeros((n, c, 2), np.int64)
    rows, verts = [], []
    for i in range(n):
        for ch in range(c):
            conts = trace_plane(stack[i, :, :, ch])
            ncont[i, ch] = len(conts)
            for ct in conts:
                rows.append([i * c + ch, len(verts), ct['vertices'], ct['area'], ct['edges'], ct['x0'], ct['y0'], ct['x1'], ct['y1'], ct['label']])
                verts.extend(ct['ring'])
                counts[i, ch, 0] += ct['edges']
                counts[i, ch, 1] += ct['vertices']
    table = np.asarray(rows, np.int32).reshape(-1, len(FIELDS))
    return ncont, table, np.asarray(verts, np.int32).reshape(-1, 2), counts


# ---- the cases the tests share
def seeded_stack(h, w, seed=0, channels=(0.5, 0.01, 0.0, 1.0), n=3):
    rng = np.random.default_rng(seed + 1000 * h + w)
    return np.stack([(rng.random((n, h, w)) < d).astype(np.float32) for d in channels], axis=-1)


def spiral(h, w):
    """A one-pixel-wide arm wound inwards with one-pixel gaps (the pattern of test_gpu_cleanup.py, stated again): a single component without a
    hole whose contour is the longest cycle of the suite."""
    m = np.zeros((h, w), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    while True:
        moved = False
        for _ in range(2):
            ny, nx, ny2, nx2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= ny2 < h and 0 <= nx2 < w and m[ny2, nx2]):
                y, x = ny, nx
                m[y, x] = True
                moved = True
                break
            dy, dx = dx, -dy
        if not moved:
            return m


def patterns():
    """name -> 2-D bool mask."""
    out = {}
    yy, xx = np.mgrid[0:9, 0:11]
    out['checkerboard'] = (yy + xx) % 2 == 0
    out['staircase'] = np.eye(23, dtype=bool)
    ring = np.ones((12, 12), bool)            # three closed curves inside one another: a ring's outside, its hole, the island in the hole
    ring[2:10, 2:10] = False
    ring[4:8, 4:8] = True
    out['rings'] = ring
    out['spiral'] = spiral(130, 97)
    for n in (63, 64, 65, 127, 1023):
        out[f'bar{n}'] = np.ones((1, n), bool)
        out[f'column{n}'] = np.ones((n, 1), bool)
    frame = np.zeros((40, 70), bool)
    frame[0:25, 0:30] = True                  # meets the top and the left side
    frame[18:40, 45:70] = True                # meets the bottom and the right side
    out['frame_blobs'] = frame
    hole = np.zeros((10, 10), bool)
    hole[1:9, 1:9] = True
    hole[3, 3] = False                        # a hole whose top-left clear pixel (3, 3) has ...
    hole[2, 2] = False                        # ... a clear diagonal neighbour: vertex (3, 3) is a checkerboard vertex
    hole[4:6, 3:6] = False
    out['hole_at_checker_vertex'] = hole
    return out
