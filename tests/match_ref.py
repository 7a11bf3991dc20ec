"""Host restatement of the lesion matching (``oct_segmentation_amd/match.py``, ``csrc/match.hip``) for the tests: numpy and
scipy only, independent of the package's wrappers and of the kernels.

Labels and tables come from ``lesions_ref`` (scipy.ndimage.label with the explicit 3 x 3 x 3 structure).  The RANK of a set voxel is the row of its
lesion in the ranked table (voxels descending, first voxel ascending), 0..31, or 32 for a lesion beyond the 32 listed; ``overlap`` is accumulated by
``np.add.at`` over the ranks of the voxels both sides set; ``frames`` are plain sums.  ``scores`` is an independent, loop-and-boolean-mask
implementation of what ``match.build_match`` reports.  ``CASES`` are the stack pairs the GPU test runs; the CPU test proves this file on every one
of them against sklearn's contingency_matrix.
"""
import numpy as np
from scipy import ndimage

import lesions_ref as LR

TOPL = 32
RANKS = TOPL + 1


def rank_volume(vol, across):
    """(int64 [N, H, W]: the rank 0..32 of every set voxel, -1 where clear; nles; top int32 [32, 8])."""
    lab, nles, top, _ = LR.analyse(vol, across)
    rank = np.full(lab.shape, TOPL, np.int64)
    k = min(nles, TOPL)
    if k:
        listed = top[:k, 1].astype(np.int64) + 1                   # the labels of the ranked lesions
        order = np.argsort(listed)
        at = np.minimum(np.searchsorted(listed[order], lab), k - 1)
        hit = listed[order][at] == lab
        rank[hit] = order[at][hit]
    rank[lab == 0] = -1
    return rank, nles, top


def tables(pred, truth, across='overlap'):
    """(nles int32 [channels, 2], top int32 [channels, 2, 32, 8], overlap int32 [channels, 33, 33], frames int32 [channels, N, 3]) of two stacks
    [N, H, W, channels]."""
    pred, truth = np.asarray(pred), np.asarray(truth)
    assert pred.shape == truth.shape and pred.ndim == 4
    n, h, w, sc = pred.shape
    nles = np.zeros((sc, 2), np.int32)
    top = np.zeros((sc, 2, TOPL, 8), np.int32)
    overlap = np.zeros((sc, RANKS, RANKS), np.int32)
    frames = np.zeros((sc, n, 3), np.int32)
    for c in range(sc):
        p, t = pred[..., c] != 0, truth[..., c] != 0
        rp, nles[c, 0], top[c, 0] = rank_volume(p, across)
        rt, nles[c, 1], top[c, 1] = rank_volume(t, across)
        both = p & t
        np.add.at(overlap[c], (rp[both], rt[both]), 1)
        frames[c, :, 0] = both.reshape(n, -1).sum(axis=1)
        frames[c, :, 1] = p.reshape(n, -1).sum(axis=1)
        frames[c, :, 2] = t.reshape(n, -1).sum(axis=1)
    return nles, top, overlap, frames


_tables = {}


def case_tables(name, across):
    """``tables`` of ``CASES[name]``, computed once per process and rule.  Read-only."""
    key = (name, across)
    if key not in _tables:
        out = tables(*case(name), across)
        for a in out:
            a.setflags(write=False)
        _tables[key] = out
    return _tables[key]


def contingency_by_rank(pred_vol, truth_vol, across):
    """The same 33 x 33 table by another road: sklearn's contingency matrix of the two canonical labellings, re-indexed by rank, with the rest row
    and column summed and the background row and column dropped."""
    from sklearn.metrics.cluster import contingency_matrix
    lp, lt = LR.canonical_labels(pred_vol, across), LR.canonical_labels(truth_vol, across)
    cm = np.asarray(contingency_matrix(lp.reshape(-1), lt.reshape(-1)))           # rows: np.unique(lp), columns: np.unique(lt)
    out = np.zeros((RANKS, RANKS), np.int64)

    def rank_of(labels, vol):
        order = {r[1] + 1: i for i, r in enumerate(LR.lesions(vol, across))}      # label -> place in the full ranking
        return [-1 if v == 0 else min(order[int(v)], TOPL) for v in labels]
    ri, rj = rank_of(np.unique(lp), pred_vol), rank_of(np.unique(lt), truth_vol)
    for a, i in enumerate(ri):
        for b, j in enumerate(rj):
            if i >= 0 and j >= 0:
                out[i, j] += int(cm[a, b])
    return out


# ---- the scores, independently of match.build_match: loops and boolean masks
def _div(a, b):
    return float(a) / float(b) if b else None


def scores(nles, top, overlap, frames, criterion='iou', iou=0.5, min_overlap=1, min_pixels=1):
    """Per channel (a list, in channel order) the numbers ``build_match`` must report."""
    out = []
    for c in range(len(nles)):
        n_pred, n_truth = int(nles[c][0]), int(nles[c][1])
        rp, rt = min(n_pred, TOPL), min(n_truth, TOPL)
        pairs = []
        matched_p, matched_t, ious = set(), set(), []
        for i in range(rp):
            for j in range(rt):
                inter = int(overlap[c][i][j])
                if inter == 0:
                    continue
                vp, vt = int(top[c][0][i][0]), int(top[c][1][j][0])
                union = vp + vt - inter
                pairs.append({'pred': i, 'truth': j, 'intersection': inter, 'iou': inter / union, 'dice': 2 * inter / (vp + vt),
                              'length_pred': int(top[c][0][i][3]) - int(top[c][0][i][2]) + 1,
                              'length_truth': int(top[c][1][j][3]) - int(top[c][1][j][2]) + 1,
                              'start_offset': int(top[c][0][i][2]) - int(top[c][1][j][2]),
                              'end_offset': int(top[c][0][i][3]) - int(top[c][1][j][3])})
                hit = 2 * inter > union if iou == 0.5 else inter > iou * union
                if hit:
                    assert i not in matched_p and j not in matched_t             # above one half a lesion has one partner at most
                    matched_p.add(i)
                    matched_t.add(j)
                    ious.append(inter / union)
        res = {'n_pred': n_pred, 'n_truth': n_truth, 'truncated': n_pred > TOPL or n_truth > TOPL, 'pairs': pairs,
               'unranked_overlap': {'pred_rest': sum(int(v) for v in overlap[c][TOPL]), 'truth_rest': sum(int(row[TOPL]) for row in overlap[c])}}
        if criterion == 'iou':
            tp = len(ious)
            fp, fn = rp - tp, rt - tp
            sq, rq = _div(sum(ious), tp), _div(tp, tp + 0.5 * fp + 0.5 * fn)
            res.update(tp=tp, fp=fp, fn=fn, sensitivity=_div(tp, tp + fn), precision=_div(tp, tp + fp), f1=_div(2 * tp, 2 * tp + fp + fn), sq=sq, rq=rq,
                       pq=None if sq is None or rq is None else sq * rq)
        else:
            detected = sum(1 for j in range(rt) if sum(int(overlap[c][i][j]) for i in range(RANKS)) >= min_overlap)
            true_pos = sum(1 for i in range(rp) if sum(int(overlap[c][i][j]) for j in range(RANKS)) >= min_overlap)
            res.update(detected=detected, missed=rt - detected, false_positives=rp - true_pos, sensitivity=_div(detected, rt),
                       precision=_div(true_pos, rp))
        res['split'] = sum(1 for j in range(rt) if sum(1 for i in range(rp) if overlap[c][i][j] > 0) >= 2)
        res['merged'] = sum(1 for i in range(rp) if sum(1 for j in range(rt) if overlap[c][i][j] > 0) >= 2)
        tot = [sum(int(f[k]) for f in frames[c]) for k in range(3)]
        res['voxel_dice'] = _div(2 * tot[0], tot[1] + tot[2])
        fr = {'tp': 0, 'fp': 0, 'fn': 0, 'tn': 0}
        dice = []
        for f in frames[c]:
            has_p, has_t = int(f[1]) >= min_pixels, int(f[2]) >= min_pixels
            fr['tp' if has_p and has_t else 'fp' if has_p else 'fn' if has_t else 'tn'] += 1
            dice.append(_div(2 * int(f[0]), int(f[1]) + int(f[2])))
        fr['sensitivity'], fr['specificity'], fr['dice'] = _div(fr['tp'], fr['tp'] + fr['fn']), _div(fr['tn'], fr['tn'] + fr['fp']), dice
        res['frames'] = fr
        out.append(res)
    return out


def assert_report_equals_scores(report, want, classes):
    """Every number of ``scores`` stands in ``build_match``'s report under the same key, equal (the report may say more)."""
    def same(a, b, where):
        if isinstance(b, dict):
            for k in b:
                same(a[k], b[k], f'{where}.{k}')
        elif isinstance(b, list) and b and isinstance(b[0], dict):
            assert len(a) == len(b), where
            for q, (x, y) in enumerate(zip(a, b)):
                same(x, y, f'{where}[{q}]')
        else:
            assert a == b and type(a) is type(b), (where, a, b)
    assert list(report) == list(classes)
    for name, w in zip(classes, want):
        same(report[name], w, name)


# ---- the stack pairs of the GPU test: name -> () -> (pred, truth), float32 [N, H, W, channels]
def _stack(*vols):
    return np.stack([np.asarray(v, np.float32) for v in vols], axis=-1)


def _blobs(rng, n, h, w, count):
    """A few boxes and discs that live over several slices."""
    v = np.zeros((n, h, w), bool)
    yy, xx = np.mgrid[:h, :w]
    for _ in range(count):
        z0 = rng.randint(0, n)
        z1 = rng.randint(z0, n) + 1
        cy, cx, r = rng.randint(0, h), rng.randint(0, w), rng.randint(1, max(2, min(h, w) // 3 + 2))
        shape = (np.abs(yy - cy) <= r) & (np.abs(xx - cx) <= 2 * r) if rng.rand() < 0.5 else (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        v[z0:z1] |= shape
    return v


def _shift(v, dy, dx):
    out = np.zeros_like(v)
    h, w = v.shape[1:]
    ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
    xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    out[:, yd, xd] = v[:, ys, xs]
    return out


def _drop_some(v, every):
    """The volume without every ``every``-th of its lesions (in ranking order)."""
    lab = LR.canonical_labels(v)
    gone = [r[1] + 1 for r in LR.lesions(v)][::every]
    return v & ~np.isin(lab, gone)


def seeded(n, h, w):
    """Four channels: truth blobs against a jittered, an eroded, a partly deleted and a noisy copy."""
    def make():
        rng = np.random.RandomState(7 + 100000 * n + 1000 * h + w)
        t = [_blobs(rng, n, h, w, 5) for _ in range(3)] + [rng.rand(n, h, w) < 0.4]
        p = [_shift(t[0], min(1, h - 1), min(2, w - 1)),
             ndimage.binary_erosion(t[1], structure=np.ones((1, 1, 3), bool)),
             _drop_some(t[2], 2),
             t[3] ^ (rng.rand(n, h, w) < 0.1)]
        return _stack(*p), _stack(*t)
    return make


def _two_rows(h, w, y, x0, x1):
    """A lesion of two rows whose root is NOT the start of its second row's run: the row above starts one pixel earlier."""
    v = np.zeros((1, h, w), bool)
    v[0, y - 1, x0 - 1:x1] = True
    v[0, y, x0:x1] = True
    return v


def inner_runs():
    """Runs of the intersection that start 3 pixels inside a longer run of the other side: in a word's middle (x 10..40 against 13..30), across
    a word boundary (50..80 against 53..70), and the same with the sides swapped in channel 1.  The longer run's lesion has its root in the row
    above, so the run start is not the root and a pixel inside the run is two hops away."""
    h, w = 6, 130
    long_ = _two_rows(h, w, 2, 10, 41) | _two_rows(h, w, 5, 50, 81)
    short = _two_rows(h, w, 2, 13, 31) | _two_rows(h, w, 5, 53, 71)
    short[0, 1] = False                                  # the short side keeps its second row only; rows 1 and 4 differ between the sides
    short[0, 4] = False
    return _stack(short, long_), _stack(long_, short)


def cover_two():
    """One predicted lesion over two truth lesions (merged) in channel 0 and the reverse (split) in channel 1."""
    n, h, w = 2, 8, 70
    one = np.zeros((n, h, w), bool)
    one[:, 2:6, 5:68] = True
    two = np.zeros((n, h, w), bool)
    two[:, 2:6, 8:30] = True
    two[:, 3:5, 40:66] = True
    return _stack(one, two), _stack(two, one)


def thirty_four():
    """34 lesions of 6 voxels per side, no two of a side in contact: ranking ties go by first voxel and the last two fill the rest row / column.
    Pred is truth moved one pixel right, so lesion k overlaps lesion k only."""
    n, h, w = 2, 24, 140
    v = np.zeros((n, h, w), bool)
    spots = [(z, y + 3 * z, x) for z in range(n) for y in (1, 7, 13, 19) for x in (2, 40, 62, 100, 130)][:34]
    for z, y, x in spots:
        v[z, y:y + 2, x:x + 3] = True
    return _stack(_shift(v, 0, 1)), _stack(v)


def late_join():
    """Truth: two columns that join in the last slice only (one lesion); pred: the same without the bridge (two lesions)."""
    n, h, w = 5, 9, 65
    t = np.zeros((n, h, w), bool)
    t[:, 2:h - 2, 3] = True
    t[:, 2:h - 2, w - 4] = True
    p = t.copy()
    t[n - 1, h - 3, 3:w - 3] = True
    return _stack(p, t), _stack(t, p)


def _designed(kind, n=2, h=5, w=65):
    def make():
        rng = np.random.RandomState(11)
        t = _blobs(rng, n, h, w, 4)
        o = _blobs(rng, n, h, w, 4)
        if kind == 'same':
            return _stack(t, o), _stack(t, o)
        if kind == 'disjoint':
            return _stack(t & ~o, o), _stack(o & ~t, ~o)
        if kind == 'empty':                             # one side empty, either way
            return _stack(np.zeros_like(t), t, np.zeros_like(t)), _stack(t, np.zeros_like(t), np.zeros_like(t))
        assert kind == 'full'                           # one side full, either way, and both
        return _stack(np.ones_like(t), t, np.ones_like(t)), _stack(t, np.ones_like(t), np.ones_like(t))
    return make


def straddle():
    """H * W64 = 15 words per slice and 75 per channel: the 64 words of a wave straddle slices, and the stack's second wave two channels."""
    rng = np.random.RandomState(5)
    t = rng.rand(5, 5, 130, 2) < 0.3
    p = t ^ (rng.rand(5, 5, 130, 2) < 0.15)
    return p.astype(np.float32), t.astype(np.float32)


CASES = {'same': _designed('same'), 'disjoint': _designed('disjoint'), 'empty': _designed('empty'), 'full': _designed('full'),
         'inner_runs': inner_runs, 'cover_two': cover_two, 'thirty_four': thirty_four, 'late_join': late_join, 'straddle': straddle}
for _n, _h, _w in ((1, 1, 1), (2, 1, 63), (5, 1, 64), (1, 7, 65), (2, 3, 129), (5, 37, 63), (2, 9, 64), (5, 4, 65), (1, 1, 129), (5, 70, 129)):
    CASES[f'seeded_{_n}x{_h}x{_w}'] = seeded(_n, _h, _w)

_cases = {}


def case(name):
    """(pred, truth) of a case, built once per process.  Read-only."""
    if name not in _cases:
        p, t = CASES[name]()
        p.setflags(write=False)
        t.setflags(write=False)
        _cases[name] = (p, t)
    return _cases[name]
