"""Restatement of the slice interpolation (include/octseg.h) in scipy and numpy only: it shares nothing with
oct_segmentation_amd/interp.py.  Stacks are arrays [N, H, W, channels], any value != 0 set; maps are int64 [N, channels, H, W]."""
import numpy as np
from scipy import ndimage

NONE = 0x7fffffff
MAX_WEIGHT = 32767


def _edt2(target):
    """Squared distance of every pixel to the nearest True pixel of ``target`` (which is not empty)."""
    d = ndimage.distance_transform_edt(~target)
    return np.rint(d * d).astype(np.int64)


def sd2_plane(m):
    m = np.asarray(m) != 0
    if not m.any():
        return np.full(m.shape, -NONE, np.int64)
    if m.all():
        return np.full(m.shape, NONE, np.int64)
    return np.where(m, _edt2(~m), -_edt2(m))


def sd2_stack(stack):
    stack = np.asarray(stack)
    n, h, w, ch = stack.shape
    out = np.empty((n, ch, h, w), np.int64)
    for i in range(n):
        for c in range(ch):
            out[i, c] = sd2_plane(stack[i, :, :, c])
    return out


def blend(a, b, wa, wb):
    """bool [H, W]: wa * s_a + wb * s_b > 0 with s = sign(sd2) * sqrt(|sd2|), NONE infinite, decided in int64."""
    a, b, wa, wb = np.asarray(a, np.int64), np.asarray(b, np.int64), int(wa), int(wb)
    assert 0 <= wa <= MAX_WEIGHT and 0 <= wb <= MAX_WEIGHT and (wa or wb)
    if wa == 0:
        return b > 0
    if wb == 0:
        return a > 0
    out = (a > 0) & (b > 0)
    for p, q, wp, wq in ((a, b, wa, wb), (b, a, wb, wa)):          # p the positive side, q the negative one
        opp = (p > 0) & (q < 0)
        pinf, qinf = p == NONE, q == -NONE
        finite = wp * wp * np.where(pinf, 0, p) > wq * wq * np.where(qinf, 0, -q)
        out |= opp & np.where(pinf & qinf, wp > wq, np.where(pinf, True, np.where(qinf, False, finite)))
    return out


def apply_plan(sd2, plan, out):
    """Rows (channel, out_slice, lo, hi, w_lo, w_hi) written into ``out`` float32 [N_out, H, W, channels] in place; (out, made)."""
    made = []
    for c, o, lo, hi, wa, wb in np.asarray(plan, np.int64).reshape(-1, 6).tolist():
        m = blend(sd2[lo, c], sd2[hi, c], wa, wb)
        out[o, :, :, c] = m
        made.append(int(m.sum()))
    return out, np.array(made, np.int64)


def gap_plan(present, max_gap, frames=None):
    """Rows sorted by (channel, slice).  A slice is ACCEPTED unless listed in frames.  Every rejected slice k gets, for every channel, a row from
    the nearest accepted slices below and above it (a copy of the one that exists when the other is off the stack's end); every accepted slice k
    that is absent in channel c and lies between the nearest accepted, present slices lo < k < hi of c gets a row from those two when
    hi - lo - 1 <= max_gap.  Weights: (hi - k, k - lo).  Nothing is made past the first or last present slice."""
    present = np.asarray(present, bool)
    n, ch = present.shape
    frames = sorted(set(int(f) for f in (frames or [])))
    accepted = [k for k in range(n) if k not in frames]
    if frames and not accepted:
        raise ValueError('nothing accepted')
    rows = set()
    for k in frames:
        below = [a for a in accepted if a < k]
        above = [a for a in accepted if a > k]
        lo = below[-1] if below else None
        hi = above[0] if above else None
        run = (hi if hi is not None else n) - (lo if lo is not None else -1) - 1
        if run > max_gap:
            raise ValueError('rejected run too long')
        for c in range(ch):
            if lo is None:
                rows.add((c, k, hi, hi, 1, 0))
            elif hi is None:
                rows.add((c, k, lo, lo, 1, 0))
            else:
                rows.add((c, k, lo, hi, hi - k, k - lo))
    for c in range(ch):
        good = [k for k in accepted if present[k, c]]
        for k in accepted:
            if present[k, c]:
                continue
            below = [a for a in good if a < k]
            above = [a for a in good if a > k]
            if below and above and above[0] - below[-1] - 1 <= max_gap:
                rows.add((c, k, below[-1], above[0], above[0] - k, k - below[-1]))
    return np.array(sorted(rows), np.int32).reshape(-1, 6)


def bridge(stack, max_gap, frames=None):
    """(new stack float32, plan, made): the planes of gap_plan re-made from the whole stack's maps, everything else copied."""
    stack = np.asarray(stack)
    present = (stack != 0).any(axis=(1, 2))
    plan = gap_plan(present, max_gap, frames)
    out = np.array(stack, dtype=np.float32)
    if plan.shape[0] == 0:
        return out, plan, np.zeros((0,), np.int64)
    sd2 = {}                                                         # only the planes a row names
    made = []
    for c, o, lo, hi, wa, wb in plan.tolist():
        for k in (lo, hi):
            if (k, c) not in sd2:
                sd2[(k, c)] = sd2_plane(stack[k, :, :, c])
        m = blend(sd2[(lo, c)], sd2[(hi, c)], wa, wb)
        out[o, :, :, c] = m
        made.append(int(m.sum()))
    return out, plan, np.array(made, np.int64)


def resample(stack, factor):
    """float32 [(N - 1) * factor + 1, H, W, channels]: key slice i at i * factor as 0 / 1, slice j of a gap blended with weights (factor - j, j)."""
    stack = np.asarray(stack)
    n, h, w, ch = stack.shape
    sd2 = sd2_stack(stack)
    out = np.zeros(((n - 1) * factor + 1, h, w, ch), np.float32)
    for i in range(n):
        out[i * factor] = stack[i] != 0
        if i + 1 < n:
            for j in range(1, factor):
                for c in range(ch):
                    out[i * factor + j, :, :, c] = blend(sd2[i, c], sd2[i + 1, c], factor - j, j)
    return out


def dice(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return 2.0 * (a & b).sum() / (a.sum() + b.sum())


def disc(cy, cx, r, h=64, w=64):
    """(x - cx)^2 + (y - cy)^2 <= r^2"""
    yy, xx = np.mgrid[:h, :w]
    return (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
