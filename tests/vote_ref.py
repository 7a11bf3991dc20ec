"""Host restatement of csrc/vote.hip, written from the header comment of octseg_vote_assemble in include/octseg.h.  numpy only; views and un-views
are array operations, the mean probability is float64 from the float32 logits."""
import numpy as np

STAT_COLUMNS = ('set', 'disputed', 'disputed_and_set', 'dissent_sum')


def view(x, code):
    """View ``code = a + 2 b + 4 t`` of an array whose last two axes are the frame: transpose if t, reverse the rows if b, the columns if a."""
    if code & 4:
        x = np.swapaxes(x, -1, -2)
    if code & 2:
        x = x[..., ::-1, :]
    if code & 1:
        x = x[..., ::-1]
    return np.ascontiguousarray(x)


def unview(y, code):
    """The inverse of ``view``: the steps undone in reverse order (each is its own inverse)."""
    if code & 1:
        y = y[..., ::-1]
    if code & 2:
        y = y[..., ::-1, :]
    if code & 4:
        y = np.swapaxes(y, -1, -2)
    return np.ascontiguousarray(y)


def compose(v, w):
    """The code of ``view(view(x, v), w)``, found on a frame of distinct values."""
    x = np.arange(9).reshape(3, 3)
    y = view(view(x, v), w)
    return next(c for c in range(8) if np.array_equal(view(x, c), y))


def center_index(src, dst):
    """The null-table rule: floor((i + 0.5) * src / dst) in exact integers."""
    i = np.arange(dst, dtype=np.int64)
    return ((2 * i + 1) * src // (2 * dst)).astype(np.int64)


def sigmoid64(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def vote(members, channels, views, out_hw, rows=None, cols=None, mode=0):
    """members: float32 [N, classes_m, Hm, Wm] in view coordinates.  Returns a dict of [N, out_h, out_w] arrays -- ``pbar`` float64, ``votes`` /
    ``mask`` / ``dissent`` integer -- and ``stats`` int64 [N, 4] (STAT_COLUMNS)."""
    M = len(members)
    oh, ow = out_hw
    planes = [unview(np.asarray(z)[:, c], v) for z, c, v in zip(members, channels, views)]       # [N, H, W] each, un-viewed
    H, W = planes[0].shape[1:]
    assert all(p.shape == planes[0].shape for p in planes)
    r = center_index(H, oh) if rows is None else np.asarray(rows, dtype=np.int64)
    c = center_index(W, ow) if cols is None else np.asarray(cols, dtype=np.int64)
    r, c = np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)
    z = np.stack([p[:, r][:, :, c] for p in planes])                                             # [M, N, oh, ow] float32
    pbar = sigmoid64(z).sum(axis=0) / M
    votes = (z > 0).sum(axis=0).astype(np.int64)       # sigmoid(z) > 0.5; the cases keep |z| >= 0.01, where every arithmetic agrees
    mask = (2 * votes > M) if mode else (pbar > 0.5)
    dissent = np.where(mask, M - votes, votes)
    disputed = (votes > 0) & (votes < M)
    stats = np.stack([mask.sum(axis=(1, 2)), disputed.sum(axis=(1, 2)), (disputed & mask).sum(axis=(1, 2)), dissent.sum(axis=(1, 2))], axis=1)
    return {'pbar': pbar, 'votes': votes, 'mask': mask.astype(np.int64), 'dissent': dissent.astype(np.int64), 'stats': stats.astype(np.int64)}
