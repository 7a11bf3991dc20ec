"""numpy restatement of octseg_logit_histogram, written from the header comment of include/octseg.h (not from the kernel): a float64 sigmoid,
bin = clamp(ceil(p * 256) - 1, 0, 255), a pixel is positive iff its target is != 0, hist[n][c][label][bin].  Beside it the f32 restatement of
the engine's one sigmoid, which tests/test_curves.py holds against the float64 rule on every case, and direct threshold counts."""
import numpy as np

BINS = 256


def sigmoid64(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bins64(z):
    return np.clip(np.ceil(sigmoid64(z) * 256.0).astype(np.int64) - 1, 0, BINS - 1)


def sigmoid_acc32(z):
    """The header's f32 rule step by step: e = expf(-|z|); p = z >= 0 ? 1 / (1 + e) : e / (1 + e), every operation rounded to float32."""
    z = np.asarray(z, dtype=np.float32)
    one = np.float32(1.0)
    e = np.exp(-np.abs(z)).astype(np.float32)
    return np.where(z >= 0, one / (one + e), e / (one + e)).astype(np.float32)


def bins32(z):
    p = sigmoid_acc32(z)
    return np.clip(np.ceil(p * np.float32(256.0)).astype(np.int64) - 1, 0, BINS - 1)


def histogram(logits, target, bins=bins64):
    """int64 [N, C, 2, 256]: per frame and class the bin counts of the truth-negative (0) and the truth-positive (1) pixels."""
    logits, target = np.asarray(logits), np.asarray(target)
    N, C = logits.shape[:2]
    b = bins(logits).reshape(N, C, -1)
    lab = (target != 0).reshape(N, C, -1)
    out = np.zeros((N, C, 2, BINS), dtype=np.int64)
    for n in range(N):
        for c in range(C):
            for label in (0, 1):
                out[n, c, label] = np.bincount(b[n, c][lab[n, c] == bool(label)], minlength=BINS)
    return out


def counts_at(logits, target, cut):
    """int64 [N, C, 4]: tp, fp, fn, tn of the mask ``logits > cut`` (cut = 0 is sigmoid > 0.5) against ``target != 0``, counted directly."""
    pred, pos = np.asarray(logits) > cut, np.asarray(target) != 0
    s = lambda a: a.sum(axis=(2, 3)).astype(np.int64)      # noqa: E731
    return np.stack([s(pred & pos), s(pred & ~pos), s(~pred & pos), s(~pred & ~pos)], axis=-1)
