"""Host restatements of csrc/volume.hip, written from the semantics stated in include/octseg.h: the per-slice cv2.normalize(NORM_MINMAX, CV_8U)
+ channel reversal in numpy, and Pillow's 8-bit two-pass resample applied from the PRODUCT's tables (oct_segmentation_amd.pullback
.pil_resample_table) with int64 numpy sums -- so a test that holds pil_resize_ref to Image.resize pins the tables, and a test that holds the
kernel to Image.resize pins the kernel."""
import numpy as np

from oct_segmentation_amd.pullback import pil_resample_table


def slice_minmax(volume):
    """[S, 2] int64: minimum and maximum of every slice over all its channels."""
    v = np.asarray(volume)
    flat = v.reshape(v.shape[0], -1)
    return np.stack([flat.min(axis=1), flat.max(axis=1)], axis=1).astype(np.int64)


def normalize_ref(volume, swap_rb=True):
    """uint8 | uint16 [S,H,W,3] or [S,H,W] -> uint8 [S,H,W,3].  Per slice scale = 255 * (smax - smin > eps ? 1 / (smax - smin) : 0) and
    shift = 0 - smin * scale in double, both cast to float32; per sample np.float32 multiply, THEN np.float32 add (two roundings), np.rint
    (half to even), clip to 0..255; the three channels reversed with swap_rb, a grey volume written to three equal channels."""
    v = np.asarray(volume)
    assert v.dtype in (np.uint8, np.uint16) and v.ndim in (3, 4)
    if v.ndim == 3:
        v = v[..., None]
    out = np.empty(v.shape[:3] + (3,), np.uint8)
    for s, (smin, smax) in enumerate(slice_minmax(v)):
        d = float(smax) - float(smin)
        scale = 255.0 * (1.0 / d if d > np.finfo(np.float64).eps else 0.0)
        shift = 0.0 - float(smin) * scale
        a, b = np.float32(scale), np.float32(shift)
        prod = (v[s].astype(np.float32) * a).astype(np.float32)
        y = np.clip(np.rint((prod + b).astype(np.float32)), 0, 255).astype(np.uint8)
        if y.shape[2] == 1:
            y = np.repeat(y, 3, axis=2)
        elif swap_rb:
            y = y[:, :, ::-1]
        out[s] = y
    return out


def _pass(a, axis, out_len):
    """One pass of ImagingResample along `axis` of an int64 [H, W, C] array with 0..255 values."""
    bounds, kk = pil_resample_table(a.shape[axis], out_len)
    a = np.moveaxis(a, axis, 0)
    out = np.empty((out_len,) + a.shape[1:], np.int64)
    for i, (first, n) in enumerate(bounds):
        ss = (1 << 21) + np.tensordot(kk[i, :n].astype(np.int64), a[first:first + n], axes=(0, 0))
        out[i] = np.clip(ss >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def pil_resize_ref(frame, oh, ow):
    """uint8 [H,W] or [H,W,C] -> uint8 [oh,ow(,C)]: horizontal pass first, a pass that keeps its length skipped, as Pillow does."""
    a = np.asarray(frame)
    assert a.dtype == np.uint8
    squeeze = a.ndim == 2
    x = (a[:, :, None] if squeeze else a).astype(np.int64)
    if ow != x.shape[1]:
        x = _pass(x, 1, ow)
    if oh != x.shape[0]:
        x = _pass(x, 0, oh)
    x = x.astype(np.uint8)
    return x[:, :, 0] if squeeze else x
