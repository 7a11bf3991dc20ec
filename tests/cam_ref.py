"""Host restatement of csrc/cam.hip, written from the semantics stated in include/octseg.h and DESIGN.md section 12 (the role
tests/analysis_ref.py has for the measuring kernel).  numpy only; nothing here is shared with oct_segmentation_amd/cam.py.

    m = cam_map(A, G, 'XGradCAM', S)              # A, G: [K, h, w] -> [S, S] in `dtype` (float64 unless asked otherwise)
    b = binarize(m, thr); counts(b, gt)           # uint8 0/255; tp, pred, true after cv2's nearest resize to gt's size
    o = overlay(frame_bgr_planes, m32, 0.5)       # uint8 [S, S, 3] BGR, float32 arithmetic in numpy's order of operations
"""
import numpy as np

METHODS = ('GradCAM', 'HiResCAM', 'GradCAMElementWise', 'GradCAMPlusPlus', 'XGradCAM', 'LayerCAM')


def raw_map(A, G, method, dtype=np.float64):
    """The method's map before any scaling: A, G [K, h, w]."""
    A, G = np.asarray(A, dtype), np.asarray(G, dtype)
    if method == 'GradCAM':
        return (G.mean(axis=(1, 2))[:, None, None] * A).sum(axis=0)
    if method == 'HiResCAM':
        return (G * A).sum(axis=0)
    if method == 'GradCAMElementWise':
        return np.maximum(G * A, 0).sum(axis=0)
    if method == 'GradCAMPlusPlus':
        g2 = G * G
        sA = A.sum(axis=(1, 2))[:, None, None]
        den = 2 * g2 + sA * (g2 * G) + dtype(1e-6)
        aij = np.where(G != 0, g2 / np.where(den == 0, 1, den), 0)
        w = (np.maximum(G, 0) * aij).sum(axis=(1, 2))
        return (w[:, None, None] * A).sum(axis=0)
    if method == 'XGradCAM':
        w = (G * A).sum(axis=(1, 2)) / (A.sum(axis=(1, 2)) + dtype(1e-7))
        return (w[:, None, None] * A).sum(axis=0)
    if method == 'LayerCAM':
        return (np.maximum(G, 0) * A).sum(axis=0)
    raise ValueError(method)


def scale01(x):
    x = x - x.min()
    return x / (x.dtype.type(1e-7) + x.max())


def _taps(src, dst):
    """cv2.resize INTER_LINEAR, float images: fx = (float)((d + 0.5) * scale - 0.5), clamped taps with a zero fraction at the borders."""
    scale = float(src) / float(dst)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= src - 1
    f[lo | hi] = 0
    s[lo] = 0
    s[hi] = src - 1
    return s, np.minimum(s + 1, src - 1), f


def resize_linear(img, S):
    """[h, w] -> [S, S], horizontal pass then vertical pass, in img's dtype."""
    dt = img.dtype.type
    x0, x1, fx = _taps(img.shape[1], S)
    y0, y1, fy = _taps(img.shape[0], S)
    fx, fy = fx.astype(img.dtype), fy.astype(img.dtype)
    rows = img[:, x0] * (dt(1) - fx)[None, :] + img[:, x1] * fx[None, :]
    return rows[y0] * (dt(1) - fy)[:, None] + rows[y1] * fy[:, None]


def cam_map(A, G, method, S, dtype=np.float64):
    cam = np.maximum(raw_map(A, G, method, dtype), 0)
    cam = scale01(cam)
    cam = np.maximum(resize_linear(cam, S), 0)
    return scale01(cam)


def jet_bgr():
    v = np.arange(256) / 255.0
    b, g, r = (np.clip(1.5 - np.abs(4 * v - k), 0, 1) for k in (1, 2, 3))
    return np.rint(np.stack([b, g, r], 1) * 255).astype(np.uint8)


def overlay(frame_planes, m, image_weight=0.5):
    """show_cam_on_image(frame / 255, m, use_rgb=False, image_weight): frame_planes [3, S, S] BGR 0..255, m float32 [S, S]."""
    m = np.asarray(m, np.float32)
    heat = jet_bgr()[np.uint8(np.float32(255) * m)].astype(np.float32) / np.float32(255)          # [S, S, 3]
    img = np.asarray(frame_planes, np.float32).transpose(1, 2, 0) / np.float32(255)
    o = np.float32(1 - image_weight) * heat + np.float32(image_weight) * img
    o = o / o.max()
    return np.uint8(np.float32(255) * o)


def nearest_index(src, dst):
    """cv2 INTER_NEAREST: min(floor(d * (1 / (dst / src))), src - 1)."""
    return np.minimum(np.floor(np.arange(dst) * (1.0 / (float(dst) / float(src)))).astype(np.int64), src - 1)


def binarize(m, thr):
    return ((np.asarray(m) > np.float32(thr)).astype(np.uint8)) * 255


def resize_nearest(b, gh, gw):
    return b[nearest_index(b.shape[0], gh)][:, nearest_index(b.shape[1], gw)]


def counts(b, gt):
    """tp, pred, true of the 0/255 map b (nearest-resized to gt's size) against the plane gt (non-zero = set)."""
    p, t = resize_nearest(b, *gt.shape) != 0, np.asarray(gt) != 0
    return int((p & t).sum()), int(p.sum()), int(t.sum())


def metrics(tp, pred, true):
    d = lambda a, b: a / b if b else 0.0   # noqa: E731
    return {'Dice': d(2 * tp, pred + true), 'IoU': d(tp, pred + true - tp), 'Precision': d(tp, pred), 'Recall': d(tp, true),
            'F1': d(2 * tp, pred + true)}


def synth(K, h, w, seed, dead=True):
    """Synthetic A >= 0 (a few dead channels) and signed G with a smooth component, [K, h, w] float32."""
    rng = np.random.default_rng(seed)
    A = np.maximum(rng.standard_normal((K, h, w)) + 0.3, 0).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    bump = np.exp(-(((yy - 0.4 * h) ** 2 + (xx - 0.6 * w) ** 2) / (0.1 * (h * w) + 1.0)))
    A = (A * (0.5 + bump)[None]).astype(np.float32)
    G = (rng.standard_normal((K, h, w)) * 1e-2 + 2e-3 * (rng.random((K, 1, 1)) - 0.3)).astype(np.float32)
    if dead:
        A[::7] = 0
        G[3::11] = 0
    return A, G


def bf16_round(x):
    """float32 -> nearest-even bfloat16 -> float32."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)
