"""Host restatement of the reference's save_results (src/data/utils.py:195-235) for the rendering tests -- independent of
oct_segmentation_amd/postprocess.py and of the kernel.  cv2 is not installed, so its three operations are restated from their definitions
(OpenCV 4.8.1): morphology with getStructuringElement(MORPH_ELLIPSE) and the default border ("outside the frame does not take part"),
GaussianBlur((5, 5), 0) = the fixed (1, 4, 6, 4, 1) / 16 kernel per axis with BORDER_REFLECT_101.  The pastes and the colour mask are done by PIL
itself, the library the reference calls."""
import numpy as np
from PIL import Image

CLASS_IDS = {'Lumen': 1, 'Fibrous cap': 2, 'Lipid core': 3, 'Vasa vasorum': 4}
CLASS_COLORS_RGB = {'Lumen': (228, 30, 199), 'Fibrous cap': (123, 171, 226), 'Lipid core': (125, 227, 127), 'Vasa vasorum': (208, 2, 27)}
ALL_CLASSES = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
ROW_WIDTHS = {5: (1, 5, 5, 5, 1), 7: (1, 5, 7, 7, 7, 5, 1)}


def footprint(n):
    """The n x n ellipse from its row widths (centred rows)."""
    fp = np.zeros((n, n), bool)
    for i, w in enumerate(ROW_WIDTHS[n]):
        fp[i, n // 2 - w // 2:n // 2 + w // 2 + 1] = True
    return fp


def _morph(m, fp, erode):
    """One dilation (max) or erosion (min) of a boolean mask; outside the frame = the operation's neutral value."""
    m = np.asarray(m).astype(bool)
    r = fp.shape[0] // 2
    h, w = m.shape
    p = np.pad(m, r, mode='constant', constant_values=bool(erode))
    out = np.ones_like(m) if erode else np.zeros_like(m)
    for i in range(fp.shape[0]):
        for j in range(fp.shape[1]):
            if fp[i, j]:
                v = p[i:i + h, j:j + w]
                out = (out & v) if erode else (out | v)
    return out


def dilate(m, n):
    return _morph(m, footprint(n), False)


def erode(m, n):
    return _morph(m, footprint(n), True)


def close(m, iterations):
    """cv2.morphologyEx(m, MORPH_CLOSE, ellipse(5, 5), iterations=it): it dilations, then it erosions."""
    m = np.asarray(m).astype(bool)
    for _ in range(iterations):
        m = dilate(m, 5)
    for _ in range(iterations):
        m = erode(m, 5)
    return m


def blur256(m):
    """256 * cv2.GaussianBlur(m, (5, 5), 0) of a 0/1 mask, as integers: (1,4,6,4,1) per axis, BORDER_REFLECT_101 (numpy's 'reflect')."""
    m = np.asarray(m).astype(np.int64)
    h, w = m.shape
    taps = (1, 4, 6, 4, 1)
    p = np.pad(m, ((0, 0), (2, 2)), mode='reflect') if w > 1 else np.repeat(m, 5, axis=1)
    hor = sum(t * p[:, j:j + w] for j, t in enumerate(taps))
    p = np.pad(hor, ((2, 2), (0, 0)), mode='reflect') if h > 1 else np.repeat(hor, 5, axis=0)
    return sum(t * p[i:i + h, :] for i, t in enumerate(taps))


def wrap_alpha(x):
    """uint8(x) as the reference's platform casts a float64 beyond 255: truncate, keep the low byte -- by integer arithmetic, no astype('uint8')."""
    return (np.floor(np.asarray(x, np.float64)).astype(np.int64) % 256).astype(np.uint8)


def paste_int(inp, col, a):
    """PIL's paste of a solid colour through an L mask, per channel."""
    t = inp.astype(np.int64) * (255 - a.astype(np.int64)) + int(col) * a.astype(np.int64) + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def render(img, mask, classes, close_iterations=1):
    """save_results for one frame.  img: PIL RGB image; mask: [H, W, 4] array of 0 / 1.  Returns (overlay, color_mask) uint8 [H, W, 3]."""
    img = img.convert('RGB').copy()
    mask = np.asarray(mask)
    color_mask = Image.new('RGB', size=img.size, color=(128, 128, 128))
    for class_name in classes:
        m0 = mask[:, :, CLASS_IDS[class_name] - 1].astype(np.float64)
        color = CLASS_COLORS_RGB[class_name]
        m = close(m0 != 0, close_iterations)
        ring = dilate(m, 7) & ~erode(m, 7)
        b = blur256(m) / 256.0
        class_img = Image.new('RGB', size=img.size, color=color)
        for alpha_src in (b * 64, ring.astype(np.float64) * 255):        # get_img_mask_union_pil: mask * alpha * 255, cast to uint8
            a = wrap_alpha(alpha_src * 0.85 * 255)
            img.paste(class_img, (0, 0), Image.fromarray(a))
        color_mask.paste(class_img, (0, 0), Image.fromarray(m0 * 255).convert('L'))
    return np.asarray(img), np.asarray(color_mask)


def render_batch(frames, masks, classes, close_iterations=1):
    """frames uint8 [N, H, W, 3], masks [N, H, W, 4] -> (overlay, color_mask) uint8 [N, H, W, 3]."""
    outs = [render(Image.fromarray(f), m, classes, close_iterations) for f, m in zip(frames, masks)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


# ---- the reference pin: a window of the authors' own run (tests/golden/demo_overlay_crop.npz, made by tests/golden/make_overlay_fixture.py)
PIN_DISTANCE = 20     # the chain reaches 15 px; compared pixels are further than this from anything that is not a pure colour, and from the crop's border


def _dilate_square(a, r):
    """Chebyshev dilation by r (separable)."""
    h, w = a.shape
    p = np.pad(a, ((0, 0), (r, r)))
    a = np.any([p[:, j:j + w] for j in range(2 * r + 1)], axis=0)
    p = np.pad(a, ((r, r), (0, 0)))
    return np.any([p[i:i + h, :] for i in range(2 * r + 1)], axis=0)


def load_pin(path):
    """The fixture as (frame uint8 [h,w,3], masks float64 [h,w,4], authors' overlay, compared bool [h,w]).  Masks = pixels of exactly a class
    colour; compared = more than PIN_DISTANCE px (Chebyshev) from any pixel that is neither a class colour nor (128,128,128), and from the
    crop's border."""
    z = np.load(path)
    frame, cm, overlay = z['frame'], z['mask'], z['overlay']
    h, w = cm.shape[:2]
    masks = np.zeros((h, w, 4))
    pure = np.all(cm == 128, axis=2)
    for name in ALL_CLASSES:
        hit = np.all(cm == np.array(CLASS_COLORS_RGB[name], np.uint8), axis=2)
        masks[:, :, CLASS_IDS[name] - 1] = hit
        pure |= hit
    compared = ~_dilate_square(~pure, PIN_DISTANCE)
    d = PIN_DISTANCE
    inner = np.zeros((h, w), bool)
    inner[d:h - d, d:w - d] = True                      # more than d px from the first pixel outside the crop
    return frame, masks, overlay, compared & inner


def check_pin_coverage(frame, overlay, compared):
    """The comparison cannot quietly shrink: at least half of the crop is compared, and at least a quarter of the crop are compared pixels that
    the overlay changes."""
    n = compared.size
    changed = compared & np.any(frame != overlay, axis=2)
    assert compared.sum() * 2 >= n, (int(compared.sum()), n)
    assert changed.sum() * 4 >= n, (int(changed.sum()), n)
    return int(compared.sum()), int(changed.sum())
