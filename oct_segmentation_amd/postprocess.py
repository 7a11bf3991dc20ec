"""Overlays and colour masks on the GPU -- the output half of the pipeline, mirror of the reference's ``save_results``
(``src/data/utils.py:195-235``) and its paste helper ``get_img_mask_union_pil`` (``src/models/smp/utils.py:203-213``).

Per frame and class, in list order, the reference closes the class's 0/1 mask (``cv2.morphologyEx(m, MORPH_CLOSE, ellipse(5, 5), 3)``),
builds a ring (``dilate(m, ellipse(7, 7))`` with ``erode(m, ellipse(7, 7)) > 0`` cleared), blurs the closed mask
(``GaussianBlur(m, (5, 5), 0)``) and pastes the class colour into the frame through PIL twice: with ``uint8(blur * 64 * 0.85 * 255)`` and with
``uint8(ring * 255 * 0.85 * 255)`` as the alpha.  Both products exceed 255 and numpy's cast wraps, so a class's interior is blended with alpha
48 and the ring with alpha 231; the published demo overlays show exactly that, and it is kept.  The colour mask is (128,128,128) with the class
colour wherever the RAW mask is set.  One kernel (``octseg_render_results``, ``csrc/render.hip``) does all of it for a batch in integer
arithmetic; the host only decodes and encodes image files.

``close_iterations``: in OpenCV's Python signature ``morphologyEx(src, op, kernel[, dst[, anchor[, iterations ...`` the fourth positional
argument is ``dst``, not ``iterations``; the bindings take an integer there as a throw-away matrix, so the reference's call as written most
likely runs ONE iteration, not the three it seems to ask for.  cv2 is not available to settle it and the published overlays do not discriminate
(DESIGN 5b), so the count is a parameter (1, 2 or 3) whose default, 1, is what the call as written executes.

    overlay, color_mask = render_results(frames_u8, stack, classes)            # uint8 [N,H,W,3] CUDA, float32 [N,H,W,4] CUDA
    save_results(images, stack, names, classes, save_dir)                       # the reference's call; masks: numpy arrays or the device stack
"""
import os

import numpy as np
import torch
from PIL import Image

from . import _lib as L
from .model import CLASS_IDS

# src/data/utils.py:16-37
CLASS_COLORS_RGB = {'Lumen': (228, 30, 199), 'Fibrous cap': (123, 171, 226), 'Lipid core': (125, 227, 127), 'Vasa vasorum': (208, 2, 27)}
PASTE_ALPHA = 0.85                    # get_img_mask_union_pil's default
BLUR_TAPS = (1, 4, 6, 4, 1)           # cv2.getGaussianKernel(5, 0) * 16: OpenCV's fixed kernel for ksize <= 7 and sigma <= 0
MAX_CLASSES = 16

_consts = {}   # (kind, ..., device) -> device tensor


def ellipse(n):
    """``cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (n, n))`` (OpenCV 4.8.1 morph.dispatch.cpp): row ``i`` is set on ``[c - dx, c + dx]`` with
    ``dx = cvRound(c * sqrt((r * r - dy * dy) / (r * r)))``, ``r = c = n // 2``, ``dy = i - r``.  uint8 [n, n]."""
    n = int(n)
    r = c = n // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    out = np.zeros((n, n), np.uint8)
    for i in range(n):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) * inv_r2)))      # saturate_cast<int>(double) = cvRound: half to even
            out[i, max(c - dx, 0):min(c + dx + 1, n)] = 1
    return out


def _wrap_u8(x):
    """``x.astype('uint8')`` of non-negative float64 beyond 255 as numpy does it on the reference's platform: truncate, keep the low byte."""
    return (np.asarray(x, np.float64).astype(np.int64) & 255).astype(np.uint8)


def alpha_table():
    """Alpha of the first paste for every value of the blur: on a 0/1 mask ``GaussianBlur(m, (5, 5), 0)`` is ``k / 256``, ``k`` = 0..256, and
    the reference pastes through ``uint8(b * 64 * 0.85 * 255)`` (utils.py:223, smp/utils.py:209-212), float64 products in that order, wrapped by
    the cast.  uint8 [257]; ``[256]`` (a class's interior) is 48."""
    b = np.arange(257, dtype=np.float64) / 256.0
    return _wrap_u8(b * 64 * PASTE_ALPHA * 255)


RING_ALPHA = int(_wrap_u8(np.float64(1.0) * 255 * PASTE_ALPHA * 255))     # utils.py:228: the ring's paste, 55271 & 255 = 231


def _const_dev(key, make, device):
    key = key + (str(device),)
    if key not in _consts:
        _consts[key] = make().to(device)
    return _consts[key]


def _check_classes(classes, channels):
    classes = list(classes)
    if not classes or len(classes) > MAX_CLASSES:
        raise ValueError(f'classes must name 1..{MAX_CLASSES} classes, got {len(classes)}')
    for cl in classes:
        if cl not in CLASS_IDS or cl not in CLASS_COLORS_RGB:
            raise ValueError(f'unknown class {cl!r}')
        if CLASS_IDS[cl] > channels:
            raise ValueError(f'class {cl!r} needs mask channel {CLASS_IDS[cl] - 1}, the stack has {channels}')
    return classes


def render_results(frames_u8, stack, classes, close_iterations=1):
    """The array part of ``save_results`` for a batch: ``frames_u8`` uint8 CUDA [N,H,W,3] RGB (the frames at output size), ``stack`` float32
    CUDA [N,H,W,channels] of 0 / 1 (``predict.segment_stack``), ``classes`` in the order they are drawn (it matters where classes overlap).
    Returns ``(overlay, color_mask)``, uint8 CUDA [N,H,W,3].  One launch, no host synchronisation."""
    if not (torch.is_tensor(frames_u8) and frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and frames_u8.dim() == 4
            and frames_u8.shape[3] == 3):
        raise ValueError('frames_u8 must be a uint8 CUDA tensor [N, H, W, 3]')
    if not (torch.is_tensor(stack) and stack.is_cuda and stack.dtype == torch.float32 and stack.dim() == 4):
        raise ValueError('stack must be a float32 CUDA tensor [N, H, W, channels]')
    if stack.device != frames_u8.device or tuple(stack.shape[:3]) != tuple(frames_u8.shape[:3]):
        raise ValueError(f'frames {tuple(frames_u8.shape)} and stack {tuple(stack.shape)} must share device, batch and frame size')
    if 0 in stack.shape or 0 in frames_u8.shape:
        raise ValueError('empty batch or frame')
    if int(close_iterations) not in (1, 2, 3):
        raise ValueError(f'close_iterations must be 1, 2 or 3, got {close_iterations}')
    classes = _check_classes(classes, stack.shape[3])
    dev = frames_u8.device
    frames_u8, stack = frames_u8.contiguous(), stack.contiguous()
    n, h, w, sc = stack.shape
    key = tuple(classes)
    ch = _const_dev(('render_ch', key), lambda: torch.tensor([CLASS_IDS[c] - 1 for c in classes], dtype=torch.int32), dev)
    rgb = _const_dev(('render_rgb', key), lambda: torch.tensor([CLASS_COLORS_RGB[c] for c in classes], dtype=torch.uint8), dev)
    tab = _const_dev(('render_alpha',), lambda: torch.from_numpy(alpha_table()), dev)
    overlay, color_mask = torch.empty_like(frames_u8), torch.empty_like(frames_u8)
    L.check(L.lib().octseg_render_results(L.ptr(stack), L.ptr(frames_u8), n, h, w, sc, L.ptr(ch), L.ptr(rgb), len(classes), L.ptr(tab),
                                          RING_ALPHA, int(close_iterations), L.ptr(overlay), L.ptr(color_mask), L.stream_ptr()))
    return overlay, color_mask


def epoch_panels(frames_f32, logits, gt_u8, classes, labels=True):
    """The array part of ``log_predict_model_on_epoch`` (reference ``src/models/smp/model.py:227-242``) for a group of frames whose ground
    truth shares one source size: ``frames_f32`` float32 CUDA [N,3,S,S], BGR planes 0..255 (``ingest.resize_image_u8``); ``logits`` float32
    CUDA [N,len(classes),S,S] (``predict_logits`` of those frames); ``gt_u8`` uint8 CUDA [N,Hs,Ws,channels], the RAW TIFF samples at their own
    size -- the kernel nearest-resizes them with cv2's rule and paints a class where its channel is exactly 255.  ``classes`` in the order they
    are drawn.  Returns ``(panels, labels)``: uint8 CUDA [N,S,3*S,3] RGB strips image | ground truth | prediction, and uint8 CUDA [N,2,S,S]
    label maps (0: prediction, 1: ground truth; ``labels=False``: None).  One launch (``octseg_epoch_panels``, ``csrc/panels.hip``), no host
    synchronisation."""
    from .ingest import _nearest_dev
    if not (torch.is_tensor(frames_f32) and frames_f32.is_cuda and frames_f32.dtype == torch.float32 and frames_f32.dim() == 4
            and frames_f32.shape[1] == 3 and frames_f32.shape[2] == frames_f32.shape[3]):
        raise ValueError('frames_f32 must be a float32 CUDA tensor [N, 3, S, S]')
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4):
        raise ValueError('logits must be a float32 CUDA tensor [N, classes, S, S]')
    if not (torch.is_tensor(gt_u8) and gt_u8.is_cuda and gt_u8.dtype == torch.uint8 and gt_u8.dim() == 4):
        raise ValueError('gt_u8 must be a uint8 CUDA tensor [N, H, W, channels]')
    if 0 in frames_f32.shape or 0 in logits.shape or 0 in gt_u8.shape:
        raise ValueError('empty batch or frame')
    classes = _check_classes(classes, gt_u8.shape[3])
    n, _, s, _ = frames_f32.shape
    if logits.device != frames_f32.device or gt_u8.device != frames_f32.device or tuple(logits.shape) != (n, len(classes), s, s) \
            or gt_u8.shape[0] != n:
        raise ValueError(f'frames {tuple(frames_f32.shape)}, logits {tuple(logits.shape)} and ground truth {tuple(gt_u8.shape)} must share '
                         f'device and batch, and the logits the frame size and one plane per class')
    dev = frames_f32.device
    frames_f32, logits, gt_u8 = frames_f32.contiguous(), logits.contiguous(), gt_u8.contiguous()
    _, sh, sw, sc = gt_u8.shape
    key = tuple(classes)
    ch = _const_dev(('render_ch', key), lambda: torch.tensor([CLASS_IDS[c] - 1 for c in classes], dtype=torch.int32), dev)
    rgb = _const_dev(('render_rgb', key), lambda: torch.tensor([CLASS_COLORS_RGB[c] for c in classes], dtype=torch.uint8), dev)
    ids = _const_dev(('panel_ids', key), lambda: torch.tensor([CLASS_IDS[c] for c in classes], dtype=torch.uint8), dev)
    rows, cols = _nearest_dev(sh, s, dev), _nearest_dev(sw, s, dev)
    panels = torch.empty((n, s, 3 * s, 3), dtype=torch.uint8, device=dev)
    lab = torch.empty((n, 2, s, s), dtype=torch.uint8, device=dev) if labels else None
    L.check(L.lib().octseg_epoch_panels(L.ptr(frames_f32), L.ptr(logits), L.ptr(gt_u8), n, s, len(classes), sh, sw, sc, L.ptr(rows), L.ptr(cols),
                                        L.ptr(ch), L.ptr(rgb), L.ptr(ids), L.ptr(panels), L.ptr(lab), L.stream_ptr()))
    return panels, lab


def save_results(images, masks, images_name, classes, save_dir, close_iterations=1, device='cuda'):
    """utils.py:195-235.  ``images``: PIL images at output size, or the same frames as a uint8 CUDA tensor [n, H, W, 3] (RGB), which skips the
    upload.  PIL images are converted to RGB: the reference pastes into whatever mode
    ``Image.open`` gave, and for other modes (L, RGBA, P) PIL's paste of an RGB colour behaves differently; RGB is what the demo frames are.
    ``masks``: the list of numpy [H, W, 4] arrays ``segment`` returns, or the device stack [n, H, W, 4] of ``segment_stack`` (then the masks
    never visit the host).  Masks must be 0 / 1 -- what ``segment`` produces and what makes the arithmetic exact; anything else raises
    ``ValueError``.  One upload, one launch, one device-to-host copy of uint8, then ``{name}_mask.png`` and ``{name}_overlay.png`` through PIL."""
    frames = None
    if torch.is_tensor(images):       # uint8 RGB frames that are on the device already: no upload (render_results checks them)
        frames = images
    images, images_name = list(images), list(images_name)
    if torch.is_tensor(masks):
        stack = masks
        if not (stack.dim() == 4 and stack.dtype == torch.float32 and stack.is_cuda):
            raise ValueError('a mask stack must be a float32 CUDA tensor [n, H, W, channels]')
        dev = stack.device
    else:
        arrs = [np.asarray(m) for m in masks]
        if not arrs or any(a.ndim != 3 or a.shape != arrs[0].shape for a in arrs):
            raise ValueError('masks must be equally sized [H, W, channels] arrays')
        host = np.stack(arrs)
        if not np.isin(host, (0, 1)).all():
            raise ValueError('masks must hold only 0 and 1')
        dev = torch.device(device)
        stack = torch.from_numpy(host.astype(np.float32)).to(dev)
    if not (len(images) == len(images_name) == stack.shape[0]) or not images:
        raise ValueError(f'{len(images)} images, {len(images_name)} names and {stack.shape[0]} masks')
    if torch.is_tensor(masks) and not bool(((stack == 0) | (stack == 1)).all()):
        raise ValueError('masks must hold only 0 and 1')
    h, w = int(stack.shape[1]), int(stack.shape[2])
    if frames is None:
        for img in images:
            if img.size != (w, h):
                raise ValueError(f'image size {img.size} does not match the masks ({w}, {h})')
        frames = torch.from_numpy(np.stack([np.asarray(img.convert('RGB')) for img in images])).to(dev)
    overlay, color_mask = render_results(frames, stack, classes, close_iterations)
    out = torch.stack([overlay, color_mask]).cpu().numpy()
    os.makedirs(save_dir, exist_ok=True)
    for i, name in enumerate(images_name):
        Image.fromarray(out[1, i]).save(f'{save_dir}/{name}_mask.png')
        Image.fromarray(out[0, i]).save(f'{save_dir}/{name}_overlay.png')
