"""uint8 frames and masks -> the nets' float32 NCHW batch on the GPU -- device half of the input pipeline.

Mirror of the array lines of ``OCTDataset.__getitem__`` (reference ``src/models/smp/dataset.py:108-127``) and of
``preprocessing_img`` (``src/data/utils.py:159-166``): ``cv2.resize`` of the uint8 frame, ``cv2.resize(..., INTER_NEAREST)`` of
the mask, channel select, bool -> float, HWC -> CHW float32.  The decoded uint8 arrays cross to the device as they are and two
kernels (``octseg_ingest_image`` / ``octseg_ingest_mask``, ``csrc/ingest.hip``) do the rest from per-axis tables made here with
OpenCV's roundings (``predict.cv2_linear_coeffs`` / ``cv2_nearest_index``): integer arithmetic, equal to cv2's result.

    img = resize_image_u8(frames_u8, 704)                        # [B,H,W,3] uint8 CUDA -> [B,3,704,704] float32 0..255
    mask = select_resize_mask(masks_u8, [1, 3], 704)             # [B,H,W,4] uint8 CUDA, CLASS_IDS -> [B,2,704,704] float32 0/1
"""
import numpy as np
import torch

from . import _lib as L
from .predict import cv2_linear_coeffs, cv2_nearest_index

_tables = {}   # (kind, src, dst[, horizontal], device) -> device int32 tensor


def _size2(size):
    """``size``: an int (square, the reference's input_size) or (height, width)."""
    if isinstance(size, (tuple, list)):
        h, w = size
    else:
        h = w = size
    h, w = int(h), int(w)
    if h <= 0 or w <= 0:
        raise ValueError(f'size must be positive, got {size}')
    return h, w


def linear_table(src, dst, horizontal):
    """int32 [4, dst] of one axis: first tap, second tap, their 11-bit coefficients (the layout octseg_ingest_image documents)."""
    s0, s1, a0, a1 = cv2_linear_coeffs(int(src), int(dst), horizontal=horizontal)
    return np.stack([s0, s1, a0, a1]).astype(np.int32)


def _linear_dev(src, dst, horizontal, device):
    key = ('linear', int(src), int(dst), bool(horizontal), str(device))
    if key not in _tables:
        _tables[key] = torch.from_numpy(linear_table(src, dst, horizontal)).to(device)
    return _tables[key]


def _nearest_dev(src, dst, device):
    key = ('nearest', int(src), int(dst), str(device))
    if key not in _tables:
        _tables[key] = torch.from_numpy(cv2_nearest_index(int(src), int(dst))).to(device)
    return _tables[key]


def _channels_dev(class_ids, device):
    ids = tuple(int(c) - 1 for c in class_ids)
    key = ('channels', ids, str(device))
    if key not in _tables:
        _tables[key] = torch.tensor(ids, dtype=torch.int32).to(device)
    return _tables[key]


def _check_u8(t, name, last=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 4):
        raise ValueError(f'{name} must be a uint8 CUDA tensor [B, H, W, C]')
    if last is not None and t.shape[3] != last:
        raise ValueError(f'{name} must have {last} channels, got {tuple(t.shape)}')
    if t.shape[0] == 0:
        raise ValueError(f'{name} is an empty batch')


def resize_image_u8(frames_u8, size, swap_rb=False, out=None):
    """``cv2.resize(frame, (W, H))`` of every uint8 HWC frame, as float32 planes: [B,Hs,Ws,3] uint8 CUDA -> [B,3,H,W] float32 0..255.
    ``swap_rb``: the source is RGB and the planes come out BGR (``cvtColor(RGB2BGR)`` of preprocessing_img).  ``out``: a contiguous
    float32 [B,3,H,W] tensor (or slice of a batch) to write instead of a new one."""
    _check_u8(frames_u8, 'frames_u8', 3)
    dh, dw = _size2(size)
    x = frames_u8.contiguous()
    B, sh, sw, _ = x.shape
    if out is None:
        out = torch.empty((B, 3, dh, dw), dtype=torch.float32, device=x.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, 3, dh, dw)):
        raise ValueError(f'out must be a contiguous float32 CUDA tensor {(B, 3, dh, dw)}')
    xt, yt = _linear_dev(sw, dw, True, x.device), _linear_dev(sh, dh, False, x.device)
    L.check(L.lib().octseg_ingest_image(L.ptr(x), B, sh, sw, int(bool(swap_rb)), L.ptr(out), dh, dw, L.ptr(xt), L.ptr(yt), L.stream_ptr()))
    return out


def select_resize_mask(masks_u8, class_ids, size, out=None):
    """dataset.py:111-118: ``cv2.resize(mask, (W, H), INTER_NEAREST)``, channel ``class_id - 1`` per class, bool -> float:
    [B,Hs,Ws,Cs] uint8 CUDA -> [B,len(class_ids),H,W] float32 0/1.  ``class_ids``: the reference's 1-based CLASS_IDS values."""
    _check_u8(masks_u8, 'masks_u8')
    dh, dw = _size2(size)
    ids = [int(c) for c in class_ids]
    x = masks_u8.contiguous()
    B, sh, sw, cs = x.shape
    if not ids or min(ids) < 1 or max(ids) > cs:
        raise ValueError(f'class_ids {ids} do not fit a mask of {cs} channels')
    if out is None:
        out = torch.empty((B, len(ids), dh, dw), dtype=torch.float32, device=x.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, len(ids), dh, dw)):
        raise ValueError(f'out must be a contiguous float32 CUDA tensor {(B, len(ids), dh, dw)}')
    rows, cols, ch = _nearest_dev(sh, dh, x.device), _nearest_dev(sw, dw, x.device), _channels_dev(ids, x.device)
    L.check(L.lib().octseg_ingest_mask(L.ptr(x), B, sh, sw, cs, L.ptr(ch), len(ids), L.ptr(out), dh, dw, L.ptr(rows), L.ptr(cols),
                                       L.stream_ptr()))
    return out
