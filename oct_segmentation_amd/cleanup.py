"""Mask clean-up on the GPU: the reference's ``MaskProcessor`` (``src/data/mask_processor.py:5-37``), which ``process_pair`` runs over every
annotated object (``convert_int_to_cv.py:191-199``), for the mask stacks the pipeline carries: connected components, keep-largest, hole fill
and the frame-sized smoothing, all in ``csrc/components.hip`` (``octseg_stack_components`` / ``octseg_stack_cleanup``).

A thresholded network output carries specks; ``analysis.measure_stack`` counts every set pixel and walks its rays into them, and one speck on an
otherwise empty slice makes a class "present" there.  ``clean_stack`` in front of the measurements removes them:

    labels = label_stack(stack)                                # int32 CUDA [N, channels, H, W]: 1 + y * W + x of the first pixel, 0 background
    ncomp, top = component_table(stack)                        # int32 CUDA [N, channels], [N, channels, 8, 6]
    stack = clean_stack(stack)                                 # smooth_mask, keep the 3 largest (ties stay), fill holes

``stack`` is float32 CUDA [N, H, W, channels], any value != 0 set; results are 0.0 / 1.0 in the same layout and feed ``render_results``,
``measure_stack`` and ``analyze_stack`` unchanged.  Components are ranked by PIXEL COUNT, not by ``cv2.contourArea`` over ``RETR_TREE``
contours as ``remove_artifacts`` ranks them: holes never compete for a slot.  Everything is integer: results EQUAL
``scipy.ndimage``'s, no tolerance.  Nothing synchronises with the host; scratch comes from torch's allocator, sized by the library.
"""
import numpy as np
import torch

from . import _lib as L

MAX_CHANNELS = 16
MAX_SMOOTH = 7
TOPK = 8
TOP_COLUMNS = ('area', 'first_pixel', 'x0', 'y0', 'x1', 'y1')
DEFAULT_SCRATCH = 512 << 20


def smooth_kernel_size(h, w):
    """``max(int(0.005 * min_dim), 1)`` (mask_processor.py:16-17)."""
    return max(int(0.005 * min(int(h), int(w))), 1)


def _check(stack):
    if not (torch.is_tensor(stack) and stack.is_cuda and stack.dtype == torch.float32 and stack.dim() == 4):
        raise ValueError('stack must be a float32 CUDA tensor [N, H, W, channels]')
    if 0 in stack.shape:
        raise ValueError('empty batch or frame')
    n, h, w, sc = (int(v) for v in stack.shape)
    if sc > MAX_CHANNELS:
        raise ValueError(f'at most {MAX_CHANNELS} channels, got {sc}')
    if h * w >= 2 ** 31 - 1:
        raise ValueError(f'frame {h} x {w} has 2^31 - 1 pixels or more')
    return stack.contiguous(), n, h, w, sc


def _scratch(planes, h, w, device):
    need = int(L.lib().octseg_components_scratch_bytes(planes, h, w))
    return torch.empty((need,), dtype=torch.uint8, device=device), need


def _slices_per_chunk(n, h, w, sc, scratch_bytes):
    """Slices a call may take under the scratch budget (the library needs about 9.3 bytes per pixel and plane); 0: not even one slice fits."""
    per_slice = int(L.lib().octseg_components_scratch_bytes(sc, h, w))
    return min(n, int(scratch_bytes) // per_slice)


def _components(stack, want_labels, want_table, scratch_bytes=DEFAULT_SCRATCH):
    stack, n, h, w, sc = _check(stack)
    dev = stack.device
    labels = torch.empty((n, sc, h, w), dtype=torch.int32, device=dev) if want_labels else None
    ncomp = torch.empty((n, sc), dtype=torch.int32, device=dev) if want_table else None
    top = torch.empty((n, sc, TOPK, 6), dtype=torch.int32, device=dev) if want_table else None
    step = max(_slices_per_chunk(n, h, w, sc, scratch_bytes), 1)
    with torch.cuda.device(dev):
        scratch, nbytes = _scratch(step * sc, h, w, dev)
        for i in range(0, n, step):
            m = min(step, n - i)
            L.check(L.lib().octseg_stack_components(L.ptr(stack[i:i + m]), m, h, w, sc, L.ptr(scratch), nbytes,
                                                    L.ptr(labels[i:i + m]) if want_labels else None,
                                                    L.ptr(ncomp[i:i + m]) if want_table else None,
                                                    L.ptr(top[i:i + m]) if want_table else None, L.stream_ptr()))
    return labels, ncomp, top


def label_stack(stack, connectivity=8):
    """The 8-connected foreground components of every (slice, channel) plane: int32 CUDA [N, channels, H, W], the label of a component is
    ``1 + y * W + x`` of its first pixel in raster order, background 0 (``scipy.ndimage.label`` with the full 3 x 3 structure, relabelled).
    Storage is per pixel: no cap on the number of components.  The 4-connected form exists only inside the hole fill."""
    if connectivity != 8:
        raise ValueError(f'connectivity must be 8, got {connectivity!r} (4-connectivity is used only inside fill_holes)')
    return _components(stack, True, False)[0]


def component_table(stack):
    """``(ncomp, top)``: int32 CUDA [N, channels], the number of components per plane, and int32 CUDA [N, channels, 8, 6], the 8 largest by
    area descending then first pixel ascending, columns ``TOP_COLUMNS`` (inclusive bounding box); rows beyond ``ncomp`` are zero."""
    return _components(stack, False, True)[1:]


def clean_stack(stack, smooth=True, keep=3, min_area=0, fill_holes=True, return_table=False, scratch_bytes=DEFAULT_SCRATCH):
    """The clean-up chain on every plane: ``smooth_mask`` (``smooth``: True = the reference's size rule, an int = that ellipse size, False /
    0 / 1 = off), then the ``keep`` largest components (ties at the threshold all stay, as the reference's ``area in sorted_areas``;
    ``keep=0``: no rank filter) minus those below ``min_area`` pixels, then the hole fill.  Returns the cleaned stack (float32 0.0 / 1.0, the
    input's layout; the input is not modified); with ``return_table`` also ``(ncomp, top)`` of the kept components before the fill.

    The stack is processed in chunks of slices whose scratch stays under ``scratch_bytes`` (one chunk when it fits; channel by channel when
    not even one slice fits); the result does not depend on the chunking."""
    stack, n, h, w, sc = _check(stack)
    if smooth is True:
        k = smooth_kernel_size(h, w)
    elif smooth is False or smooth is None:
        k = 0
    else:
        k = int(smooth)
    if k < 0 or k > MAX_SMOOTH:
        raise ValueError(f'smoothing ellipse size must be 1..{MAX_SMOOTH} (frames whose short side is below 1600), got {k}')
    keep, min_area = int(keep), int(min_area)
    if keep < 0 or min_area < 0:
        raise ValueError('keep and min_area must not be negative')
    dev = stack.device
    out = torch.empty_like(stack)
    ncomp = torch.empty((n, sc), dtype=torch.int32, device=dev) if return_table else None
    top = torch.empty((n, sc, TOPK, 6), dtype=torch.int32, device=dev) if return_table else None

    def run(src, dst, m, ch, nc, tp, scratch, nbytes):
        L.check(L.lib().octseg_stack_cleanup(L.ptr(src), m, h, w, ch, k, keep, min_area, int(bool(fill_holes)), L.ptr(scratch), nbytes,
                                             L.ptr(dst), L.ptr(nc), L.ptr(tp), L.stream_ptr()))

    step = _slices_per_chunk(n, h, w, sc, scratch_bytes)
    with torch.cuda.device(dev):
        if step >= 1:
            scratch, nbytes = _scratch(step * sc, h, w, dev)
            for i in range(0, n, step):
                m = min(step, n - i)
                run(stack[i:i + m], out[i:i + m], m, sc, ncomp[i:i + m] if return_table else None, top[i:i + m] if return_table else None,
                    scratch, nbytes)
        else:                                  # one plane at a time: a channel is copied out, cleaned and copied back
            scratch, nbytes = _scratch(1, h, w, dev)
            nc1 = torch.empty((1, 1), dtype=torch.int32, device=dev) if return_table else None
            tp1 = torch.empty((1, 1, TOPK, 6), dtype=torch.int32, device=dev) if return_table else None
            for i in range(n):
                for c in range(sc):
                    src = stack[i:i + 1, :, :, c:c + 1].contiguous()
                    dst = torch.empty_like(src)
                    run(src, dst, 1, 1, nc1, tp1, scratch, nbytes)
                    out[i:i + 1, :, :, c:c + 1] = dst
                    if return_table:
                        ncomp[i, c] = nc1[0, 0]
                        top[i, c] = tp1[0, 0]
    return (out, (ncomp, top)) if return_table else out


def smooth_stack(stack, kernel_size=None):
    """``MaskProcessor.smooth_mask`` on every plane: open, close, dilate with ``cv2.getStructuringElement(MORPH_ELLIPSE, (k, k))`` (anchor
    ``k // 2``, the element not reflected, outside the frame not taking part).  ``kernel_size=None``: the reference's
    ``k = max(int(0.005 * min(H, W)), 1)``; 1 is the identity; above 7 is refused."""
    return clean_stack(stack, smooth=True if kernel_size is None else int(kernel_size), keep=0, min_area=0, fill_holes=False)


def keep_largest(stack, keep=3, min_area=0, fill_holes=True):
    """``MaskProcessor.remove_artifacts`` on every plane, on components by pixel count: see ``clean_stack``."""
    return clean_stack(stack, smooth=False, keep=keep, min_area=min_area, fill_holes=fill_holes)


class MaskProcessor:
    """The reference's class: a 2-D numpy mask in, a uint8 0 / 1 mask out.  One upload, the kernels, one download per call."""

    @staticmethod
    def _run(mask, device, **kw):
        mask = np.asarray(mask)
        if mask.ndim != 2:
            raise ValueError(f'mask must be 2-D, got shape {mask.shape}')
        stack = torch.from_numpy(np.ascontiguousarray(mask != 0).astype(np.float32)).to(device)[None, :, :, None]
        return clean_stack(stack, **kw)[0, :, :, 0].to(torch.uint8).cpu().numpy()

    @staticmethod
    def smooth_mask(mask, device='cuda'):
        return MaskProcessor._run(mask, device, smooth=True, keep=0, fill_holes=False)

    @staticmethod
    def remove_artifacts(mask, device='cuda'):
        return MaskProcessor._run(mask, device, smooth=False, keep=3, fill_holes=True)


def clean_kwargs(clean):
    """The ``clean`` argument of ``analyze_stack`` / ``analyze_pullback``: None / False = off, True = ``clean_stack``'s defaults, a dict = its
    keywords.  Returns None (off) or the keyword dict."""
    if clean is None or clean is False:
        return None
    if clean is True:
        return {}
    if isinstance(clean, dict):
        bad = set(clean) - {'smooth', 'keep', 'min_area', 'fill_holes', 'scratch_bytes'}
        if bad:
            raise ValueError(f'unknown clean_stack keywords: {sorted(bad)}')
        return dict(clean)
    raise ValueError(f'clean must be None, a bool or a dict of clean_stack keywords, got {clean!r}')
