"""Ensemble inference, host mirror of the reference's ``src/predict.py:23-101``.

Per class the reference loads ``<models_dir>/<LM|FC_LC|VV>/{config.json,weights.ckpt}``, resizes every image
to that model's ``input_size``, runs ``model.predict`` frame by frame (no normalisation, sigmoid > 0.5),
nearest-resizes the mask to ``output_size`` and writes channel ``MODELS_META[class]['index']`` into
``mask[:, :, CLASS_ID - 1]``.  Same semantics here; two deliberate host-side differences, both
result-neutral: the FC_LC network is run once for its two classes instead of twice,
and frames go through the engine in batches.  cv2 is absent in this image, so the two OpenCV resizes on the path
are restated from OpenCV 4.8.1 (``environment.yaml:23``) ``modules/imgproc/src/resize.cpp`` in integer / double
arithmetic: ``INTER_NEAREST`` of the predicted mask (``resizeNN``: ``min(floor(x * (1 / (dst / src))), src - 1)``) as
index tables for the GPU epilogue, and the default 8-bit ``INTER_LINEAR`` of ``preprocessing_img`` (``resizeGeneric_``
with 11-bit fixed-point coefficients, no antialiasing) in numpy.
"""
import json
import os

import numpy as np
import torch
from PIL import Image

from .model import CLASS_IDS, OCTSegmentationModel

MODELS_META = {
    'Lumen': {'model_dir': 'LM', 'index': 0},
    'Lipid core': {'model_dir': 'FC_LC', 'index': 0},
    'Fibrous cap': {'model_dir': 'FC_LC', 'index': 1},
    'Vasa vasorum': {'model_dir': 'VV', 'index': 0},
}


def load_model(model_dir, device='cuda', compute_dtype=torch.bfloat16, use_graph=False):
    """predict.py:31-50."""
    with open(os.path.join(model_dir, 'config.json')) as f:
        cfg = json.load(f)
    model = OCTSegmentationModel.load_from_checkpoint(
        checkpoint_path=os.path.join(model_dir, 'weights.ckpt'), encoder_weights=None, arch=cfg['architecture'],
        encoder_name=cfg['encoder'], model_name=cfg['model_name'], in_channels=3, classes=cfg['classes'],
        map_location=device, compute_dtype=compute_dtype)
    model.eval()
    # serving option: every eval forward of a (B, H, W) plan replays one captured hipGraph (bit-exact; measured no faster
    # than the eager launches on MI355X -- 5.87 vs 5.74 ms at B=1 704x704 -- so it is off unless asked for)
    model.model.use_graph = bool(use_graph)
    return model, cfg


def cv2_linear_coeffs(src, dst, horizontal=True):
    """Per output coordinate: (first tap index, second tap index, 11-bit coefficient pair) of OpenCV's 8-bit INTER_LINEAR
    (resize.cpp ``resize_``: ``fx = (float)((dx + 0.5) * scale - 0.5)``, ``saturate_cast<short>(coef * INTER_RESIZE_COEF_SCALE)``,
    INTER_RESIZE_COEF_SCALE = 2048).  Horizontal taps that leave the row get fx = 0; the vertical table keeps its fraction
    and clips the two row indices (resizeGeneric_Invoker)."""
    scale = 1.0 / (dst / float(src))                      # scale_x = 1. / inv_scale_x, both double
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)      # the (float) cast
    s0 = np.floor(f).astype(np.int64)
    f = (f - s0.astype(np.float32)).astype(np.float32)
    if horizontal:
        lo = s0 < 0
        f[lo] = 0.0; s0[lo] = 0
        hi = s0 >= src - 1
        f[hi] = 0.0; s0[hi] = src - 1
    s1 = np.clip(s0 + 1, 0, src - 1)
    s0 = np.clip(s0, 0, src - 1)
    one = np.float32(1.0)
    a0 = np.rint((one - f) * np.float32(2048.0)).astype(np.int64)   # cvRound: round half to even, as np.rint
    a1 = np.rint(f * np.float32(2048.0)).astype(np.int64)
    return s0, s1, a0, a1


def _is_exact_half(src, dst):
    """OpenCV's ``is_area_fast && iscale == 2`` per axis: scale = 1. / ((double)dst / src), iscale = saturate_cast<int>(scale) (= cvRound),
    |scale - iscale| < DBL_EPSILON."""
    scale = 1.0 / (dst / float(src))
    return int(np.rint(scale)) == 2 and abs(scale - 2.0) < np.finfo(np.float64).eps


def cv2_resize_linear_u8(img, dst_w, dst_h):
    """``cv2.resize(img_u8, (dst_w, dst_h))`` (default INTER_LINEAR) restated: horizontal pass in int32 with 11-bit
    coefficients, vertical pass ``(((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2`` (VResizeLinear<uchar>); an exact 2x
    decimation in both axes (e.g. 1024 -> 512) takes OpenCV's INTER_AREA fast path instead, as cv::resize does."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    squeeze = img.ndim == 2
    if squeeze:
        img = img[:, :, None]
    H, W = img.shape[:2]
    if _is_exact_half(W, dst_w) and _is_exact_half(H, dst_h):
        # cv::resize switches INTER_LINEAR to INTER_AREA for an exact 2x decimation (resize.cpp: `interpolation == INTER_LINEAR &&
        # is_area_fast && iscale_x == 2 && iscale_y == 2`); the 8-bit fast path (ResizeAreaFastVec, cn = 1 / 3 / 4) averages each
        # 2x2 block as (a + b + c + d + 2) >> 2
        s = img.astype(np.int64)
        out = ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
        return out[:, :, 0] if squeeze else out
    x0, x1, ax0, ax1 = cv2_linear_coeffs(W, dst_w)
    y0, y1, ay0, ay1 = cv2_linear_coeffs(H, dst_h, horizontal=False)
    src = img.astype(np.int64)
    rows = src[:, x0, :] * ax0[None, :, None] + src[:, x1, :] * ax1[None, :, None]      # [H, dst_w, C], <= 255 * 2048
    S0, S1 = rows[y0], rows[y1]
    out = (((ay0[:, None, None] * (S0 >> 4)) >> 16) + ((ay1[:, None, None] * (S1 >> 4)) >> 16) + 2) >> 2
    out = np.clip(out, 0, 255).astype(np.uint8)
    return out[:, :, 0] if squeeze else out


def preprocessing_img(img, input_size):
    """data/utils.py:159-166: np.array(img) -> cvtColor RGB2BGR -> cv2.resize(image, (input_size, input_size))."""
    image = np.asarray(img.convert('RGB'))[:, :, ::-1]
    return cv2_resize_linear_u8(np.ascontiguousarray(image), input_size, input_size)


def cv2_nearest_index(src, dst):
    """Source index of every output coordinate of ``cv2.resize(..., interpolation=cv2.INTER_NEAREST)`` (predict.py:92-96).
    OpenCV's ``resizeNN``: ``ifx = 1. / fx`` with ``fx = (double)dst / src``, ``sx = min(cvFloor(x * ifx), src - 1)`` --
    no half-pixel centre (INTER_NEAREST_EXACT would have one; the reference does not use it)."""
    ifx = 1.0 / (float(dst) / float(src))
    x = np.arange(dst, dtype=np.float64)
    return np.minimum(np.floor(x * ifx).astype(np.int64), src - 1).astype(np.int32)


def pil_nearest_index(src, dst):
    """Source index of every output pixel of ``PIL.Image.resize((dst, ...), NEAREST)`` (Pillow steps a double by src/dst from
    src/dst/2 and truncates).  NOT the rule of ``segment()`` -- kept for callers that resample label images with Pillow."""
    a0 = src / dst
    xx = a0 * 0.5
    out = np.empty(dst, dtype=np.int32)
    for i in range(dst):
        out[i] = min(int(xx), src - 1)
        xx += a0
    return out


def _upload_frames_u8(images, device):
    """The PIL frames as uint8 RGB on the device, uploaded once: one stacked [n,H,W,3] tensor when they share a size, else a list of
    [1,H,W,3] tensors."""
    arrs = [np.array(img.convert('RGB')) for img in images]
    if all(a.shape == arrs[0].shape for a in arrs):
        return torch.from_numpy(np.stack(arrs)).to(device)
    return [torch.from_numpy(a)[None].to(device) for a in arrs]


def _resize_frames_on_device(frames, lo, hi, size):
    """preprocessing_img of frames lo..hi-1 on the GPU (octseg_ingest_image, RGB -> BGR planes): float32 [hi - lo, 3, size, size]."""
    from . import ingest
    if torch.is_tensor(frames):
        return ingest.resize_image_u8(frames[lo:hi], size, swap_rb=True)
    hi = min(hi, len(frames))
    out = torch.empty((hi - lo, 3, size, size), dtype=torch.float32, device=frames[lo].device)
    for k in range(lo, hi):
        ingest.resize_image_u8(frames[k], size, swap_rb=True, out=out[k - lo:k - lo + 1])
    return out


def segment_stack(images, output_size, classes, models_dir, device='cuda', batch_size=8, compute_dtype=torch.bfloat16, use_graph=False,
                  device_preprocess=False, thresholds=None):
    """``segment()`` up to and including the mask assembly, with the result left where it was made: the float32 0 / 1 stack
    [n, output_size[0], output_size[1], 4] on the device (channel = CLASS_ID - 1; classes that were not asked for stay 0).  What
    ``postprocess.save_results`` / ``render_results`` take; ``segment()`` copies it to the host arrays of the reference's interface.
    ``images``: the list of PIL images, or a uint8 CUDA tensor [n, H, W, 3] of RGB frames, which takes the device-preprocess path as it is.
    ``thresholds`` (default ``None``: nothing changes): ``{class name: t}``; the logits channel of each class named is shifted by
    ``curves.apply_thresholds`` before the assembly, so that its mask is cut at ``t`` instead of 0.5."""
    from . import _lib as L
    if thresholds is not None:
        from .curves import apply_thresholds, read_thresholds
        thresholds = read_thresholds(thresholds)
    frames_u8 = None
    if torch.is_tensor(images):     # frames that are on the device already (pullback.normalize_volume / resize_pil_u8): nothing to upload
        if not (images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4 and images.shape[3] == 3 and images.shape[0] > 0):
            raise ValueError('a frame tensor must be a non-empty uint8 CUDA tensor [n, H, W, 3] (RGB)')
        frames_u8, device, device_preprocess = images.contiguous(), images.device, True
    n = len(images)
    # cv2 sizes are (width, height); the reference allocates masks as [output_size[0], output_size[1], 4] and resizes
    # to tuple(output_size): the assignment into mask[:, :, c] only works for square sizes, and so do the extents below
    oh, ow = int(output_size[0]), int(output_size[1])
    stack = torch.zeros((n, oh, ow, 4), dtype=torch.float32, device=device)
    cache, tables, loaded = {}, {}, {}
    if frames_u8 is None and device_preprocess:
        frames_u8 = _upload_frames_u8(images, device)
    for class_name in classes:     # every distinct model once: weights and the preprocessed frames at that model's input size
        model_dir = os.path.join(models_dir, MODELS_META[class_name]['model_dir'])
        if model_dir not in loaded:
            model, cfg = load_model(model_dir, device, compute_dtype, use_graph=use_graph)
            # host path: the preprocessed frames [n, S, S, 3]; device path: just S, the frames are resized per batch below
            loaded[model_dir] = (model, int(cfg['input_size']) if device_preprocess else
                                 np.array([preprocessing_img(img, cfg['input_size']) for img in images]))
    parts = {d: [] for d in loaded}
    for i in range(0, n, batch_size):
        if use_graph:
            # the replayed forwards of the (up to three) nets are started together, each on its plan's own stream, and joined in order:
            # at one frame per step a single net fills a fraction of the chip (SegNet.forward_async)
            handles = {}
            for d, (model, batch) in loaded.items():
                if device_preprocess:
                    x = _resize_frames_on_device(frames_u8, i, i + batch_size, batch)
                else:
                    x = torch.as_tensor(np.ascontiguousarray(batch[i:i + batch_size].transpose((0, 3, 1, 2))), dtype=torch.float32).to(model.model.device)
                handles[d] = model.model.eval().forward_async(x, normalize=False)
            for d, h in handles.items():
                parts[d].append(loaded[d][0].model.forward_join(h))
        else:
            for d, (model, batch) in loaded.items():
                parts[d].append(model.predict_logits(_resize_frames_on_device(frames_u8, i, i + batch_size, batch) if device_preprocess
                                                     else batch[i:i + batch_size]))
    for d in loaded:
        cache[d] = torch.cat(parts[d], dim=0)
    del loaded
    for class_name in classes:
        meta = MODELS_META[class_name]
        model_dir = os.path.join(models_dir, meta['model_dir'])
        z = cache[model_dir]
        ch = meta['index'] if z.shape[1] > 1 else 0
        key = (z.shape[2], z.shape[3])
        if key not in tables:   # cv2.resize(predict_mask, tuple(output_size), INTER_NEAREST): resizeNN's row / column tables
            tables[key] = (torch.from_numpy(cv2_nearest_index(z.shape[2], oh)).to(device),
                           torch.from_numpy(cv2_nearest_index(z.shape[3], ow)).to(device))
        rows, cols = tables[key]
        if thresholds is not None and class_name in thresholds:
            apply_thresholds(z, [int(ch)], [thresholds.pop(class_name)])      # (popped: a class listed twice is shifted once)
        L.check(L.lib().octseg_mask_assemble(L.ptr(z), n, z.shape[1], z.shape[2], z.shape[3], int(ch), L.ptr(stack), oh, ow, 4,
                                             CLASS_IDS[class_name] - 1, L.ptr(rows), L.ptr(cols), L.stream_ptr()))
    return stack


def segment(images, masks, output_size, classes, models_dir, device='cuda', batch_size=8, compute_dtype=torch.bfloat16,
            use_graph=False, device_preprocess=False):
    """predict.py:61-101.  images: list of PIL images; masks: list of zero arrays [H_out, W_out, 4].

    ``device_preprocess`` (default off: the host path above stays what every existing caller gets): every frame is uploaded ONCE as
    uint8 RGB and resized to each model's ``input_size`` on the GPU (``ingest.resize_image_u8``, equal to ``preprocessing_img`` sample
    for sample), batch by batch; the nets take those tensors as they are -- no numpy resize and no float32 host-to-device copy.

    Every model runs once (the reference runs FC_LC once per class), in batches (with ``use_graph`` the nets' replayed forwards side by
    side); thresholding, the nearest resize to
    ``output_size`` and the 4-channel mask assembly happen on the GPU (``octseg_mask_assemble``); one D2H copy of the
    assembled 0/1 stack at the end instead of one logits tensor per frame and class."""
    stack = segment_stack(images, masks[0].shape[:2], classes, models_dir, device=device, batch_size=batch_size, compute_dtype=compute_dtype,
                          use_graph=use_graph, device_preprocess=device_preprocess)
    host = stack.cpu().numpy()
    for i, mask in enumerate(masks):
        for class_name in classes:
            c = CLASS_IDS[class_name] - 1
            mask[:, :, c] = host[i, :, :, c]
    return masks


def data_processing(image_paths, output_size):
    """data/utils.py:169-192 without the directory creation."""
    images, masks = [], []
    for p in image_paths:
        images.append(Image.open(p).resize(tuple(output_size)))
        masks.append(np.zeros((output_size[0], output_size[1], 4)))
    return images, masks


def _frames_on_device(image_paths, output_size, device):
    """``data_processing`` with the resize on the GPU: every file whose PIL mode is ``RGB`` or ``L`` goes up at SOURCE size and is resized by
    ``pullback.resize_pil_u8`` (equal to ``Image.resize`` byte for byte; an ``L`` frame is spread to three channels afterwards, as
    ``convert('RGB')`` does).  Other modes keep the host ``Image.resize``: Pillow resizes ``P`` with NEAREST and ``RGBA`` premultiplied.
    Returns the frames at output size, uint8 CUDA [n, output_size[1], output_size[0], 3] in path order."""
    from .pullback import resize_pil_u8
    ow, oh = int(output_size[0]), int(output_size[1])          # Image.resize takes (width, height)
    frames = torch.empty((len(image_paths), oh, ow, 3), dtype=torch.uint8, device=device)
    groups = {}
    for i, p in enumerate(image_paths):
        img = Image.open(p)
        if img.mode in ('RGB', 'L'):
            a = np.asarray(img)
            groups.setdefault(a.shape, []).append((i, a))
        else:
            frames[i] = torch.from_numpy(np.array(img.resize((ow, oh)).convert('RGB'))).to(device)
    for items in groups.values():
        src = np.stack([a for _, a in items])
        out = resize_pil_u8(torch.from_numpy(src.reshape(src.shape[:3] + (-1,))).to(device), (oh, ow))
        frames[torch.tensor([i for i, _ in items], device=device)] = out.expand(-1, -1, -1, 3)
    return frames


def _main_volume(cfg, device, dtypes, log):
    """``data_dir`` is a ``.npy`` file: a raw volume [S,H,W,3] | [S,H,W], uint8 | uint16 (a DICOM's ``pixel_array``), through
    ``pullback.analyze_pullback``.  Slice ``k`` (from 1) is written as ``{stem}_{k:03d}_mask.png`` / ``_overlay.png``, the names
    convert_dicoms gives its frames."""
    from .pullback import analyze_pullback
    folds, tta, _ = _vote_keys(cfg)
    if folds or tta != 'none':      # analyze_pullback segments with one network per class: refuse, do not quietly serve an unvoted stack
        raise ValueError('folds / tta vote over image files only: a .npy volume goes through pullback.analyze_pullback, which does not vote')
    path = str(cfg['data_dir'])
    volume = np.load(path)
    stem = os.path.basename(path).split('.')[0]
    names = [f'{stem}_{k + 1:03d}' for k in range(volume.shape[0])]
    log.info(f'Number of slices: {len(names)}')
    res = analyze_pullback(volume, str(cfg['models_dir']), cfg['classes'], output_size=cfg['output_size'], names=names, render=True,
                           close_iterations=int(cfg.get('close_iterations', 1)), device=device, batch_size=int(cfg.get('batch_size', 8)),
                           compute_dtype=dtypes[str(cfg.get('compute_dtype', 'bf16'))], use_graph=bool(cfg.get('use_graph', False)),
                           clean=bool(cfg.get('clean', False)), plaque=bool(cfg.get('plaque', False)), lumen=bool(cfg.get('lumen', False)))
    out = torch.stack([res.overlay, res.color_mask]).cpu().numpy()
    save_dir = str(cfg['save_dir'])
    for i, name in enumerate(names):
        Image.fromarray(out[1, i]).save(f'{save_dir}/{name}_mask.png')
        Image.fromarray(out[0, i]).save(f'{save_dir}/{name}_overlay.png')
    if bool(cfg.get('analysis', False)):
        with open(os.path.join(save_dir, 'analysis.json'), 'w') as f:
            json.dump(res.data, f)
    if res.plaque is not None:
        _save_plaque(res.plaque, res.stack, cfg['classes'], save_dir)
    if bool(cfg.get('lesions', False)):
        _save_lesions(res.stack, names, save_dir)
    if bool(cfg.get('medial', False)):
        _save_medial(res.stack, names, save_dir, int(cfg.get('medial_spur') or 0), int(cfg.get('medial_trim') or 0))
    if res.lumen is not None:
        _save_lumen(res.lumen, save_dir)
    if bool(cfg.get('contours', False)):
        _save_contours(res.stack, names, save_dir)


def _bridge(stack, paths, names, max_gap, save_dir):
    """``bridge=K``: the stack with gaps of at most K slices filled (``interp.bridge_gaps`` over the slices in sorted file-name order), in the
    order it came in, and ``{save_dir}/bridge.json``, ``interp.bridge_report`` of what was made."""
    from .interp import bridge_gaps, bridge_report
    order = sorted(range(len(paths)), key=lambda i: os.path.basename(paths[i]))
    index = torch.tensor(order, device=stack.device)
    bridged, plan, made = bridge_gaps(stack[index], max_gap=max_gap, return_plan=True)
    with open(os.path.join(save_dir, 'bridge.json'), 'w') as f:
        json.dump({'max_gap': int(max_gap), 'images': [names[i] for i in order],
                   'classes': bridge_report(plan, made, [names[i] for i in order], channels=int(stack.shape[3]))}, f)
    out = torch.empty_like(bridged)
    out[index] = bridged
    return out


def _save_lumen(report, save_dir):
    """``lumen=true``: ``{save_dir}/lumen.json``, ``shape.lumen_report`` of the stack that is rendered and measured (after ``clean``)."""
    with open(os.path.join(save_dir, 'lumen.json'), 'w') as f:
        json.dump(report, f)


def _save_contours(stack, names, save_dir):
    """``contours=true``: ``{save_dir}/contours.json``, ``contours.contour_report`` of the stack that is rendered and measured (after ``clean``)."""
    from .contours import contour_report
    with open(os.path.join(save_dir, 'contours.json'), 'w') as f:
        json.dump(contour_report(stack, names), f)


def _save_lesions(stack, names, save_dir):
    """``lesions=true``: ``{save_dir}/lesions.json``, ``lesions.lesion_report`` of the stack, slices in the order given."""
    from .lesions import lesion_report
    with open(os.path.join(save_dir, 'lesions.json'), 'w') as f:
        json.dump(lesion_report(stack, names), f)


def _save_medial(stack, names, save_dir, spur=0, trim=0):
    """``medial=true``: ``{save_dir}/medial_thickness.json``, ``skeleton.thickness_report`` of the stack, slices in the order given.  With
    ``medial_spur`` or ``medial_trim`` above 0 the report is that of the pruned centreline and carries ``spur`` and ``trim`` at top level."""
    from .skeleton import thickness_report
    report = thickness_report(stack, names=names, spur=spur, trim=trim)
    if spur or trim:
        report = {'spur': spur, 'trim': trim, **report}
    with open(os.path.join(save_dir, 'medial_thickness.json'), 'w') as f:
        json.dump(report, f)


def _save_plaque(report, stack, classes, save_dir):
    """``plaque=true``: ``{save_dir}/plaque.json`` (``polar.plaque_report``) and ``plaque_carpet.png`` (``polar.carpet_view``: rows are degrees,
    columns the slices in the report's order)."""
    from .polar import carpet_view, polar_profile
    with open(os.path.join(save_dir, 'plaque.json'), 'w') as f:
        json.dump(report, f)
    Image.fromarray(carpet_view(polar_profile(stack), classes)).save(os.path.join(save_dir, 'plaque_carpet.png'))


def _vote_keys(cfg):
    """The three voting keys: ``folds`` (default false), ``tta`` (``none`` | ``flips`` | ``d4``, default ``none``), ``vote`` (``soft`` | ``majority``,
    default ``soft``).  Unknown names are refused here, before anything is loaded."""
    folds, tta, mode = bool(cfg.get('folds', False)), str(cfg.get('tta') or 'none'), str(cfg.get('vote') or 'soft')
    if tta not in ('none', 'flips', 'd4'):
        raise ValueError(f'tta must be none, flips or d4, got {tta!r}')
    if mode not in ('soft', 'majority'):
        raise ValueError(f'vote must be soft or majority, got {mode!r}')
    return folds, tta, mode


def _threshold_key(cfg):
    """The ``thresholds`` key (absent by default): the path of a ``curves.json`` or ``{class name: t}``, as ``{class name: t}`` or ``None``.  Unknown
    class names and ``t`` outside (0, 1) are refused here, before anything is loaded."""
    if cfg.get('thresholds') is None:
        return None
    from .curves import read_thresholds
    return read_thresholds(cfg['thresholds'])


def _save_vote(voted, paths, names, classes, save_dir):
    """A voted prediction's own files: ``{save_dir}/vote.json`` (``vote.vote_report``, slices in sorted file-name order, as ``analysis`` uses) and,
    where the dissent maps were asked for, ``{name}_dissent.png`` per frame (``vote.dissent_images``)."""
    from .vote import dissent_images, vote_report
    order = sorted(range(len(paths)), key=lambda i: os.path.basename(paths[i]))
    ordered = voted._replace(stats=voted.stats[torch.tensor(order, device=voted.stats.device)])
    with open(os.path.join(save_dir, 'vote.json'), 'w') as f:
        json.dump(vote_report(ordered, [names[i] for i in order], classes), f)
    if voted.dissent is not None:
        for name, img in zip(names, dissent_images(voted, classes)):
            Image.fromarray(img).save(f'{save_dir}/{name}_dissent.png')


def _image_paths(data_path):
    """data/utils.py:175-178: one file, or the directory's ``*.[pj][np][ge]*`` (png, jpg, jpeg ...)."""
    if os.path.isfile(data_path):
        return [data_path]
    from glob import glob
    return glob(f'{data_path}/*.[pj][np][ge]*')


def main(argv=None):
    """src/predict.py:109-149 from ``configs/predict.yaml`` (``key=value`` overrides as with hydra): data_processing -> segment -> save_results,
    two PNGs per frame in ``save_dir``.  The frames go up once as uint8, the masks stay on the device from the nets to the rendering kernel
    (``segment_stack`` -> ``postprocess.save_results``); what comes back is the uint8 overlay and colour mask, 6 bytes per pixel instead of the
    16 of the float32 stack.  Extra keys: ``compute_dtype`` (bf16 | fp16 | fp32), ``batch_size``, ``use_graph``, ``close_iterations``, and
    ``analysis`` (default false): also write ``{save_dir}/analysis.json``, the dict of the app's ``get_analysis`` measured on the same stack
    (``analysis.analyze_stack``), with the frames as the slices of one pullback in sorted file-name order, as the app sorts its mask files;
    ``clean`` (default false): the mask stack goes through ``cleanup.clean_stack`` (the reference's ``MaskProcessor``: smoothing, the three
    largest components, hole fill) before it is rendered and measured;
    ``bridge`` (default 0: off, nothing changes): after ``clean`` and before everything that is rendered or measured, gaps of at most ``bridge``
    slices inside a class are filled by interpolation between the neighbouring slices (``interp.bridge_gaps``, slices in the order ``analysis``
    uses) and ``{save_dir}/bridge.json`` (``interp.bridge_report``: per class the slices made, from which, how many pixels) is written; image
    files only;
    ``plaque`` (default false): also write ``{save_dir}/plaque.json``, the polar plaque report of the same stack (``polar.plaque_report``: lipid
    arc, cap thickness where lipid lies behind it), and ``plaque_carpet.png`` (``polar.carpet_view``), slices in the order ``analysis`` uses;
    ``lesions`` (default false): also write ``{save_dir}/lesions.json``, the 3-D lesion report of the same stack (``lesions.lesion_report``:
    components across the slices, their length, voxels, bounding box and area profile), slices in the order ``analysis`` uses;
    ``medial`` (default false): also write ``{save_dir}/medial_thickness.json``, the thickness of every class across its own centreline
    (``skeleton.thickness_report``: skeleton pixels, end and junction points, width statistics per slice), slices in the order ``analysis`` uses;
    ``medial_spur`` / ``medial_trim`` (default 0): the centreline is pruned first (``skeleton.prune_stack``: side branches of at most
    ``medial_spur`` pixels removed, ``medial_trim`` pixels off every end that is left), the report gains ``tips``, ``length``, ``removed`` and
    ``restored`` per class and carries ``spur`` and ``trim`` at top level;
    ``lumen`` (default false): also write ``{save_dir}/lumen.json``, the lumen report of the same stack (``shape.lumen_report``: lumen area and
    the diameters through the lumen's own centroid per frame, the minimal-lumen-area frame, percent area stenosis), slices in the order
    ``analysis`` uses;
    ``contours`` (default false): also write ``{save_dir}/contours.json``, the outlines of the same stack as integer polygons along the pixel
    sides with their holes (``contours.contour_report``; its ``convention`` key states the coordinates), slices in the order ``analysis`` uses;
    ``folds`` (default false), ``tta`` (``none`` | ``flips`` | ``d4``, default ``none``), ``vote`` (``soft`` | ``majority``, default ``soft``): with
    ``folds`` true or a ``tta`` the stack is voted by every ``fold_<k>`` network of a class on every view (``vote.segment_stack_voted``) and
    ``{save_dir}/vote.json`` (``vote.vote_report``) is written, slices in the order ``analysis`` uses; ``dissent_maps`` (default false) adds
    ``{name}_dissent.png`` per frame, grayscale, the maximum over the classes of ``dissent * (255 // members)``;
    ``thresholds`` (absent by default): the path of a ``curves.json`` written by ``python -m oct_segmentation_amd.curves`` or a dict
    ``{"Lumen": 0.4, ...}``: the masks of the classes named are cut at that probability instead of 0.5 (``curves.apply_thresholds`` on the
    logits before the assembly, voted or not); unknown class names and values outside (0, 1) are refused before anything is loaded;
    ``device_resize`` (default true): ``RGB`` and ``L`` files go up at source size and ``data_processing``'s ``Image.resize`` runs on the GPU
    (``pullback.resize_pil_u8``, byte-identical; false restores the host resize for every file).  A ``data_dir`` that is a ``.npy`` file is a
    raw volume (a DICOM's ``pixel_array``) and goes through ``pullback.analyze_pullback``: see ``_main_volume``."""
    import logging
    import sys
    import time
    from .config import load_config
    from .postprocess import save_results
    log = logging.getLogger('oct_segmentation_amd.predict')
    if not logging.getLogger().handlers:
        logging.basicConfig(level=logging.INFO, format='[%(asctime)s][%(name)s][%(levelname)s] - %(message)s')
    cfg = load_config('predict', list(sys.argv[1:] if argv is None else argv))
    thresholds = _threshold_key(cfg)
    device = 'cuda' if cfg.get('device', 'auto') in ('auto', 'gpu', 'cuda') else cfg['device']
    if not (str(device).startswith('cuda') and torch.cuda.is_available()):
        raise RuntimeError(f'predict needs a GPU (device={cfg.get("device")!r}): there is no CPU path')
    dtypes = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
    start = time.time()
    paths = _image_paths(str(cfg['data_dir']))
    if not paths:
        raise FileNotFoundError(f'no images under {cfg["data_dir"]}')
    os.makedirs(str(cfg['save_dir']), exist_ok=True)
    bridge = int(cfg.get('bridge') or 0)
    if bridge < 0:
        raise ValueError(f'bridge must be an integer >= 0 (the longest gap of slices to fill; 0 is off), got {bridge}')
    if str(cfg['data_dir']).endswith('.npy'):
        if bridge:                      # analyze_pullback renders and measures inside: refuse, do not quietly serve the unbridged stack
            raise ValueError('bridge applies to image files only: a .npy volume goes through pullback.analyze_pullback, which does not bridge')
        if thresholds is not None:      # analyze_pullback segments at 0.5: refuse, do not quietly serve the default cut
            raise ValueError('thresholds apply to image files only: a .npy volume goes through pullback.analyze_pullback, which cuts at 0.5')
        _main_volume(cfg, device, dtypes, log)
        log.info(f'Overall computation time: {time.time() - start:.1f} s')
        log.info('Complete')
        return 0
    if bool(cfg.get('device_resize', True)):
        images = _frames_on_device(paths, cfg['output_size'], device)
    else:
        images, _ = data_processing(paths, cfg['output_size'])
    names = [os.path.basename(p).split('.')[0] for p in paths]
    log.info(f'Number of images: {len(names)}')
    start_inference = time.time()
    folds, tta, vote_mode = _vote_keys(cfg)
    voted = None
    if bool(cfg.get('dissent_maps', False)) and not (folds or tta != 'none'):
        raise ValueError('dissent_maps=true needs a vote: folds=true or tta=flips | d4')
    if folds or tta != 'none':
        from .vote import segment_stack_voted
        voted = segment_stack_voted(images, cfg['output_size'], cfg['classes'], str(cfg['models_dir']), tta=tta, folds=folds, mode=vote_mode,
                                    want_dissent=bool(cfg.get('dissent_maps', False)), device=device, batch_size=int(cfg.get('batch_size', 8)),
                                    compute_dtype=dtypes[str(cfg.get('compute_dtype', 'bf16'))], thresholds=thresholds)
        stack = voted.stack
    else:
        stack = segment_stack(images, cfg['output_size'], cfg['classes'], str(cfg['models_dir']), device=device,
                              batch_size=int(cfg.get('batch_size', 8)), compute_dtype=dtypes[str(cfg.get('compute_dtype', 'bf16'))],
                              use_graph=bool(cfg.get('use_graph', False)), device_preprocess=True, thresholds=thresholds)
    if voted is not None:
        _save_vote(voted, paths, names, cfg['classes'], str(cfg['save_dir']))
    if bool(cfg.get('clean', False)):
        from .cleanup import clean_stack
        stack = clean_stack(stack)
    if bridge:
        stack = _bridge(stack, paths, names, bridge, str(cfg['save_dir']))
    torch.cuda.synchronize()
    log.info(f'Prediction time: {time.time() - start_inference:.1f} s')
    save_results(images, stack, names, cfg['classes'], str(cfg['save_dir']), close_iterations=int(cfg.get('close_iterations', 1)))
    if bool(cfg.get('analysis', False)):
        from .analysis import analyze_stack
        order = sorted(range(len(paths)), key=lambda i: os.path.basename(paths[i]))      # _image_paths is the glob's order
        data = analyze_stack(stack[torch.tensor(order, device=stack.device)], [names[i] for i in order])
        with open(os.path.join(str(cfg['save_dir']), 'analysis.json'), 'w') as f:
            json.dump(data, f)
    if bool(cfg.get('plaque', False)):
        from .polar import plaque_report
        order = sorted(range(len(paths)), key=lambda i: os.path.basename(paths[i]))
        ordered = stack[torch.tensor(order, device=stack.device)]
        _save_plaque(plaque_report(ordered, [names[i] for i in order]), ordered, cfg['classes'], str(cfg['save_dir']))
    if bool(cfg.get('lesions', False)):
        order = sorted(range(len(paths)), key=lambda i: os.path.basename(paths[i]))
        _save_lesions(stack[torch.tensor(order, device=stack.device)], [names[i] for i in order], str(cfg['save_dir']))
    if bool(cfg.get('medial', False)):
        order = sorted(range(len(paths)), key=lambda i: os.path.basename(paths[i]))
        _save_medial(stack[torch.tensor(order, device=stack.device)], [names[i] for i in order], str(cfg['save_dir']),
                     int(cfg.get('medial_spur') or 0), int(cfg.get('medial_trim') or 0))
    if bool(cfg.get('lumen', False)):
        from .shape import lumen_report
        order = sorted(range(len(paths)), key=lambda i: os.path.basename(paths[i]))
        _save_lumen(lumen_report(stack[torch.tensor(order, device=stack.device)], [names[i] for i in order]), str(cfg['save_dir']))
    if bool(cfg.get('contours', False)):
        order = sorted(range(len(paths)), key=lambda i: os.path.basename(paths[i]))
        _save_contours(stack[torch.tensor(order, device=stack.device)], [names[i] for i in order], str(cfg['save_dir']))
    log.info(f'Overall computation time: {time.time() - start:.1f} s')
    log.info('Complete')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
