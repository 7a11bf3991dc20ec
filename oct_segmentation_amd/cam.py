"""Class activation maps on the GPU: the reference's ``src/models/cam_processor.py`` (``CAMProcessor`` over the pytorch-grad-cam
package) and its tool ``src/models/visualize_activation_maps.py``, configured by ``configs/visualize_activation_maps.yaml``.

The engine has no per-layer modules to hook.  A dedicated plan per ``(B, H, W)`` runs the training op path with every BatchNorm frozen on
its running statistics (the reference explains ``model.eval()``), keeps the output ``A`` of ``encoder.layer4[-1]``, and a seeded data-only
backward (``dL/dlogits`` = the predicted mask on the class plane: ``SemanticSegmentationTarget``) leaves ``G = dL/dA`` in the workspace.
``csrc/cam.hip`` turns ``A, G`` into the map, the thresholded map, its confusion counts against the ground truth and the JET overlay;
only what is saved comes back to the host.  Restated from pytorch-grad-cam 1.5.0 (the package is not a dependency and no test runs it: parity with it
is not pinned; DESIGN.md section 5e lists the deviations).

Runs: GradCAM, HiResCAM, GradCAMElementWise, GradCAMPlusPlus, XGradCAM, LayerCAM.  Refused with a reason: AblationCAM, EigenCAM,
EigenGradCAM, the smoothing flags, any target layer but ``model.model.encoder.layer4[-1]``, and the graphs listed in ``unsupported_reason``.

    python -m oct_segmentation_amd.cam cam_method=XGradCAM model_dir=models/LM data_dir=data/final
"""
import csv
import os

import numpy as np
import torch

from . import _lib as L
from .model import CLASS_IDS

CAM_METHODS = {'GradCAM': 0, 'HiResCAM': 1, 'GradCAMElementWise': 2, 'GradCAMPlusPlus': 3, 'XGradCAM': 4,
               'AblationCAM': None, 'EigenCAM': None, 'EigenGradCAM': None, 'LayerCAM': 5}
_REFUSED = {'AblationCAM': 'ablation needs the network re-executed from a mid-graph tensor, once per channel group; the engine runs whole plans only',
            'EigenCAM': "the map is a projection on the first right-singular vector, whose sign is LAPACK's choice and cannot be pinned here",
            'EigenGradCAM': "the map is a projection on the first right-singular vector, whose sign is LAPACK's choice and cannot be pinned here"}
CLASS_IDS_REVERSED = {v: k for k, v in CLASS_IDS.items()}
CSV_COLUMNS = ['Image path', 'Image name', 'Class', 'Class ID', 'CAM', 'Model', 'Dice', 'IoU', 'Precision', 'Recall', 'F1']
_CAM_ARCHS = ('unet', 'unetplusplus', 'linknet', 'manet')


def unsupported_reason(arch, encoder_name, dtype_code=L.F32):
    """Why this (arch, encoder, dtype) has no class-activation-map path, or None.  Mirrors octseg_plan_set_frozen_bn's refusals."""
    arch = arch.lower()
    if dtype_code == L.F16:
        return 'float16 is a serving dtype: it has no backward, so no class activation maps'
    if not encoder_name.startswith('resnet'):
        return f"encoder '{encoder_name}' has no encoder.layer4 (the reference's target layer does not exist there either)"
    if arch in ('pan', 'deeplabv3', 'deeplabv3plus'):
        return f"arch '{arch}': encoder.layer4 runs dilated, in a parity-re-arranged layout; its block output is not the reference's tensor"
    if arch in ('fpn', 'pspnet'):
        return f"arch '{arch}': the graph holds a dropout op" + ('; PSPNet never runs encoder.layer4' if arch == 'pspnet' else '')
    if arch not in _CAM_ARCHS:
        return f"arch '{arch}' has no class-activation-map path"
    return None


def jet_table_bgr():
    """The 256-entry colour table of the overlay, uint8 [256, 3] in BGR.  OpenCV's own COLORMAP_JET table is not restated in this project; this is
    the closed form r = clamp(1.5 - |4v - 3|), g = clamp(1.5 - |4v - 2|), b = clamp(1.5 - |4v - 1|), v = i / 255, clamps to [0, 1],
    rounded to 8 bits -- a documented deviation of a few grey levels."""
    v = np.arange(256, dtype=np.float64) / 255.0
    ch = [np.clip(1.5 - np.abs(4.0 * v - k), 0.0, 1.0) for k in (1.0, 2.0, 3.0)]     # b, g, r
    return np.rint(np.stack(ch, axis=1) * 255.0).astype(np.uint8)


def metrics_from_counts(tp, pred, true):
    """sklearn's f1 / jaccard / precision / recall with average='micro' on 2-D 0/255 arrays (read as multilabel indicators: the binary
    metric over all pixels with non-zero as positive) from the integer counts tp = |pred and true|, pred, true; 0 / 0 -> 0."""
    tp, pred, true = int(tp), int(pred), int(true)
    div = lambda a, b: a / b if b else 0.0   # noqa: E731
    dice = div(2 * tp, pred + true)
    return {'Dice': dice, 'IoU': div(tp, pred + true - tp), 'Precision': div(tp, pred), 'Recall': div(tp, true), 'F1': dice}


def class_name_of(class_idx):
    """visualize_activation_maps.py:151: the class INDEX of the model is used as a CLASS_ID (and, at :172, as the TIFF channel), whatever the
    model's class list says -- the reference's quirk, mirrored."""
    return CLASS_IDS_REVERSED[class_idx + 1]


def output_names(stem, class_name, cam_method):
    """The five files per frame and class (visualize_activation_maps.py:188-196), spaces replaced as save_images does."""
    names = [f'{stem}_input.png', f'{stem}_{class_name}_{cam_method}.png', f'{stem}_{class_name}_{cam_method}_mask.png',
             f'{stem}_{class_name}_pred.png', f'{stem}_{class_name}_gt.png']
    return [n.replace(' ', '_') for n in names]


def metrics_row(img_path, class_idx, cam_method, architecture, counts, root=None):
    row = {'Image path': os.path.relpath(img_path, root or os.getcwd()), 'Image name': os.path.basename(img_path),
           'Class': class_name_of(class_idx), 'Class ID': class_idx, 'CAM': cam_method, 'Model': architecture}
    row.update(metrics_from_counts(*counts))
    return row


def _layer_path(layer):
    return getattr(layer, '_prefix', None) or getattr(layer, 'name', None)


def _need_cuda(name, t, dtype, dims):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.dim() == dims):
        got = f'{tuple(t.shape)} {t.dtype} {t.device}' if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f'{name} must be a {dtype} CUDA tensor with {dims} dimensions, got {got}')
    return t.contiguous()


def cam_maps(A, G, S, method, threshold=None, gt=None, frames=None, image_weight=0.5, want_bin=False):
    """The map kernels on A, G [N,h,w,K] (float32 or bfloat16 CUDA) for one of the six methods (by name).  Returns a dict: 'maps' float32 [N,S,S]; with ``want_bin`` 'bin'
    uint8 [N,S,S]; with ``gt`` (uint8 CUDA [N,gh,gw]) 'counts' int32 [N,3] = tp, pred, true; with ``frames`` 'overlay' uint8 [N,S,S,3] BGR."""
    method_id = CAM_METHODS.get(method)
    if method_id is None:
        raise ValueError(f'Invalid CAM method: {method}')
    for name, t in (('A', A), ('G', G)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 4 and t.dtype in (torch.float32, torch.bfloat16)):
            raise ValueError(f'{name} must be a float32 / bfloat16 CUDA tensor [N,h,w,K]')
    if A.shape != G.shape or A.dtype != G.dtype:
        raise ValueError(f'A and G differ: {tuple(A.shape)} {A.dtype} vs {tuple(G.shape)} {G.dtype}')
    A, G = A.contiguous(), G.contiguous()
    N, h, w, K = A.shape
    dev = A.device
    lib = L.lib()
    scratch = torch.empty(max(lib.octseg_cam_scratch_bytes(N, h, w, K), 16), dtype=torch.uint8, device=dev)
    out = {'maps': torch.empty((N, S, S), dtype=torch.float32, device=dev)}
    thr = 0.0 if threshold is None else float(threshold)
    if (want_bin or gt is not None) and threshold is None:
        raise ValueError('the thresholded map and the counts need a threshold')
    if want_bin:
        out['bin'] = torch.empty((N, S, S), dtype=torch.uint8, device=dev)
    rows = cols = None
    gh = gw = 0
    if gt is not None:
        gt = _need_cuda('gt', gt, torch.uint8, 3)
        if gt.shape[0] != N:
            raise ValueError(f'gt must hold {N} planes, got {tuple(gt.shape)}')
        from .predict import cv2_nearest_index
        gh, gw = int(gt.shape[1]), int(gt.shape[2])
        rows = torch.from_numpy(cv2_nearest_index(S, gh)).to(dev)
        cols = torch.from_numpy(cv2_nearest_index(S, gw)).to(dev)
        out['counts'] = torch.empty((N, 3), dtype=torch.int32, device=dev)
    jet = None
    if frames is not None:
        frames = _need_cuda('frames', frames, torch.float32, 4)
        if tuple(frames.shape) != (N, 3, S, S):
            raise ValueError(f'frames must be {(N, 3, S, S)}, got {tuple(frames.shape)}')
        jet = torch.from_numpy(jet_table_bgr()).to(dev)
        out['overlay'] = torch.empty((N, S, S, 3), dtype=torch.uint8, device=dev)
    L.check(lib.octseg_cam_maps(L.F32 if A.dtype == torch.float32 else L.BF16, L.ptr(A), L.ptr(G), N, h, w, K, method_id, int(S),
                                L.ptr(scratch), L.ptr(out['maps']), thr, L.ptr(out.get('bin')), L.ptr(gt), gh, gw, L.ptr(rows), L.ptr(cols),
                                L.ptr(out.get('counts')), L.ptr(frames), L.ptr(jet), float(image_weight), L.ptr(out.get('overlay')),
                                L.stream_ptr()))
    return out


class SemanticSegmentationTarget:
    """cam_processor.py:116-140: L = sum(logits[category] * mask).  Held as data: the engine seeds its backward with dL/dlogits = mask."""

    def __init__(self, category, mask):
        self.category = int(category)
        self.mask = mask

    def __call__(self, model_output):
        return (model_output[self.category, :, :] * torch.as_tensor(self.mask).to(model_output.device)).sum()


class CAMProcessor:
    """cam_processor.py:19-113 on the engine.  ``model``: an ``OCTSegmentationModel`` (its forward normalises, as the reference's CAM forward
    does) or a bare ``SegNet``."""

    CAM_METHODS = CAM_METHODS

    def __init__(self, model, device='cuda', cam_method='GradCAM', target_layers=None):
        if cam_method not in CAM_METHODS:
            raise ValueError(f'Invalid CAM method: {cam_method}')
        if CAM_METHODS[cam_method] is None:
            raise NotImplementedError(f'{cam_method}: {_REFUSED[cam_method]}')
        self.model, self.device, self.cam_method, self.method_id = model, device, cam_method, CAM_METHODS[cam_method]
        self.net = getattr(model, 'model', model)
        why = unsupported_reason(self.net.arch, self.net.encoder_name, self.net.dtype_code)
        if why:
            raise NotImplementedError(why)
        want = _layer_path(self.net.encoder.layer4[-1])
        got = [_layer_path(t) for t in (target_layers or [])]
        if got != [want]:
            raise NotImplementedError(f'target_layers must be [model.model.encoder.layer4[-1]] ({want}), got {got}: the engine keeps the '
                                      f'activation and gradient of that block output only')
        self.target_layers = target_layers

    @staticmethod
    def get_targets(class_idx, class_mask):
        return [SemanticSegmentationTarget(class_idx, class_mask)]

    # ------------------------------------------------------------------ device-side batch calls
    def activations(self, frames, class_idx, masks):
        """Frozen forward + seeded backward of N frames.  frames: float32 CUDA [N,3,S,S] BGR 0..255; class_idx: N ints; masks: float32 CUDA
        [N,S,S] (the predicted mask of that class).  Returns (logits, A, G): A, G = views [N,h,w,K] (plan dtype) into the CAM plan's
        workspace, valid until its next call."""
        x = _need_cuda('frames', frames, torch.float32, 4)
        m = _need_cuda('masks', masks, torch.float32, 3)
        N, _, H, W = x.shape
        idx = [int(c) for c in class_idx]
        if len(idx) != N or tuple(m.shape) != (N, H, W) or min(idx) < 0 or max(idx) >= self.net.classes:
            raise ValueError(f'need {N} class indices below {self.net.classes} and masks {(N, H, W)}, got {idx} and {tuple(m.shape)}')
        seed = torch.zeros((N, self.net.classes, H, W), dtype=torch.float32, device=x.device)
        seed[torch.arange(N, device=x.device), torch.tensor(idx, device=x.device)] = m
        normalize = hasattr(self.model, '_mean')
        return self.net.cam_forward_backward(x, seed, normalize, getattr(self.model, '_mean', None), getattr(self.model, '_std', None))

    def maps_from(self, A, G, S, **kw):
        """``cam_maps`` with this processor's method."""
        return cam_maps(A, G, S, self.cam_method, **kw)

    def batch(self, frames, class_idx, masks, **kw):
        """activations + maps_from for N (frame, class) pairs; keywords as ``maps_from`` (``frames=True``: overlay on the input frames)."""
        _, A, G = self.activations(frames, class_idx, masks)
        if kw.get('frames') is True:
            kw['frames'] = frames
        return self.maps_from(A, G, int(frames.shape[-1]), **kw)

    # ------------------------------------------------------------------ the reference's per-frame interface
    def extract_activation_map(self, image, targets, eigen_smooth=False, aug_smooth=False):
        """image: HWC BGR 0..255 (numpy); targets: ``get_targets(...)``.  Returns the float32 [S, S] map in [0, 1]."""
        _refuse_smoothing(eigen_smooth, aug_smooth)
        if torch.is_tensor(image):
            raise ValueError('extract_activation_map takes the HWC numpy frame of the reference; device tensors go through batch()')
        if len(targets) != 1:
            raise NotImplementedError('one SemanticSegmentationTarget per call, as the reference passes')
        dev = self.net.device
        x = torch.as_tensor(np.ascontiguousarray(np.asarray(image).transpose(2, 0, 1)), dtype=torch.float32)[None].to(dev)
        m = torch.as_tensor(np.asarray(targets[0].mask), dtype=torch.float32)[None].to(dev)
        return self.batch(x, [targets[0].category], m)['maps'][0].cpu().numpy()

    def overlay_activation_map(self, image, mask, image_weight=0.5):
        """show_cam_on_image((image / 255).astype(float32), mask, use_rgb=False, image_weight) -> uint8 HWC BGR, on the GPU."""
        if torch.is_tensor(image) or torch.is_tensor(mask):
            raise ValueError('overlay_activation_map takes numpy arrays; device tensors go through maps_from(frames=...)')
        dev = self.net.device
        x = torch.as_tensor(np.ascontiguousarray(np.asarray(image).transpose(2, 0, 1)), dtype=torch.float32)[None].to(dev)
        m = torch.as_tensor(np.asarray(mask), dtype=torch.float32).to(dev)
        return overlay_on_device(x, m[None], image_weight)[0].cpu().numpy()


def overlay_on_device(frames, maps, image_weight=0.5):
    """show_cam_on_image of maps that exist already: frames float32 CUDA [N,3,S,S] BGR 0..255, maps float32 CUDA [N,S,S] -> uint8 [N,S,S,3] BGR."""
    frames = _need_cuda('frames', frames, torch.float32, 4)
    maps = _need_cuda('maps', maps, torch.float32, 3)
    N, S = int(maps.shape[0]), int(maps.shape[1])
    if tuple(maps.shape) != (N, S, S) or tuple(frames.shape) != (N, 3, S, S):
        raise ValueError(f'need square maps [N,S,S] and frames [N,3,S,S], got {tuple(maps.shape)} and {tuple(frames.shape)}')
    jet = torch.from_numpy(jet_table_bgr()).to(maps.device)
    scratch = torch.empty(16 * N, dtype=torch.uint8, device=maps.device)
    out = torch.empty((N, S, S, 3), dtype=torch.uint8, device=maps.device)
    L.check(L.lib().octseg_cam_overlay(L.ptr(maps), L.ptr(frames), L.ptr(jet), N, S, float(image_weight), L.ptr(out), L.ptr(scratch), L.stream_ptr()))
    return out


def _refuse_smoothing(eigen_smooth, aug_smooth):
    if eigen_smooth:
        raise NotImplementedError("eigen_smooth projects the map on its first singular vector, whose sign is LAPACK's choice and cannot be pinned")
    if aug_smooth:
        raise NotImplementedError('aug_smooth averages the maps of flipped and rescaled copies of the input (package-specific transforms): not built')


# ---------------------------------------------------------------------- the tool
def _resize_for_save(image, output_size, num_colors_threshold=10):
    """save_images (visualize_activation_maps.py:48-72): nearest for images of at most 10 distinct colours, else -- LANCZOS4 in the reference
    -- the cv2-exact 8-bit bilinear of predict.cv2_resize_linear_u8 (a listed deviation)."""
    from .predict import cv2_nearest_index, cv2_resize_linear_u8
    if not output_size:
        return image
    ow, oh = int(output_size[0]), int(output_size[1])     # cv2 dsize = (width, height)
    few = image.ndim == 2 or len(np.unique(image.reshape(-1, 3), axis=0)) <= num_colors_threshold
    if few:
        return image[cv2_nearest_index(image.shape[0], oh)][:, cv2_nearest_index(image.shape[1], ow)]
    return cv2_resize_linear_u8(np.ascontiguousarray(image), ow, oh)


def _write_png(path, image_bgr):
    from PIL import Image
    Image.fromarray(image_bgr if image_bgr.ndim == 2 else np.ascontiguousarray(image_bgr[:, :, ::-1])).save(path)   # cv2.imwrite takes BGR


def _colorize(plane, class_name, shape):
    """colorize_mask(mask, [class_name]) then cvtColor(BGR2RGB): the class colour (as BGR for imwrite) where the plane is exactly 255."""
    from .postprocess import CLASS_COLORS_RGB
    out = np.full((shape[0], shape[1], 3), 128, np.uint8)
    out[plane == 255] = CLASS_COLORS_RGB[class_name][::-1]
    return out


def main(argv=None):
    """visualize_activation_maps.py:80-207 from ``configs/visualize_activation_maps.yaml`` (``key=value`` overrides).  Extra keys:
    ``compute_dtype`` (fp32 | bf16, default fp32) and ``batch_size`` (frames per forward; every frame runs once per class)."""
    import logging
    import sys
    from glob import glob
    from . import ingest
    from .config import load_config
    from .dataset import read_image_bgr, read_mask_tiff
    from .predict import cv2_nearest_index, load_model
    log = logging.getLogger('oct_segmentation_amd.cam')
    if not logging.getLogger().handlers:
        logging.basicConfig(level=logging.INFO)
    cfg = load_config('visualize_activation_maps', list(sys.argv[1:] if argv is None else argv))
    device = 'cuda' if cfg.get('device', 'auto') in ('auto', 'gpu', 'cuda') else cfg['device']
    if not (str(device).startswith('cuda') and torch.cuda.is_available()):
        raise RuntimeError(f'the activation-map tool needs a GPU (device={cfg.get("device")!r}): there is no CPU path')
    dtype = {'bf16': torch.bfloat16, 'fp32': torch.float32}[str(cfg.get('compute_dtype', 'fp32'))]
    model, mcfg = load_model(str(cfg['model_dir']), device, dtype)
    method, arch = str(cfg['cam_method']), mcfg['architecture']
    proc = CAMProcessor(model=model, device=device, cam_method=method, target_layers=[model.model.encoder.layer4[-1]])
    _refuse_smoothing(cfg.get('eigen_smooth'), cfg.get('aug_smooth'))
    S, C_ = int(mcfg['input_size']), len(mcfg['classes'])
    img_paths = sorted(glob(os.path.join(str(cfg['data_dir']), 'img', '*.png')))
    if not img_paths:
        raise FileNotFoundError(f'no *.png under {cfg["data_dir"]}/img')
    out_dir = os.path.join(str(cfg['save_dir']), arch)
    os.makedirs(out_dir, exist_ok=True)
    thr, out_size, bs = float(cfg['map_threshold']), cfg.get('output_size'), max(1, int(cfg.get('batch_size', 4)))
    rows = []
    lib = L.lib()
    for i0 in range(0, len(img_paths), bs):
        paths = img_paths[i0:i0 + bs]
        n = len(paths)
        x = torch.empty((n, 3, S, S), dtype=torch.float32, device=device)
        for k, p in enumerate(paths):     # cv2.imread + cv2.resize(img, input_size) on the device (frames may differ in size)
            ingest.resize_image_u8(torch.from_numpy(read_image_bgr(p))[None].to(device), S, out=x[k:k + 1])
        z = model.predict_logits(x)       # model.predict: un-normalised, sigmoid > 0.5 (the engine's serving epilogue)
        pred = torch.empty((n, S, S, C_), dtype=torch.float32, device=device)
        for ch in range(C_):
            L.check(lib.octseg_mask_assemble(L.ptr(z), n, C_, S, S, ch, L.ptr(pred), S, S, C_, ch, None, None, L.stream_ptr()))
        xs = x.repeat_interleave(C_, dim=0)                                   # frame-major: (frame 0, class 0), (frame 0, class 1), ...
        ms = pred.permute(0, 3, 1, 2).reshape(n * C_, S, S).contiguous()
        _, A, G = proc.activations(xs, list(range(C_)) * n, ms)
        pred_u8 = (pred * 255).to(torch.uint8).cpu().numpy()
        frames_u8 = x.permute(0, 2, 3, 1).to(torch.uint8).cpu().numpy()
        for k, p in enumerate(paths):
            stem = os.path.splitext(os.path.basename(p))[0]
            gt = read_mask_tiff(os.path.join(str(cfg['data_dir']), 'mask', f'{stem}.tiff'))
            gt_planes = torch.from_numpy(np.ascontiguousarray(gt[:, :, :C_].transpose(2, 0, 1))).to(device)   # TIFF channel = class index (:172)
            sl = slice(k * C_, (k + 1) * C_)
            o = proc.maps_from(A[sl], G[sl], S, threshold=thr, gt=gt_planes, frames=xs[sl], image_weight=0.5, want_bin=True)
            counts, bins, ovs = o['counts'].cpu().numpy(), o['bin'].cpu().numpy(), o['overlay'].cpu().numpy()
            ri, ci = cv2_nearest_index(S, gt.shape[0]), cv2_nearest_index(S, gt.shape[1])
            for c in range(C_):
                cname = class_name_of(c)
                rows.append(metrics_row(p, c, method, arch, counts[c]))
                images = [frames_u8[k], ovs[c], bins[c][ri][:, ci], _colorize(pred_u8[k][:, :, c], cname, (S, S)),
                          _colorize(gt[:, :, c], cname, gt.shape[:2])]
                for image, name in zip(images, output_names(stem, cname, method)):
                    _write_png(os.path.join(out_dir, name), _resize_for_save(image, out_size))
    csv_path = os.path.join(str(cfg['save_dir']), f'{arch}_{method}_metrics.csv')
    with open(csv_path, 'w', newline='') as f:
        w = csv.DictWriter(f, fieldnames=CSV_COLUMNS)
        w.writeheader()
        w.writerows(rows)
    log.info(f'{len(rows)} maps, metrics in {csv_path}')
    log.info('Complete!')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
