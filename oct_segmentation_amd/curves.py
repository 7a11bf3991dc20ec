"""Operating curves from one streaming pass: per frame and class the 256-bin histogram of the predicted probability over the truth-negative and
over the truth-positive pixels (``csrc/curves.hip``, ``octseg_logit_histogram``; no reference counterpart).

Every mask of the engine is ``sigmoid(z) > 0.5``, and the reference scores per-class DSC at that one threshold.  From the integer histograms
tp / fp / fn / tn at EVERY threshold ``k / 256`` are suffix sums on the host: the ROC and precision-recall curves, the reliability diagram and the
DSC-optimal threshold come from a 2 KB table per frame and class, and no logits tensor goes to the host.

    hist = logit_histograms(logits, target)                 # int32 CUDA [N, C, 2, 256], label-major: [.., 0, :] truth-negative, [.., 1, :] truth-positive
    cur = operating_curves(hist)                            # pooled over the frames: counts, DSC / IoU / precision / recall at k = 0..256, AUC, AP, ECE
    best = best_thresholds(hist)                            # per class the k in 1..255 of the largest pooled DSC, and DSC there and at 128
    apply_thresholds(logits, [0], [best['threshold'][0]])   # in place: afterwards every `> 0.5` epilogue of the engine cuts at that threshold

Bin rule (include/octseg.h): ``p`` = the engine's f32 sigmoid, ``bin = clamp(ceil(p * 256) - 1, 0, 255)``; a pixel is set at threshold ``k / 256`` iff
``bin >= k``, exactly ``p > k / 256`` in f32, and ``k = 128`` is the engine's own mask pixel for pixel.

    python -m oct_segmentation_amd.curves model_dir=models/LM data_dir=data/fold_1/test [batch_size=8] [compute_dtype=bf16] [save_dir=<model_dir>]

writes ``curves.json`` (``curve_report``) and ``curves.png``; ``predict ... thresholds=curves.json`` serves with the thresholds it found.
"""
import json
import math
import os

import numpy as np

BINS = 256
HALF = BINS // 2
METRICS = ('dice', 'iou', 'precision', 'recall')


def logit_histograms(logits, target, out=None):
    """The thin door to ``octseg_logit_histogram``: ``logits`` and ``target`` contiguous float32 NCHW CUDA tensors of one shape on one device (a
    target pixel is positive iff ``!= 0``); returns int32 CUDA ``[N, C, 2, 256]`` (``out`` if given: the call clears it).  Enqueue only."""
    import torch
    from . import _lib as L
    for t, name in ((logits, 'logits'), (target, 'target')):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
            raise ValueError(f'{name} must be a contiguous float32 NCHW CUDA tensor')
    if tuple(logits.shape) != tuple(target.shape) or logits.device != target.device:
        raise ValueError(f'logits {tuple(logits.shape)} on {logits.device} and target {tuple(target.shape)} on {target.device} differ in shape or device')
    if 0 in logits.shape:
        raise ValueError(f'logits {tuple(logits.shape)} are empty')
    N, C, H, W = (int(v) for v in logits.shape)
    if out is None:
        out = torch.empty((N, C, 2, BINS), dtype=torch.int32, device=logits.device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (N, C, 2, BINS)
              and out.device == logits.device):
        raise ValueError(f'out must be a contiguous int32 CUDA tensor {(N, C, 2, BINS)} on the device of logits')
    with torch.cuda.device(logits.device):
        L.check(L.lib().octseg_logit_histogram(L.ptr(logits), L.ptr(target), N, C, H, W, L.ptr(out), L.stream_ptr()))
    return out


def _host(hist):
    """``hist`` (torch or numpy, host or device) as int64 numpy ``[..., C, 2, 256]``; one copy to the host."""
    if hasattr(hist, 'detach'):
        hist = hist.detach().cpu().numpy()
    h = np.asarray(hist)
    if h.ndim not in (3, 4) or h.shape[-2:] != (2, BINS) or h.dtype.kind not in 'iu':
        raise ValueError(f'hist must be an integer array [N, C, 2, {BINS}] or [C, 2, {BINS}], got {h.dtype} {h.shape}')
    return h.astype(np.int64)


def _pooled(hist):
    h = _host(hist)
    return h.sum(axis=0) if h.ndim == 4 else h


def _suffix(a):
    """[..., 256] -> [..., 257]: the sum over bins >= k for k = 0..256."""
    s = np.cumsum(a[..., ::-1], axis=-1)[..., ::-1]
    return np.concatenate([s, np.zeros(a.shape[:-1] + (1,), dtype=np.int64)], axis=-1)


def _curves(h):
    """The curves of int64 histograms ``[..., 2, 256]``, one set per leading index."""
    from .metrics import _metrics_from_numpy
    neg, pos = h[..., 0, :], h[..., 1, :]
    tp, fp = _suffix(pos), _suffix(neg)
    P, Nn = tp[..., :1], fp[..., :1]
    fn, tn = P - tp, Nn - fp
    m = _metrics_from_numpy(np.stack([tp, fp, fn, tn], axis=-1), np.float32(0))      # the float32 ratios of the epoch CSV, 0 / 0 -> 1e-7
    out = {'tp': tp, 'fp': fp, 'fn': fn, 'tn': tn}
    for k in METRICS:
        out[k] = m[k].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        tpr, fpr = tp / P.astype(np.float64), fp / Nn.astype(np.float64)            # nan for a class without positives / negatives
        out['tpr'], out['fpr'] = tpr, fpr
        out['auc'] = ((fpr[..., :-1] - fpr[..., 1:]) * (tpr[..., :-1] + tpr[..., 1:]) * 0.5).sum(axis=-1)
        prec = np.where(tp + fp > 0, tp / np.maximum(tp + fp, 1).astype(np.float64), 0.0)      # (a threshold that sets nothing adds no recall)
        out['ap'] = ((tpr[..., :-1] - tpr[..., 1:]) * prec[..., :-1]).sum(axis=-1)
        count = neg + pos
        frac = pos / count.astype(np.float64)
        mid = (np.arange(BINS) + 0.5) / BINS
        total = count.sum(axis=-1, keepdims=True).astype(np.float64)
        out['ece'] = (np.where(count > 0, np.abs(frac - mid), 0.0) * count / total).sum(axis=-1)
    out['bin_count'], out['bin_positive'], out['bin_mid'] = count, frac, mid
    out['thresholds'] = np.arange(BINS + 1) / BINS
    return out


def operating_curves(hist):
    """Host curves per class of ``hist`` ``[N, C, 2, 256]`` (summed over the frames first) or ``[C, 2, 256]`` (summed already), host or device.
    int64 ``[C, 257]``: ``tp``, ``fp``, ``fn``, ``tn`` at the thresholds ``k / 256``, ``k = 0..256`` -- a pixel is set iff its bin is ``>= k``, so
    ``k = 0`` sets everything and ``k = 256`` nothing.  float64 ``[C, 257]``: ``dice``, ``iou``, ``precision``, ``recall`` by the ratio rule of
    ``metrics.py`` (float32 ratios, ``0 / 0 -> 1e-7``, ``dice = 2 iou / (iou + 1)``), so that ``k = 128`` reproduces the epoch CSV's numbers on the
    same counts; ``tpr``, ``fpr``.  float64 ``[C]``: ``auc`` (ROC, trapezoid rule over the 257 points), ``ap`` (average precision,
    ``sum_k (R_k - R_{k+1}) P_k``), both ``nan`` for a class without positive (``auc``: or without negative) pixels; ``ece``.  The reliability
    table: ``bin_count`` int64 ``[C, 256]``, ``bin_positive`` (the positive fraction, ``nan`` in an empty bin), ``bin_mid`` ``[256]``.
    ``ece = sum_j count_j / total * |bin_positive_j - bin_mid_j|`` uses the bin MIDPOINT ``(j + 0.5) / 256`` as the bin's confidence, not the
    mean probability of its pixels, which the histogram does not hold: off by at most 1 / 512."""
    return _curves(_pooled(hist))


def _pick(values):
    """argmax over k = 1..255 of ``values`` [257]; ties to the k nearest 128, then to the smaller k."""
    v = values[1:BINS]
    ks = np.flatnonzero(v == v.max()) + 1
    return int(min(ks, key=lambda k: (abs(int(k) - HALF), int(k))))


def best_thresholds(hist, metric='dice'):
    """Per class the threshold ``k / 256``, ``k`` in 1..255, at which ``metric`` (``dice`` | ``iou`` | ``precision`` | ``recall``) of the POOLED counts
    is largest; ties go to the ``k`` nearest 128, then to the smaller ``k``.  Returns ``{'k': int64 [C], 'threshold': float64 [C], 'best': the metric
    there, 'at_half': the metric at k = 128}``."""
    if metric not in METRICS:
        raise ValueError(f'metric must be one of {METRICS}, got {metric!r}')
    values = operating_curves(hist)[metric]
    ks = np.array([_pick(v) for v in values], dtype=np.int64)
    rows = np.arange(len(ks))
    return {'k': ks, 'threshold': ks / BINS, 'best': values[rows, ks], 'at_half': values[rows, HALF]}


def _json(a):
    """A numpy array as nested lists with ``nan`` as ``None``."""
    a = np.asarray(a)
    if a.dtype.kind == 'f':
        return [None if isinstance(v, float) and math.isnan(v) else v for v in a.tolist()] if a.ndim == 1 else [_json(r) for r in a]
    return a.tolist()


def _num(v):
    v = float(v)
    return None if math.isnan(v) else v


def curve_report(hist, names, classes):
    """The JSON-able dict the tool writes as ``curves.json``, from per-frame histograms ``[N, C, 2, 256]``, the frames' ``names`` and the class
    names: per class the pooled curves, the DSC-optimal threshold, DSC at 0.5 against DSC there, AUC, AP, ECE, the reliability table, and per
    frame DSC at both thresholds.  ``nan`` is written as ``null``."""
    h = _host(hist)
    if h.ndim != 4:
        raise ValueError(f'curve_report takes per-frame histograms [N, C, 2, {BINS}], got {h.shape}')
    if h.shape[0] != len(names):
        raise ValueError(f'{len(names)} names for {h.shape[0]} frames')
    if h.shape[1] != len(classes):
        raise ValueError(f'{len(classes)} class names for {h.shape[1]} classes')
    pooled, frames = _curves(h.sum(axis=0)), _curves(h)
    best = best_thresholds(h.sum(axis=0))
    report = {'bins': BINS, 'frames': int(h.shape[0]), 'thresholds': pooled['thresholds'].tolist(), 'classes': {}}
    for c, cls in enumerate(classes):
        k = int(best['k'][c])
        report['classes'][cls] = {
            'pixels': int(h[:, c].sum()), 'positive_pixels': int(h[:, c, 1].sum()),
            'best_k': k, 'best_threshold': k / BINS,
            'dice_at_half': float(best['at_half'][c]), 'dice_at_best': float(best['best'][c]),
            'auc': _num(pooled['auc'][c]), 'ap': _num(pooled['ap'][c]), 'ece': _num(pooled['ece'][c]),
            'curves': {key: _json(pooled[key][c]) for key in ('tp', 'fp', 'fn', 'tn') + METRICS + ('tpr', 'fpr')},
            'reliability': {'count': _json(pooled['bin_count'][c]), 'positive_fraction': _json(pooled['bin_positive'][c]),
                            'midpoint': _json(pooled['bin_mid'])},
            'slices': {name: {'dice_at_half': float(frames['dice'][i, c, HALF]), 'dice_at_best': float(frames['dice'][i, c, k])}
                       for i, name in enumerate(names)},
        }
    return report


def threshold_shift(t):
    """``float32(log(t / (1 - t)))``, the logit of the threshold ``t`` in (0, 1): what ``apply_thresholds`` subtracts."""
    t = float(t)
    if not 0.0 < t < 1.0:
        raise ValueError(f'a threshold must lie in (0, 1), got {t}')
    return np.float32(math.log(t / (1.0 - t)))


def apply_thresholds(logits, channels, thresholds):
    """In place ``logits[:, ch] -= float32(log(t / (1 - t)))`` for every pair of ``channels`` and ``thresholds`` (``t`` in (0, 1)): afterwards
    ``sigmoid(z) > 0.5`` holds where ``sigmoid`` of the original logit exceeded ``t``, so every existing ``> 0.5`` epilogue of the engine
    (``octseg_mask_assemble``, ``octseg_vote_assemble``) cuts at ``t`` without a threshold argument of its own.  The shift and the subtraction are
    rounded to float32: a pixel whose probability lies within rounding of ``t`` may fall on either side.  ``t = 0.5`` changes nothing.
    ``logits``: a float32 tensor ``[N, C, H, W]``.  Returns ``logits``."""
    import torch
    channels, thresholds = [int(c) for c in channels], list(thresholds)
    if len(channels) != len(thresholds):
        raise ValueError('channels and thresholds must have one entry per channel')
    if not (torch.is_tensor(logits) and logits.dtype == torch.float32 and logits.dim() == 4):
        raise ValueError('logits must be a float32 tensor [N, C, H, W]')
    shifts = [threshold_shift(t) for t in thresholds]
    for c in channels:
        if not 0 <= c < logits.shape[1]:
            raise ValueError(f'channel {c} outside [0, {logits.shape[1]})')
    if len(set(channels)) != len(channels):
        raise ValueError(f'a channel is listed twice: {channels}')
    for c, s in zip(channels, shifts):
        if s != 0:
            logits[:, c].sub_(float(s))
    return logits


def read_thresholds(spec):
    """``predict``'s ``thresholds`` key as ``{class name: t}``: a dict, or the path of a ``curves.json`` (its ``best_threshold`` per class).  Class
    names that the engine does not know and ``t`` outside (0, 1) are refused here, before anything is loaded."""
    from .model import CLASS_IDS
    if spec is None:
        return None
    if isinstance(spec, str):
        with open(spec) as f:
            spec = {name: entry['best_threshold'] for name, entry in json.load(f)['classes'].items()}
    if not isinstance(spec, dict) or not spec:
        raise ValueError(f'thresholds must be a curves.json path or a non-empty dict of class name -> threshold, got {spec!r}')
    out = {}
    for name, t in spec.items():
        if name not in CLASS_IDS:
            raise ValueError(f'thresholds: unknown class {name!r}, not one of {sorted(CLASS_IDS)}')
        if isinstance(t, bool) or not isinstance(t, (int, float)):
            raise ValueError(f'thresholds: {name!r} needs a number in (0, 1), got {t!r}')
        threshold_shift(t)
        out[name] = float(t)
    return out


def save_plot(report, path):
    """``curves.png``: DSC against the threshold, ROC, precision-recall and the reliability diagram, one line per class (matplotlib, Agg)."""
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    nan = lambda v: np.array([np.nan if x is None else x for x in v], dtype=np.float64)      # noqa: E731
    fig, axes = plt.subplots(2, 2, figsize=(10, 9))
    th = np.asarray(report['thresholds'])
    for cls, entry in report['classes'].items():
        cur = entry['curves']
        axes[0, 0].plot(th[1:BINS], nan(cur['dice'])[1:BINS], label=f"{cls} (best {entry['best_threshold']:.3f})")
        axes[0, 1].plot(nan(cur['fpr']), nan(cur['tpr']), label=cls if entry['auc'] is None else f"{cls} (AUC {entry['auc']:.4f})")
        axes[1, 0].plot(nan(cur['tpr'])[:BINS], nan(cur['precision'])[:BINS], label=cls if entry['ap'] is None else f"{cls} (AP {entry['ap']:.4f})")
        rel = entry['reliability']
        axes[1, 1].plot(nan(rel['midpoint']), nan(rel['positive_fraction']), label=cls if entry['ece'] is None else f"{cls} (ECE {entry['ece']:.4f})")
    axes[0, 0].axvline(0.5, color='grey', linewidth=0.8)
    axes[0, 1].plot([0, 1], [0, 1], color='grey', linewidth=0.8)
    axes[1, 1].plot([0, 1], [0, 1], color='grey', linewidth=0.8)
    for ax, (title, xl, yl) in zip(axes.ravel(), (('DSC against the threshold', 'threshold', 'DSC'), ('ROC', 'false positive rate', 'true positive rate'),
                                                  ('Precision-recall', 'recall', 'precision'),
                                                  ('Reliability', 'predicted probability (bin midpoint)', 'positive fraction'))):
        ax.set_title(title); ax.set_xlabel(xl); ax.set_ylabel(yl); ax.set_xlim(0, 1); ax.set_ylim(0, 1.02); ax.legend(fontsize=8)
    fig.tight_layout()
    fig.savefig(path, dpi=100)
    plt.close(fig)


KEYS = {'model_dir': None, 'data_dir': None, 'batch_size': 8, 'compute_dtype': 'bf16', 'save_dir': None, 'device': 'auto'}


def _config(argv):
    from .config import _coerce
    cfg = dict(KEYS)
    for ov in argv:
        k, eq, v = ov.partition('=')
        if not eq or k not in KEYS:
            raise ValueError(f'curves takes key=value arguments with the keys {sorted(KEYS)}, got {ov!r}')
        cfg[k] = _coerce(v)
    for k in ('model_dir', 'data_dir'):
        if cfg[k] is None:
            raise ValueError(f'curves needs {k}=<directory>')
    if str(cfg['compute_dtype']) not in ('bf16', 'fp16', 'fp32'):
        raise ValueError(f"compute_dtype must be bf16, fp16 or fp32, got {cfg['compute_dtype']!r}")
    if not (isinstance(cfg['batch_size'], int) and cfg['batch_size'] > 0):
        raise ValueError(f"batch_size must be a positive integer, got {cfg['batch_size']!r}")
    return cfg


def fold_histograms(model, dataset, batch_size=8, device='cuda'):
    """Per-frame histograms of ``model`` (eval mode, the forward of ``validation_step``: the encoder's normalisation fused in) over ``dataset``
    through the ``DeviceBatches`` ingest: one histogram launch per batch, only the ``[n, C, 2, 256]`` tables are kept.  Returns ``(hist, order)``:
    ``order[i]`` is the dataset index of row ``i`` (``DeviceBatches`` puts the frames of one source size of a batch together)."""
    import torch
    from .dataset import DeviceBatches, group_by_shape
    model.eval()
    batches = DeviceBatches(dataset, batch_size, shuffle=False, device=device)
    parts, order = [], []
    for idx in batches.batch_indices(0):
        samples = [dataset[int(i)] for i in idx]
        order += [int(idx[p]) for _, ps in group_by_shape([(s[0].shape, s[1].shape) for s in samples]) for p in ps]
        img, mask = batches.upload(samples)
        with torch.no_grad():
            logits = model(img)
        parts.append(logit_histograms(logits.contiguous(), mask.contiguous()))
    return torch.cat(parts, dim=0), order


def main(argv=None):
    """``python -m oct_segmentation_amd.curves model_dir=<dir> data_dir=<fold>/test [batch_size=8] [compute_dtype=bf16] [save_dir=<model_dir>]``:
    the checkpoint of ``model_dir`` (``predict.load_model``) over the ``img`` / ``mask`` pairs of ``data_dir``; writes ``curves.json``
    (``curve_report``, frames named by their file stems) and ``curves.png`` into ``save_dir``."""
    import logging
    import sys
    import torch
    from .dataset import OCTDataset
    from .predict import load_model
    log = logging.getLogger('oct_segmentation_amd.curves')
    if not logging.getLogger().handlers:
        logging.basicConfig(level=logging.INFO, format='[%(asctime)s][%(name)s][%(levelname)s] - %(message)s')
    cfg = _config(list(sys.argv[1:] if argv is None else argv))
    device = 'cuda' if cfg['device'] in ('auto', 'gpu', 'cuda') else cfg['device']
    if not (str(device).startswith('cuda') and torch.cuda.is_available()):
        raise RuntimeError(f'curves needs a GPU (device={cfg["device"]!r}): there is no CPU path')
    dtypes = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
    model, mcfg = load_model(str(cfg['model_dir']), device, dtypes[str(cfg['compute_dtype'])])
    dataset = OCTDataset(str(cfg['data_dir']), mcfg['classes'], mcfg['input_size'])
    log.info(f'Number of frames: {len(dataset)}')
    hist, order = fold_histograms(model, dataset, int(cfg['batch_size']), device)
    names = [os.path.splitext(os.path.basename(dataset.img_paths[i]))[0] for i in order]
    report = curve_report(hist, names, list(mcfg['classes']))
    save_dir = str(cfg['save_dir'] if cfg['save_dir'] is not None else cfg['model_dir'])
    os.makedirs(save_dir, exist_ok=True)
    with open(os.path.join(save_dir, 'curves.json'), 'w') as f:
        json.dump(report, f)
    save_plot(report, os.path.join(save_dir, 'curves.png'))
    for cls, entry in report['classes'].items():
        log.info(f"{cls}: DSC {entry['dice_at_half']:.4f} at 0.5, {entry['dice_at_best']:.4f} at {entry['best_threshold']:.4f}; "
                 f"AUC {entry['auc']}, AP {entry['ap']}, ECE {entry['ece']}")
    log.info('Complete')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
