"""Predicted against annotated lesions on the GPU (``csrc/match.hip``, ``octseg_volume_match``; no reference counterpart):
which annotated lesions were found, which predicted lesions are false alarms, and how well the matched ones agree.

Both stacks are labelled and ranked as ``lesions.lesion_table`` does it (section 5j); one more pass over the two sets of bit planes fills, per
class, the 33 x 33 table of the voxels both stacks set, by the RANK of their lesion on either side: 0..31 for the 32 largest, 32 ("rest") for a
lesion beyond the 32 listed.  Side 0 is the prediction, side 1 the truth.

    m = match_volumes(pred, truth)                # Match(nles [channels, 2], top [channels, 2, 32, 8], overlap [channels, 33, 33], frames [channels, N, 3])
    report = match_report(pred, truth, names)     # per class: pairs, tp / fp / fn, sensitivity, precision, SQ / RQ / PQ, split, merged, frames

``pred`` and ``truth`` are float32 CUDA [N, H, W, channels] of one shape, any value != 0 set; they may be the same tensor.  Everything on the
device is integer: results EQUAL the restatement's (``tests/match_ref.py``), no tolerance.  Nothing synchronises with the host before
``match_report``'s one copy of the tables; scratch comes from torch's allocator, sized by the library.

    python -m oct_segmentation_amd.match pred_dir truth_dir [save_dir] [across=overlap|full] [iou=0.5]

writes ``lesion_match.json`` for the mask TIFFs both folders hold under the same name and prints its path.
"""
import json
import os
import sys
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from . import lesions
from .lesions import ACROSS, TOPL, TOP_COLUMNS

RANKS = TOPL + 1               # 0..31 ranked, 32 = rest
DEFAULT_SCRATCH = 8 << 30      # about 17.3 bytes per voxel and channel: a 186 x 704 x 704 x 4 pullback needs 6.4 GB and goes in one call
CRITERIA = ('iou', 'overlap')

Match = namedtuple('Match', 'nles top overlap frames')


def _check(pred, truth, across):
    pred, n, h, w, sc, ac = lesions._check(pred, across)
    truth = lesions._check(truth, across)[0]
    if pred.shape != truth.shape or pred.device != truth.device:
        raise ValueError(f'pred and truth must agree in shape and device, got {tuple(pred.shape)} and {tuple(truth.shape)}')
    return pred, truth, n, h, w, sc, ac


def _chunks(stack, n, h, w, sc, scratch_bytes):
    """``lesions._chunks`` with this call's scratch: all channels in one call when it fits the budget, else one channel at a time."""
    lib = L.lib()
    for per in (sc, 1):
        need = int(lib.octseg_match_scratch_bytes(per, n, h, w))
        if need <= int(scratch_bytes):
            return per, torch.empty((need,), dtype=torch.uint8, device=stack.device), need
    raise ValueError(f'one channel of a {n} x {h} x {w} volume needs {need} bytes of scratch, scratch_bytes is {int(scratch_bytes)}')


def match_volumes(pred, truth, across='overlap', want_top=True, want_frames=True, scratch_bytes=DEFAULT_SCRATCH):
    """``Match(nles, top, overlap, frames)`` as int32 CUDA tensors: ``nles`` [channels, 2], the lesions per side (0 = pred, 1 = truth); ``top``
    [channels, 2, 32, 8], ``lesions.lesion_table``'s rows for each side (None without ``want_top``); ``overlap`` [channels, 33, 33], the voxels
    whose pred rank is i and truth rank is j (32 = a lesion beyond the 32 listed); ``frames`` [channels, N, 3], ``|P & T|, |P|, |T|`` set
    pixels per slice (None without ``want_frames``).  All channels go in one call when the scratch fits ``scratch_bytes``, one channel at a time
    when not; the result does not depend on the chunking."""
    pred, truth, n, h, w, sc, ac = _check(pred, truth, across)
    dev = pred.device
    nles = torch.empty((sc, 2), dtype=torch.int32, device=dev)
    top = torch.empty((sc, 2, TOPL, len(TOP_COLUMNS)), dtype=torch.int32, device=dev) if want_top else None
    overlap = torch.empty((sc, RANKS, RANKS), dtype=torch.int32, device=dev)
    frames = torch.empty((sc, n, 3), dtype=torch.int32, device=dev) if want_frames else None
    with torch.cuda.device(dev):
        per, scratch, nbytes = _chunks(pred, n, h, w, sc, scratch_bytes)
        for (c, m, p), (_, _, t) in zip(lesions._pieces(pred, sc, per), lesions._pieces(truth, sc, per)):
            L.check(L.lib().octseg_volume_match(L.ptr(p), L.ptr(t), n, h, w, m, ac, L.ptr(scratch), nbytes, L.ptr(nles[c:c + m]),
                                                L.ptr(top[c:c + m]) if want_top else None, L.ptr(overlap[c:c + m]),
                                                L.ptr(frames[c:c + m]) if want_frames else None, L.stream_ptr()))
    return Match(nles, top, overlap, frames)


def _ratio(num, den):
    return float(num) / float(den) if den else None


def build_match(nles, top, overlap, frames, h, w, image_names=None, classes=None, criterion='iou', iou=0.5, min_overlap=1, min_pixels=1):
    """The match report from the integers: ``nles`` [channels, 2], ``top`` [channels, 2, 32, 8], ``overlap`` [channels, 33, 33] and ``frames``
    [channels, N, 3] (numpy or anything ``np.asarray`` takes), the frame size, optionally one name per slice and one per channel (default
    ``lesions.default_classes``).  Pure host; values are plain Python numbers, so the dict goes through ``json.dump``.  Per class:

    ``n_pred``, ``n_truth``; ``truncated`` (either side has more than the 32 lesions listed: the scores cover the ranked lesions only);
    ``unranked_overlap`` {'pred_rest', 'truth_rest'}: the sums of row 32 and of column 32.

    ``pairs``: every ranked (i, j) with overlap > 0: ``pred``, ``truth`` (ranks), ``intersection``, ``iou`` = I / (vp + vt - I), ``dice`` =
    2 I / (vp + vt), ``length_pred``, ``length_truth``, ``start_offset`` = z0 of pred - z0 of truth and ``end_offset`` likewise for z1, in slices.

    ``criterion='iou'``: a pair matches iff IoU > ``iou`` (0.5 <= iou < 1, so a lesion has at most one partner): at 0.5 by the integers,
    2 I > union, otherwise I > iou * union in float64.  ``tp``, ``fp``, ``fn``, ``sensitivity`` = tp / (tp + fn), ``precision`` = tp / (tp + fp),
    ``f1``, ``sq`` (the mean IoU of the matches), ``rq`` = tp / (tp + fp / 2 + fn / 2), ``pq`` = sq * rq, ``matches`` [[i, j], ...].
    ``criterion='overlap'``: a truth lesion is detected if its column (rest row included) sums to at least ``min_overlap``, a predicted lesion is
    a true positive if its row does: ``detected``, ``missed``, ``true_positives``, ``false_positives``, ``sensitivity``, ``precision``.
    A denominator of 0 gives None.

    Under both: ``split`` (truth lesions overlapped by >= 2 ranked predicted lesions), ``merged`` (predicted lesions overlapping >= 2 ranked
    truth lesions), ``voxel_dice`` from the ``frames`` totals, and ``frames``: per-slice presence with ``min_pixels`` as ``tp / fp / fn / tn``
    frames with ``sensitivity`` and ``specificity``, and the per-slice ``dice`` (None where both slices are empty)."""
    nles, top, overlap, frames = np.asarray(nles), np.asarray(top), np.asarray(overlap), np.asarray(frames)
    h, w = int(h), int(w)
    if (nles.ndim != 2 or nles.shape[1] != 2 or top.shape != (nles.shape[0], 2, TOPL, len(TOP_COLUMNS))
            or overlap.shape != (nles.shape[0], RANKS, RANKS) or frames.ndim != 3 or frames.shape[0] != nles.shape[0] or frames.shape[2] != 3):
        raise ValueError(f'nles {nles.shape}, top {top.shape}, overlap {overlap.shape} and frames {frames.shape} must be [channels, 2], '
                         f'[channels, 2, {TOPL}, {len(TOP_COLUMNS)}], [channels, {RANKS}, {RANKS}] and [channels, N, 3]')
    sc, n = int(nles.shape[0]), int(frames.shape[1])
    if h < 1 or w < 1:
        raise ValueError(f'frame size must be positive, got {h} x {w}')
    if criterion not in CRITERIA:
        raise ValueError(f"criterion must be 'iou' or 'overlap', got {criterion!r}")
    iou = float(iou)
    if not 0.5 <= iou < 1.0:
        raise ValueError(f'iou must be in [0.5, 1), got {iou}')
    min_overlap, min_pixels = int(min_overlap), int(min_pixels)
    if min_overlap < 1 or min_pixels < 1:
        raise ValueError('min_overlap and min_pixels must be at least 1')
    if image_names is not None:
        image_names = [str(s) for s in image_names]
        if len(image_names) != n:
            raise ValueError(f'{len(image_names)} names for {n} slices')
    classes = lesions.default_classes(sc) if classes is None else [str(s) for s in classes]
    if len(classes) != sc or len(set(classes)) != len(classes):
        raise ValueError(f'{len(classes)} class names for {sc} channels, or a name twice')
    report = {}
    for c, name in enumerate(classes):
        n_pred, n_truth = int(nles[c, 0]), int(nles[c, 1])
        rp, rt = min(n_pred, TOPL), min(n_truth, TOPL)
        ov = overlap[c].astype(np.int64)
        pairs, matches, ious = [], [], []
        for i in range(rp):
            vp, zp0, zp1 = int(top[c, 0, i, 0]), int(top[c, 0, i, 2]), int(top[c, 0, i, 3])
            for j in range(rt):
                inter = int(ov[i, j])
                if inter <= 0:
                    continue
                vt, zt0, zt1 = int(top[c, 1, j, 0]), int(top[c, 1, j, 2]), int(top[c, 1, j, 3])
                union = vp + vt - inter
                pairs.append({'pred': i, 'truth': j, 'intersection': inter, 'iou': inter / union, 'dice': 2 * inter / (vp + vt),
                              'length_pred': zp1 - zp0 + 1, 'length_truth': zt1 - zt0 + 1, 'start_offset': zp0 - zt0, 'end_offset': zp1 - zt1})
                if (2 * inter > union) if iou == 0.5 else (float(inter) > iou * float(union)):
                    matches.append([i, j])
                    ious.append(inter / union)
        ranked = ov[:rp, :rt] > 0
        tot = frames[c].astype(np.int64).sum(axis=0)
        cls = {'n_pred': n_pred, 'n_truth': n_truth, 'truncated': n_pred > TOPL or n_truth > TOPL,
               'unranked_overlap': {'pred_rest': int(ov[TOPL, :].sum()), 'truth_rest': int(ov[:, TOPL].sum())},
               'criterion': criterion, 'pairs': pairs}
        if criterion == 'iou':
            tp = len(matches)
            fp, fn = rp - tp, rt - tp
            sens, prec = _ratio(tp, tp + fn), _ratio(tp, tp + fp)
            sq = _ratio(sum(ious), tp)
            rq = _ratio(tp, tp + fp / 2 + fn / 2)
            cls.update({'iou_threshold': iou, 'matches': matches, 'tp': tp, 'fp': fp, 'fn': fn, 'sensitivity': sens, 'precision': prec,
                        'f1': _ratio(2 * tp, 2 * tp + fp + fn), 'sq': sq, 'rq': rq, 'pq': None if sq is None or rq is None else sq * rq})
        else:
            detected = int((ov[:, :rt].sum(axis=0) >= min_overlap).sum())
            true_pos = int((ov[:rp, :].sum(axis=1) >= min_overlap).sum())
            cls.update({'min_overlap': min_overlap, 'detected': detected, 'missed': rt - detected, 'true_positives': true_pos,
                        'false_positives': rp - true_pos, 'sensitivity': _ratio(detected, rt), 'precision': _ratio(true_pos, rp)})
        cls['split'] = int((ranked.sum(axis=0) >= 2).sum())
        cls['merged'] = int((ranked.sum(axis=1) >= 2).sum())
        cls['voxel_dice'] = _ratio(2 * int(tot[0]), int(tot[1]) + int(tot[2]))
        pres_p, pres_t = frames[c, :, 1] >= min_pixels, frames[c, :, 2] >= min_pixels
        ftp, ffp = int((pres_p & pres_t).sum()), int((pres_p & ~pres_t).sum())
        ffn, ftn = int((~pres_p & pres_t).sum()), int((~pres_p & ~pres_t).sum())
        cls['frames'] = {'min_pixels': min_pixels, 'tp': ftp, 'fp': ffp, 'fn': ffn, 'tn': ftn, 'sensitivity': _ratio(ftp, ftp + ffn),
                         'specificity': _ratio(ftn, ftn + ffp),
                         'dice': [_ratio(2 * int(f[0]), int(f[1]) + int(f[2])) for f in frames[c]]}
        if image_names is not None:
            cls['frames']['images'] = list(image_names)
        report[name] = cls
    return report


def _tables_to_host(m):
    """ONE device-to-host copy of the four tables, concatenated per channel."""
    sc, n = int(m.overlap.shape[0]), int(m.frames.shape[1])
    host = torch.cat([m.nles.reshape(sc, -1), m.top.reshape(sc, -1), m.overlap.reshape(sc, -1), m.frames.reshape(sc, -1)], dim=1).cpu().numpy()
    k, q = 2 * TOPL * len(TOP_COLUMNS), RANKS * RANKS
    return (host[:, :2], host[:, 2:2 + k].reshape(sc, 2, TOPL, len(TOP_COLUMNS)), host[:, 2 + k:2 + k + q].reshape(sc, RANKS, RANKS),
            host[:, 2 + k + q:].reshape(sc, n, 3))


def match_report(pred, truth, image_names=None, classes=None, across='overlap', **kw):
    """``build_match`` for two mask stacks on the device: ``match_volumes``, ONE device-to-host copy of the concatenated tables (about
    (1603 + 3 N) * 4 bytes per class), the rest on the host.  Keywords: ``build_match``'s."""
    bad = set(kw) - {'criterion', 'iou', 'min_overlap', 'min_pixels'}
    if bad:
        raise ValueError(f'unknown build_match keywords: {sorted(bad)}')
    m = match_volumes(pred, truth, across=across)
    return build_match(*_tables_to_host(m), int(pred.shape[1]), int(pred.shape[2]), image_names=image_names, classes=classes, **kw)


def _host_tables(pred, truth, across):
    """``match_volumes`` for numpy stacks: one upload each, one copy back."""
    dev = torch.device('cuda')
    up = [torch.from_numpy(np.ascontiguousarray(np.asarray(v) != 0).astype(np.float32)).to(dev) for v in (pred, truth)]
    return _tables_to_host(match_volumes(up[0], up[1], across=across))


def main(argv=None):
    from .distance import read_mask_dirs
    argv = list(sys.argv[1:] if argv is None else argv)
    usage = 'usage: python -m oct_segmentation_amd.match pred_dir truth_dir [save_dir] [across=overlap|full] [iou=0.5]'
    opts = {'across': 'overlap', 'iou': '0.5'}
    dirs = []
    for a in argv:
        key, eq, val = a.partition('=')
        if eq and key in opts:
            opts[key] = val
        else:
            dirs.append(a)
    if len(dirs) not in (2, 3) or opts['across'] not in ACROSS:
        raise SystemExit(usage)
    try:
        iou = float(opts['iou'])
    except ValueError:
        raise SystemExit(usage)
    if not 0.5 <= iou < 1.0:
        raise SystemExit(usage)
    pred_dir, truth_dir = dirs[:2]
    save_dir = dirs[2] if len(dirs) == 3 else pred_dir
    names, pred, truth = read_mask_dirs(pred_dir, truth_dir)
    n, h, w, sc = pred.shape
    if sc > lesions.MAX_CHANNELS or n * h * w >= 2 ** 31 - 1:
        raise ValueError(f'at most {lesions.MAX_CHANNELS} channels and fewer than 2^31 - 1 voxels, got {pred.shape}')
    classes = lesions.default_classes(sc)
    nles, top, overlap, frames = _host_tables(pred, truth, opts['across'])
    report = {'images': names, 'classes': classes, 'across': opts['across'], 'unit': 'voxel',
              'match': build_match(nles, top, overlap, frames, h, w, image_names=names, classes=classes, criterion='iou', iou=iou)}
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, 'lesion_match.json')
    with open(path, 'w') as f:
        json.dump(report, f, indent=1)
    print(path)
    return report


if __name__ == '__main__':
    main()
