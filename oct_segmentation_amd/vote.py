"""One mask voted by the folds of a class and by flipped / rotated views of the frame, and the map of where the members disagree
(``csrc/vote.hip``, ``octseg_vote_assemble``; no reference counterpart).

The reference trains five folds per class (``eval/training/<class>/fold_1..5``) and serves one.  Here every member -- a fold's network on one
view of the frame -- leaves its float32 logits on the device and ONE launch per class turns the ``M = folds x views`` tensors into the mask
channel, the mean probability, the per-pixel number of dissenting members and four integer counts per frame.  No logits tensor goes to the host.

    res = segment_stack_voted(images, [1000, 1000], classes, 'models', tta='flips', want_dissent=True)
    res.stack                                   # float32 CUDA [n, H, W, 4], what segment_stack returns: cleanup / analysis / polar / lesions take it
    res.dissent                                 # uint8 CUDA [n, H, W, 4]: members whose own threshold differs from the mask, 0 .. M // 2 (soft: .. M - 1)
    res.stats                                   # int32 CUDA [n, 4, 4]: frame, CLASS_ID - 1, (set, disputed, disputed_and_set, dissent_sum)
    vote_report(res, names, classes)            # the JSON dict predict writes as vote.json

View code ``v = a + 2 b + 4 t``: transpose if ``t``, then reverse the rows if ``b``, then reverse the columns if ``a`` (the dihedral group D4).
``mode='soft'`` thresholds the mean of the members' sigmoids at 0.5, ``'majority'`` counts their own thresholds; a tie is not set.
"""
import ctypes as C
import json
import os
import re
from collections import namedtuple

import torch

from . import _lib as L

MAX_MEMBERS = 64
VIEW_SETS = {'none': (0,), 'flips': (0, 1, 2, 3), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}
MODES = {'soft': 0, 'majority': 1}
STAT_COLUMNS = ('set', 'disputed', 'disputed_and_set', 'dissent_sum')

VoteResult = namedtuple('VoteResult', 'stack prob dissent stats members')


def view_batch(x, code):
    """View ``code`` of a float32 NCHW CUDA batch, contiguous: transpose if bit 2, flip the rows if bit 1, flip the columns if bit 0."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        raise ValueError('view_batch() takes a float32 NCHW CUDA tensor')
    code = int(code)
    if not 0 <= code <= 7:
        raise ValueError(f'view code must be in 0..7, got {code}')
    if code & 4:
        if x.shape[2] != x.shape[3]:
            raise ValueError(f'a transposed view needs square frames, got {tuple(x.shape[2:])}')
        x = x.transpose(-1, -2)
    dims = [d for d, bit in ((-2, 2), (-1, 1)) if code & bit]
    if dims:
        x = x.flip(dims)
    return x.contiguous()


def _check_out(t, name, like, dtype):
    if t is None:
        return
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f'{name} must be a contiguous {dtype} CUDA tensor')
    if like is not None and (tuple(t.shape) != tuple(like.shape) or t.device != like.device):
        raise ValueError(f'{name} must have the shape and device of out, {tuple(like.shape)}')


def vote_logits(members, channels, views, out, out_ch, rows=None, cols=None, mode='soft', prob=None, dissent=None, stats=None):
    """The thin door to ``octseg_vote_assemble``: ``members`` float32 NCHW CUDA logits, each in the coordinates of its view ``views[m]`` of the
    frame, of which channel ``channels[m]`` votes; ``out`` float32 CUDA [N, out_h, out_w, out_channels], written at channel ``out_ch`` only, as are
    ``prob`` (float32, the mean probability) and ``dissent`` (uint8), both of out's shape; ``stats`` int32 [N, 4].  ``rows`` / ``cols``: int32 CUDA
    source index of every output row / column of the un-viewed frame (``predict.cv2_nearest_index``), ``None`` = the centre rule.  Enqueue only."""
    if mode not in MODES:
        raise ValueError(f"mode must be 'soft' or 'majority', got {mode!r}")
    members, channels, views = list(members), [int(c) for c in channels], [int(v) for v in views]
    M = len(members)
    if not 1 <= M <= MAX_MEMBERS:
        raise ValueError(f'{M} members, not 1..{MAX_MEMBERS}')
    if len(channels) != M or len(views) != M:
        raise ValueError('members, channels and views must have one entry per member')
    _check_out(out, 'out', None, torch.float32)
    if out is None or out.dim() != 4 or 0 in out.shape:
        raise ValueError('out must be a non-empty float32 CUDA tensor [N, out_h, out_w, out_channels]')
    N, oh, ow, oc = (int(v) for v in out.shape)
    if not 0 <= int(out_ch) < oc:
        raise ValueError(f'out_ch {out_ch} outside [0, {oc})')
    _check_out(prob, 'prob', out, torch.float32)
    _check_out(dissent, 'dissent', out, torch.uint8)
    _check_out(stats, 'stats', None, torch.int32)
    if stats is not None and (tuple(stats.shape) != (N, 4) or stats.device != out.device):
        raise ValueError(f'stats must be int32 [{N}, 4] on the device of out')
    H = W = None
    for m, (z, c, v) in enumerate(zip(members, channels, views)):
        if not (torch.is_tensor(z) and z.is_cuda and z.dtype == torch.float32 and z.dim() == 4 and z.is_contiguous()):
            raise ValueError(f'member {m}: logits must be a contiguous float32 NCHW CUDA tensor')
        if 0 in z.shape or z.shape[0] != N or z.device != out.device:
            raise ValueError(f'member {m}: logits {tuple(z.shape)} are empty or do not match the {N} frames / the device of out')
        if not 0 <= v <= 7:
            raise ValueError(f'member {m}: view code {v} outside 0..7')
        if not 0 <= c < z.shape[1]:
            raise ValueError(f'member {m}: channel {c} outside [0, {z.shape[1]})')
        if v & 4 and z.shape[2] != z.shape[3]:
            raise ValueError(f'member {m}: a transposed view needs square frames, got {tuple(z.shape[2:])}')
        if H is None:
            H, W = int(z.shape[2]), int(z.shape[3])      # (a transposed member is square: the un-viewed extents either way)
        elif (int(z.shape[2]), int(z.shape[3])) != (H, W):
            raise ValueError(f'member {m}: frame {tuple(z.shape[2:])} differs from member 0, {(H, W)}')
    for t, name, length in ((rows, 'rows', oh), (cols, 'cols', ow)):
        if t is not None and not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (length,)):
            raise ValueError(f'{name} must be a contiguous int32 CUDA tensor [{length}]')
    ptrs = (C.c_void_p * M)(*[z.data_ptr() for z in members])
    ints = [(C.c_int * M)(*vals) for vals in ([int(z.shape[1]) for z in members], channels, views)]
    with torch.cuda.device(out.device):
        L.check(L.lib().octseg_vote_assemble(ptrs, ints[0], ints[1], ints[2], M, N, H, W, MODES[mode], L.ptr(out), oh, ow, oc, int(out_ch),
                                             L.ptr(rows), L.ptr(cols), L.ptr(prob), L.ptr(dissent), L.ptr(stats), L.stream_ptr()))
    return out


def _model_dir(class_name):
    from .predict import MODELS_META
    return MODELS_META[class_name]['model_dir']


def find_members(models_dir, class_name):
    """The member directories of a class: ``<models_dir>/<LM|FC_LC|VV>/fold_<k>/`` holding ``config.json`` and ``weights.ckpt``, ordered by the
    integer ``k``; when there are none, the single ``<models_dir>/<LM|FC_LC|VV>`` that ``predict.segment_stack`` loads.  Folds whose ``input_size``
    or class lists differ are refused: their logits could not be voted pixel by pixel."""
    base = os.path.join(str(models_dir), _model_dir(class_name))
    found = []
    if os.path.isdir(base):
        for name in os.listdir(base):
            m = re.fullmatch(r'fold_(\d+)', name)
            d = os.path.join(base, name)
            if m and os.path.isfile(os.path.join(d, 'config.json')) and os.path.isfile(os.path.join(d, 'weights.ckpt')):
                found.append((int(m.group(1)), name, d))
    if not found:
        return [base]
    dirs = [d for _, _, d in sorted(found)]
    first = None
    for d in dirs:
        with open(os.path.join(d, 'config.json')) as f:
            cfg = json.load(f)
        key = (int(cfg['input_size']), list(cfg['classes']))
        if first is None:
            first = key
        elif key != first:
            raise ValueError(f'{d}: input_size / classes {key} differ from those of {dirs[0]}, {first}')
    return dirs


def segment_stack_voted(images, output_size, classes, models_dir, tta='none', folds=True, mode='soft', want_prob=False, want_dissent=False,
                        device='cuda', batch_size=8, compute_dtype=torch.bfloat16, thresholds=None):
    """``predict.segment_stack`` voted: per class every fold found by ``find_members`` (``folds=False``: the single directory of today) runs once per
    view of ``VIEW_SETS[tta]``, and the ``M = folds x views`` logits tensors of a batch (folds outer, views inner) go into one
    ``octseg_vote_assemble`` launch per class.  Preprocessing, channel mapping and resize tables are ``segment_stack``'s (device-preprocess path);
    a two-class FC_LC network runs once and is voted twice.  Eager forwards; one batch of member logits is alive at a time.
    Returns ``VoteResult(stack, prob, dissent, stats, members)``: ``stack`` float32 [n, H, W, 4] as ``segment_stack``'s, ``prob`` float32 and
    ``dissent`` uint8 of the same shape (``None`` unless asked for), ``stats`` int32 [n, 4, 4] (frame, CLASS_ID - 1, STAT_COLUMNS), ``members``
    class name -> M.  Channels of classes that were not asked for stay 0.  ``thresholds`` (default ``None``: nothing changes): ``{class name: t}``;
    every member's logits channel of a class named is shifted by ``curves.apply_thresholds`` before the vote, so that each member votes, and the
    soft vote cuts, at ``t`` instead of 0.5."""
    from .model import CLASS_IDS
    from .predict import MODELS_META, _resize_frames_on_device, _upload_frames_u8, cv2_nearest_index, load_model
    if tta not in VIEW_SETS:
        raise ValueError(f'tta must be one of {sorted(VIEW_SETS)}, got {tta!r}')
    if mode not in MODES:
        raise ValueError(f"mode must be 'soft' or 'majority', got {mode!r}")
    if thresholds is not None:
        from .curves import apply_thresholds, read_thresholds
        thresholds = read_thresholds(thresholds)
    if torch.is_tensor(images):
        if not (images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4 and images.shape[3] == 3 and images.shape[0] > 0):
            raise ValueError('a frame tensor must be a non-empty uint8 CUDA tensor [n, H, W, 3] (RGB)')
        frames_u8, device = images.contiguous(), images.device
    else:
        if len(images) == 0:
            raise ValueError('no frames')
        frames_u8 = _upload_frames_u8(images, device)
    views = VIEW_SETS[tta]
    n = len(images)
    oh, ow = int(output_size[0]), int(output_size[1])
    stack = torch.zeros((n, oh, ow, 4), dtype=torch.float32, device=device)
    prob = torch.zeros_like(stack) if want_prob else None
    dissent = torch.zeros((n, oh, ow, 4), dtype=torch.uint8, device=device) if want_dissent else None
    stats = torch.zeros((4, n, 4), dtype=torch.int32, device=device)     # a launch writes the [b, 4] rows of one class
    loaded, members = {}, {}
    for class_name in classes:     # every distinct network once, as in segment_stack
        key = MODELS_META[class_name]['model_dir']
        if key not in loaded:
            dirs = find_members(models_dir, class_name) if folds else [os.path.join(str(models_dir), key)]
            nets = [load_model(d, device, compute_dtype) for d in dirs]
            sizes = {int(cfg['input_size']) for _, cfg in nets}
            if len(sizes) != 1:
                raise ValueError(f'{key}: the members have different input sizes {sorted(sizes)}')
            loaded[key] = ([model for model, _ in nets], sizes.pop())
        members[class_name] = len(loaded[key][0]) * len(views)
        if members[class_name] > MAX_MEMBERS:
            raise ValueError(f'{class_name}: {members[class_name]} members, at most {MAX_MEMBERS}')
    tables = {}
    for i in range(0, n, batch_size):
        b = min(batch_size, n - i)
        for key, (nets, size) in loaded.items():
            x = _resize_frames_on_device(frames_u8, i, i + batch_size, size)
            xs = [view_batch(x, v) for v in views]
            logits = [model.predict_logits(xv) for model in nets for xv in xs]      # folds outer, views inner
            codes = [v for _ in nets for v in views]
            if size not in tables:   # cv2.resize(predict_mask, tuple(output_size), INTER_NEAREST): resizeNN's row / column tables
                tables[size] = (torch.from_numpy(cv2_nearest_index(size, oh)).to(device), torch.from_numpy(cv2_nearest_index(size, ow)).to(device))
            rows, cols = tables[size]
            shifted = set()      # (a class listed twice is shifted once per batch)
            for class_name in classes:
                meta = MODELS_META[class_name]
                if meta['model_dir'] != key:
                    continue
                c = CLASS_IDS[class_name] - 1
                chans = [meta['index'] if z.shape[1] > 1 else 0 for z in logits]
                if thresholds is not None and class_name in thresholds and class_name not in shifted:
                    for z, ch in zip(logits, chans):
                        apply_thresholds(z, [ch], [thresholds[class_name]])
                    shifted.add(class_name)
                vote_logits(logits, chans, codes, stack[i:i + b], c, rows, cols, mode,
                            prob=None if prob is None else prob[i:i + b], dissent=None if dissent is None else dissent[i:i + b],
                            stats=stats[c, i:i + b])
            del logits, xs, x
    return VoteResult(stack, prob, dissent, stats.permute(1, 0, 2).contiguous(), members)


def vote_report(result, names, classes):
    """The JSON dict of a voted prediction: per class the number of members and, per slice in the order of ``names``, the four counts of
    ``STAT_COLUMNS`` and ``disputed_ratio = disputed / max(set, 1)``.  One copy of the [n, 4, 4] counts to the host."""
    from .model import CLASS_IDS
    stats = result.stats.cpu().numpy()
    if stats.shape[0] != len(names):
        raise ValueError(f'{len(names)} names for {stats.shape[0]} slices')
    report = {'columns': list(STAT_COLUMNS), 'classes': {}}
    for class_name in classes:
        rows = stats[:, CLASS_IDS[class_name] - 1]
        slices = {}
        for name, row in zip(names, rows):
            entry = {k: int(v) for k, v in zip(STAT_COLUMNS, row)}
            entry['disputed_ratio'] = entry['disputed'] / max(entry['set'], 1)
            slices[name] = entry
        report['classes'][class_name] = {'members': int(result.members[class_name]), 'slices': slices}
    return report


def dissent_images(result, classes):
    """uint8 host array [n, H, W]: per pixel the maximum over the classes of ``dissent * (255 // M_class)``, what predict writes as
    ``{name}_dissent.png``."""
    from .model import CLASS_IDS
    if result.dissent is None:
        raise ValueError('the result holds no dissent map (want_dissent=False)')
    ids = [CLASS_IDS[c] - 1 for c in classes]
    scale = torch.tensor([255 // int(result.members[c]) for c in classes], dtype=torch.uint8, device=result.dissent.device)
    return (result.dissent[..., ids] * scale).amax(dim=-1).cpu().numpy()
