"""Time of the per-epoch panel kernel (csrc/panels.hip, postprocess.epoch_panels).  Needs an MI355X.

One launch paints N strips of S x 3 S pixels from the resized frames, the logits and the source-size ground truth.  The kernel alone is timed
with device events around REPS back-to-back launches after a warm-up (profiler off), in ROUNDS rounds whose spread is printed; the bytes are
what the launch has to move once, from the shapes (ground truth: the source pixels the nearest tables touch).

    python tools/bench_panels.py [--n 32] [--size 512] [--src 1000] [--classes 4] [--out out/panels.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
REPS, ROUNDS, WARMUP = 200, 5, 20


def launch_bytes(n, s, src, c, labels=True):
    from oct_segmentation_amd.predict import cv2_nearest_index
    touched = len(np.unique(cv2_nearest_index(src, s))) ** 2 * 4
    return n * (3 * s * s * 4 + c * s * s * 4 + touched + 9 * s * s + (2 * s * s if labels else 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=32)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--src', type=int, default=1000)
    ap.add_argument('--classes', type=int, default=4)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from oct_segmentation_amd import _lib as L, ingest, postprocess
    if not torch.cuda.is_available():
        raise SystemExit('bench_panels: no GPU visible; there is nothing to measure without one')
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cpu').manual_seed(1)
    classes = ALL[:a.classes]
    frames = torch.randint(0, 256, (a.n, 3, a.size, a.size), generator=g).float().to(dev)
    logits = torch.randn((a.n, len(classes), a.size, a.size), generator=g).to(dev)
    gt = (torch.randint(0, 2, (a.n, a.src, a.src, 4), generator=g) * 255).to(torch.uint8).to(dev)
    want, want_lab = postprocess.epoch_panels(frames, logits, gt, classes)
    # the timed loop goes straight through the C entry into preallocated outputs: no allocation, one ctypes call per launch
    ch = torch.tensor([postprocess.CLASS_IDS[c] - 1 for c in classes], dtype=torch.int32, device=dev)
    rgb = torch.tensor([postprocess.CLASS_COLORS_RGB[c] for c in classes], dtype=torch.uint8, device=dev)
    ids = torch.tensor([postprocess.CLASS_IDS[c] for c in classes], dtype=torch.uint8, device=dev)
    idx = ingest._nearest_dev(a.src, a.size, dev)
    out, lab = torch.empty_like(want), torch.empty_like(want_lab)
    fn, st = L.lib().octseg_epoch_panels, L.stream_ptr()
    args = (L.ptr(frames), L.ptr(logits), L.ptr(gt), a.n, a.size, len(classes), a.src, a.src, 4, L.ptr(idx), L.ptr(idx), L.ptr(ch), L.ptr(rgb),
            L.ptr(ids), L.ptr(out), L.ptr(lab), st)
    for _ in range(WARMUP):
        L.check(fn(*args))
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(lab, want_lab)
    us = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn(*args)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / REPS)
    nbytes = launch_bytes(a.n, a.size, a.src, len(classes))
    med = statistics.median(us)
    res = {'kernel': 'epoch_panels_kernel', 'n': a.n, 'size': a.size, 'src': a.src, 'classes': len(classes), 'reps': REPS,
           'us_per_call_rounds': [round(u, 2) for u in us], 'us_per_call_median': round(med, 2), 'bytes': nbytes,
           'tb_per_s': round(nbytes / med / 1e6, 3),
           'note': 'device events around back-to-back launches through the C entry, preallocated outputs'}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
