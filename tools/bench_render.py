"""Measurements of the GPU rendering step (csrc/render.hip, oct_segmentation_amd/postprocess.py).  Needs an MI355X.

  kernel   launch render_kernel at N = 8, 1000 x 1000, four classes, realistic masks (filled ellipses), close_iterations 1 and 3 alternating;
           run it under the profiler, in a run of its own:
               rocprofv3 --kernel-trace --stats -d out/render_prof -- python tools/bench_render.py kernel
  compare  in ONE process, with events: the three nets' forwards + mask assembly for a batch of 8 (what bench.py's ensemble step runs),
           the render of that batch, the device-to-host copies before (float32 stack) and after (uint8 overlay + colour mask); and the host
           restatement of save_results (tests/postprocess_ref.py: numpy + PIL, NOT cv2) on one frame, for the record:
               python tools/bench_render.py compare --out out/render_compare.json
  record   merge both into profiles/render_1000.json:
               python tools/bench_render.py record --prof out/render_prof --compare out/render_compare.json --commit <id> \\
                   --out profiles/render_1000.json
"""
import argparse
import glob
import json
import os
import sqlite3
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N, SIZE, CLASSES = 8, 1000, ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
HBM_ACHIEVABLE_TBS = 6.3
# bytes the step has to move once per pixel: 16 of float32 stack, 3 of frame in, 3 + 3 out
BYTES_PER_PIXEL = 16 + 3 + 3 + 3


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_render: no GPU visible; there is nothing to measure without one')
    return torch.device('cuda:0')


def elliptic_masks(n=N, size=SIZE):
    """Vessel-like masks: a large lumen, a cap and a core beside it, a small vasa vasorum -- filled ellipses, shifted per frame."""
    yy, xx = np.mgrid[0:size, 0:size]
    masks = np.zeros((n, size, size, 4), np.float32)
    for i in range(n):
        for c, (cy, cx, ry, rx) in enumerate([(500, 470 + 8 * i, 300, 330), (420, 620 - 5 * i, 130, 210), (570, 380, 95, 60 + 4 * i), (140, 820, 40, 26)]):
            masks[i, :, :, c] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return masks


def kernel_bytes(n=N, size=SIZE):
    return n * size * size * BYTES_PER_PIXEL


def run_kernel(args):
    import torch
    from oct_segmentation_amd import postprocess
    dev = _need_gpu()
    g = torch.Generator(device='cpu').manual_seed(1)
    frames = torch.randint(0, 256, (N, SIZE, SIZE, 3), dtype=torch.uint8, generator=g).to(dev)
    stack = torch.from_numpy(elliptic_masks()).to(dev)
    for rep in range(args.reps + 3):               # the record drops the first three calls of each form (code-object load, cold caches)
        for it in (1, 3):
            postprocess.render_results(frames, stack, CLASSES, close_iterations=it)
    torch.cuda.synchronize()
    print(json.dumps({'reps': args.reps, 'order': 'close_iterations 1, 3 alternating', 'bytes': kernel_bytes()}))


def _events_ms(fn, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def run_compare(args):
    import torch
    from PIL import Image
    import postprocess_ref as R
    from oct_segmentation_amd import _lib as L, postprocess
    from oct_segmentation_amd.engine import SegNet
    from oct_segmentation_amd.model import CLASS_IDS
    from oct_segmentation_amd.predict import MODELS_META, cv2_nearest_index
    from synth import make_batch
    dev = _need_gpu()
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    S = 704
    ensemble = (('unetplusplus', 'resnet101', ['Lumen']), ('linknet', 'resnet50', ['Lipid core', 'Fibrous cap']), ('unet', 'resnet50', ['Vasa vasorum']))
    nets = []
    for i, (arch, enc, classes) in enumerate(ensemble):
        net = SegNet(arch, enc, classes=len(classes), device=dev, compute_dtype=torch.float16, seed=40 + i).eval()
        net.use_graph = True
        nets.append((net, classes))
    x = make_batch(N, 1, S, seed=7)[0].to(dev)
    stack = torch.zeros((N, SIZE, SIZE, 4), dtype=torch.float32, device=dev)
    rows = torch.from_numpy(cv2_nearest_index(S, SIZE)).to(dev)
    lib = L.lib()

    def forwards():                                # bench.py's ensemble step: replayed graphs side by side, then the mask assembly
        handles = [net.forward_async(x, normalize=False) for net, _ in nets]
        for (net, classes), h in zip(nets, handles):
            z = net.forward_join(h)
            for cl in classes:
                ch = MODELS_META[cl]['index'] if z.shape[1] > 1 else 0
                L.check(lib.octseg_mask_assemble(L.ptr(z), N, z.shape[1], S, S, int(ch), L.ptr(stack), SIZE, SIZE, 4, CLASS_IDS[cl] - 1,
                                                 L.ptr(rows), L.ptr(rows), L.stream_ptr()))

    t_fwd = _events_ms(forwards, args.reps)
    g = torch.Generator(device='cpu').manual_seed(1)
    frames = torch.randint(0, 256, (N, SIZE, SIZE, 3), dtype=torch.uint8, generator=g).to(dev)
    masks = elliptic_masks()
    real = torch.from_numpy(masks).to(dev)
    out = {'batch': N, 'frame': f'{SIZE}x{SIZE}', 'classes': len(CLASSES), 'reps': args.reps,
           'ensemble_forward_ms_per_batch': round(statistics.median(t_fwd), 3),
           'ensemble_forward_ms_per_frame': round(statistics.median(t_fwd) / N, 3)}
    for it in (1, 3):
        t = _events_ms(lambda: postprocess.render_results(frames, real, CLASSES, close_iterations=it), args.reps)
        out[f'render_events_ms_per_batch_it{it}'] = round(statistics.median(t), 4)
        out[f'render_events_ms_per_frame_it{it}'] = round(statistics.median(t) / N, 4)
    out['render_over_forward'] = round(out['render_events_ms_per_batch_it1'] / out['ensemble_forward_ms_per_batch'], 5)
    # device-to-host traffic of predict per frame: the float32 stack (parent commit's segment()) against overlay + colour mask
    ov, cm = postprocess.render_results(frames, real, CLASSES)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); real.cpu(); t1 = time.perf_counter(); torch.stack([ov, cm]).cpu(); t2 = time.perf_counter()
    out['d2h'] = {'before_bytes_per_frame': SIZE * SIZE * 4 * 4, 'after_bytes_per_frame': SIZE * SIZE * 3 * 2,
                  'before_s_per_batch_pageable': round(t1 - t0, 4), 'after_s_per_batch_pageable': round(t2 - t1, 4)}
    # (b) the host restatement on this box's CPU share, one frame, for the record only: numpy + PIL, not cv2
    fr = frames[0].cpu().numpy()
    host = {}
    for it in (1, 3):
        t0 = time.perf_counter()
        want = R.render(Image.fromarray(fr), masks[0], CLASSES, it)
        host[f'it{it}_s_per_frame'] = round(time.perf_counter() - t0, 3)
        got = postprocess.render_results(frames[:1], real[:1], CLASSES, close_iterations=it)
        host[f'it{it}_equal'] = bool(np.array_equal(got[0][0].cpu().numpy(), want[0]) and np.array_equal(got[1][0].cpu().numpy(), want[1]))
    out['host_restatement_numpy_pil'] = host
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not all(host[f'it{it}_equal'] for it in (1, 3)):
        raise SystemExit('kernel and host restatement disagree')


def _kernel_times(prof_dir):
    """render_kernel durations in microseconds, in launch order, from rocprofv3's database or its kernel-trace csv."""
    dbs = sorted(glob.glob(os.path.join(prof_dir, '**', '*.db'), recursive=True), key=os.path.getmtime)
    if dbs:
        rows = sqlite3.connect(dbs[-1]).execute('select name, start, end from kernels order by start').fetchall()
    else:
        import csv
        files = sorted(glob.glob(os.path.join(prof_dir, '**', '*kernel_trace.csv'), recursive=True), key=os.path.getmtime)
        if not files:
            raise SystemExit(f'no rocprofv3 .db or kernel_trace.csv under {prof_dir}')
        with open(files[-1], newline='') as f:
            rows = sorted(((r['Kernel_Name'], int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in csv.DictReader(f)), key=lambda r: r[1])
    return [(end - start) / 1e3 for name, start, end in rows if 'render_kernel' in name]


def run_record(args):
    us = _kernel_times(args.prof)
    nbytes = kernel_bytes()
    rec = {'commit': args.commit, 'device': 'MI355X (gfx950)', 'batch': N, 'frame': f'{SIZE}x{SIZE}', 'classes': len(CLASSES),
           'masks': 'filled ellipses (tools/bench_render.py elliptic_masks), frames uniform noise',
           'method': 'kernel times: rocprofv3 --kernel-trace --stats in a run of its own, close_iterations 1 and 3 alternating, first 3 calls of '
                     'each dropped, median of the rest; bytes from the shapes (25 B / pixel); TB/s = bytes / median time',
           'hbm_achievable_tbs': HBM_ACHIEVABLE_TBS, 'kernel': {}}
    for k, it in enumerate((1, 3)):
        t = us[k::2][3:]
        med = statistics.median(t)
        rec['kernel'][f'render_kernel close_iterations={it}'] = {
            'calls': len(t), 'median_us': round(med, 2), 'min_us': round(min(t), 2), 'max_us': round(max(t), 2), 'us_per_frame': round(med / N, 2),
            'bytes': nbytes, 'tb_per_s': round(nbytes / med / 1e6, 3), 'floor_us_at_achievable_hbm': round(nbytes / HBM_ACHIEVABLE_TBS / 1e6, 2)}
    if args.compare:
        with open(args.compare) as f:
            rec['same_process_comparison'] = json.load(f)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec, indent=1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    k = sub.add_parser('kernel'); k.add_argument('--reps', type=int, default=20)
    c = sub.add_parser('compare'); c.add_argument('--reps', type=int, default=10); c.add_argument('--out', default=None)
    r = sub.add_parser('record'); r.add_argument('--prof', required=True); r.add_argument('--compare', default=None)
    r.add_argument('--commit', default='unknown'); r.add_argument('--out', required=True)
    args = ap.parse_args()
    {'kernel': run_kernel, 'compare': run_compare, 'record': run_record}[args.cmd](args)


if __name__ == '__main__':
    main()
