"""Measurements of the raw-volume kernels (csrc/volume.hip, oct_segmentation_amd/pullback.py).  Needs an MI355X.

The volume is the size of the reference's demo pullback: 186 slices of 750 x 750 x 3, uint16 from a seed, resized to 1000 x 1000.

  compare  in ONE process, median of --reps after warm-up: normalise and resize separately, the calls alone (device events, data resident)
           and end to end from the host array (host clock to a synchronise, upload of the SOURCE-size volume included); and the host
           path on the box's CPU share -- numpy normalise + Image.resize per frame + upload of the ENLARGED frames; checks that both
           paths give the same bytes:
               python tools/bench_pullback.py compare --out out/pullback_compare.json
  kernel   the calls in a loop, for the profiler, in a run of its own:
               rocprofv3 --kernel-trace --stats -d out/pullback_prof -- python tools/bench_pullback.py kernel
  record   merge both into profiles/pullback_186.json (kernel times from the trace, bytes from the shapes):
               python tools/bench_pullback.py record --prof out/pullback_prof --compare out/pullback_compare.json --commit <id> \\
                   --out profiles/pullback_186.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

S, SRC, DST, C = 186, 750, 1000, 3
WARMUP = 3


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_pullback: no GPU visible; there is nothing to measure without one')
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    return torch.device('cuda:0')


def seeded_volume(s=S, size=SRC):
    """uint16 [s, size, size, 3]: noise over a disc, with a range of its own per slice."""
    rng = np.random.default_rng(186)
    vol = rng.integers(0, 3000, (s, size, size, C), dtype=np.uint16)
    yy, xx = np.mgrid[0:size, 0:size]
    disc = (yy - size // 2) ** 2 + (xx - size // 2) ** 2 < (size // 3) ** 2
    for k in range(s):
        vol[k][disc] += np.uint16(10000 + 200 * k)
    return vol


def kernel_bytes(s=S, src=SRC, dst=DST):
    """Bytes every kernel has to move, from its shapes."""
    vol, u8 = s * src * src * C * 2, s * src * src * 3
    return {'minmax_kernel': vol, 'normalize_kernel': vol + u8,
            'resample_kernel<horizontal>': u8 + s * src * dst * C, 'resample_kernel<vertical>': s * src * dst * C + s * dst * dst * C}


def _events_ms(fn, reps):
    import torch
    for _ in range(WARMUP):
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


def _wall_ms(fn, reps, warmup=1):
    import torch
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def _stat(t):
    return {'median': round(statistics.median(t), 3), 'min': round(min(t), 3), 'max': round(max(t), 3), 'reps': len(t)}


def run_kernel(args):
    import torch
    from oct_segmentation_amd import pullback
    dev = _need_gpu()
    vol = torch.from_numpy(seeded_volume()).to(dev)
    for _ in range(args.reps + WARMUP):
        frames = pullback.normalize_volume(vol)
        pullback.resize_pil_u8(frames, DST)
    torch.cuda.synchronize()
    print(json.dumps({'reps': args.reps}))


def run_compare(args):
    import torch
    from PIL import Image
    import volume_ref as R
    from oct_segmentation_amd import pullback
    dev = _need_gpu()
    vol = seeded_volume()
    vol_dev = torch.from_numpy(vol).to(dev)
    frames_dev = pullback.normalize_volume(vol_dev)
    out = {'slices': S, 'source': f'{SRC}x{SRC}x{C} uint16', 'output': f'{DST}x{DST}', 'volume_bytes': int(vol.nbytes),
           'source_frames_bytes': S * SRC * SRC * 3, 'enlarged_frames_bytes': S * DST * DST * 3, 'cpu_threads': torch.get_num_threads()}
    out['device_calls_events_ms'] = {
        'normalize_volume': _stat(_events_ms(lambda: pullback.normalize_volume(vol_dev), args.reps)),
        'resize_pil_u8': _stat(_events_ms(lambda: pullback.resize_pil_u8(frames_dev, DST), args.reps))}
    print(json.dumps(out['device_calls_events_ms']), flush=True)
    src_frames = frames_dev.cpu().numpy()
    out['device_end_to_end_ms'] = {
        'normalize_volume_from_host': _stat(_wall_ms(lambda: pullback.normalize_volume(vol), args.reps)),
        'upload_and_resize_from_host': _stat(_wall_ms(lambda: pullback.resize_pil_u8(torch.from_numpy(src_frames).to(dev), DST), args.reps)),
        'volume_to_enlarged_frames': _stat(_wall_ms(lambda: pullback.resize_pil_u8(pullback.normalize_volume(vol), DST), args.reps))}
    print(json.dumps(out['device_end_to_end_ms']), flush=True)
    host, t_norm, t_resize = {}, [], []
    for rep in range(args.host_reps + 1):               # the first round is warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames = R.normalize_ref(vol)
        t1 = time.perf_counter()
        host['big'] = torch.from_numpy(np.stack([np.asarray(Image.fromarray(f).resize((DST, DST))) for f in frames])).to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:
            t_norm.append((t1 - t0) * 1e3)
            t_resize.append((t2 - t1) * 1e3)
        print(f'host round {rep}: {t1 - t0:.2f} s + {t2 - t1:.2f} s', flush=True)
    out['host_path_ms'] = {'numpy_normalize': _stat(t_norm), 'pil_resize_and_upload_enlarged': _stat(t_resize),
                           'volume_to_enlarged_frames': _stat([a + b for a, b in zip(t_norm, t_resize)])}
    got = pullback.resize_pil_u8(pullback.normalize_volume(vol), DST)
    out['equal'] = bool(torch.equal(got, host['big']))
    d, h = out['device_end_to_end_ms'], out['host_path_ms']
    out['host_over_device_end_to_end'] = {
        'normalize': round(h['numpy_normalize']['median'] / d['normalize_volume_from_host']['median'], 2),
        'resize': round(h['pil_resize_and_upload_enlarged']['median'] / d['upload_and_resize_from_host']['median'], 2),
        'both': round(h['volume_to_enlarged_frames']['median'] / d['volume_to_enlarged_frames']['median'], 2)}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not out['equal']:
        raise SystemExit('device and host path disagree')


def run_record(args):
    import csv
    import glob
    import sqlite3
    rows = None
    dbs = sorted(glob.glob(os.path.join(args.prof, '**', '*.db'), recursive=True), key=os.path.getmtime)
    if dbs:
        try:
            rows = sqlite3.connect(dbs[-1]).execute('select name, start, end from kernels order by start').fetchall()
        except sqlite3.Error:
            rows = None
    if rows is None:
        files = sorted(glob.glob(os.path.join(args.prof, '**', '*kernel_trace.csv'), recursive=True), key=os.path.getmtime)
        if not files:
            raise SystemExit(f'no rocprofv3 .db or kernel_trace.csv under {args.prof}')
        with open(files[-1], newline='') as f:
            rows = sorted(((r['Kernel_Name'], int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in csv.DictReader(f)), key=lambda r: r[1])
    keys = {'minmax_kernel': lambda n: 'minmax_kernel' in n, 'normalize_kernel': lambda n: 'normalize_kernel' in n,
            'resample_kernel<horizontal>': lambda n: 'resample_kernel' in n and ('false' in n or 'Lb0' in n),
            'resample_kernel<vertical>': lambda n: 'resample_kernel' in n and ('true' in n or 'Lb1' in n)}
    nbytes = kernel_bytes()
    rec = {'commit': args.commit, 'date': args.date, 'device': 'MI355X (gfx950)', 'measured': 'once', 'slices': S,
           'source': f'{SRC}x{SRC}x{C} uint16', 'output': f'{DST}x{DST}',
           'method': f'kernel times: rocprofv3 --kernel-trace --stats in a run of its own, first {WARMUP} calls dropped, median of the rest; '
                     'bytes from the shapes; TB/s = bytes / median time', 'kernel': {}}
    for k, match in keys.items():
        t = [(e - s) / 1e3 for n, s, e in rows if match(n)][WARMUP:]
        if not t:
            raise SystemExit(f'no {k} launches in {args.prof}')
        med = statistics.median(t)
        rec['kernel'][k] = {'calls': len(t), 'median_us': round(med, 2), 'min_us': round(min(t), 2), 'max_us': round(max(t), 2),
                            'bytes': nbytes[k], 'tb_per_s': round(nbytes[k] / med / 1e6, 3)}
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
    c = sub.add_parser('compare'); c.add_argument('--reps', type=int, default=20); c.add_argument('--host-reps', type=int, default=20)
    c.add_argument('--out', default=None)
    r = sub.add_parser('record'); r.add_argument('--prof', required=True); r.add_argument('--compare', default=None)
    r.add_argument('--commit', default='unknown'); r.add_argument('--date', default='unknown'); r.add_argument('--out', required=True)
    args = ap.parse_args()
    {'kernel': run_kernel, 'compare': run_compare, 'record': run_record}[args.cmd](args)


if __name__ == '__main__':
    main()
