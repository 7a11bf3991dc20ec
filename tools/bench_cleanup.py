"""Measurements of the mask clean-up kernels (csrc/components.hip, oct_segmentation_amd/cleanup.py).  Needs an MI355X.

  kernel   clean_stack at N = 186, 1000 x 1000, four classes (the output size of configs/predict.yaml; the float32 stack is 2.98 GB), the
           golden demo planes tiled to the frame and speckled with seeded salt noise; run it under the profiler, in a run of its own:
               rocprofv3 --kernel-trace --stats -d out/cleanup_prof -- python tools/bench_cleanup.py kernel
  compare  in ONE process: clean_stack with events around the calls (median of 20 after warm-up) and as wall time end to end, and the host
           comparator -- device-to-host copy of the stack, then the scipy path of tests/cleanup_ref.py with the planes spread over 16 worker
           processes that never touch the GPU; checks that both give the same bytes:
               python tools/bench_cleanup.py compare --out out/cleanup_compare.json
  record   merge both into profiles/cleanup_186.json:
               python tools/bench_cleanup.py record --prof out/cleanup_prof --compare out/cleanup_compare.json --commit <id> \\
                   --out profiles/cleanup_186.json
"""
import argparse
import glob
import json
import multiprocessing as mp
import os
import re
import sqlite3
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

if os.environ.get('OCTSEG_LIB'):   # an experimental build of the library (timing experiments)
    from oct_segmentation_amd import _lib as _L
    _L.LIB_PATH = os.path.abspath(os.environ['OCTSEG_LIB'])

N, SIZE, CHANNELS = 186, 1000, 4
WARMUP = 3
WORKERS = 16
KERNELS = ('bits_pack_kernel', 'morph_kernel', 'ccl_init_kernel', 'ccl_merge_kernel', 'ccl_flatten_kernel', 'area_kernel', 'select_kernel',
           'ccl_keep_kernel', 'border_kernel', 'fill_kernel', 'bits_unpack_kernel')      # ccl_*: launched by the labelling and by the hole fill


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_cleanup: no GPU visible; there is nothing to measure without one')
    return torch.device('cuda:0')


def host_planes(n=N, size=SIZE, seed=186, p=0.002):
    """bool [n, 4, size, size]: per slice and class a golden demo plane of that class tiled to the frame (Lumen in every slice, the others in
    runs, Fibrous cap never: the fixture has none), plus salt noise at p on every plane."""
    import cleanup_ref as R
    planes, _, channels, _, _ = R.golden_planes()
    by_class = {c: [np.tile(planes[i], (2, 2))[:size, :size] for i in range(len(planes)) if channels[i] == c] for c in range(CHANNELS)}
    rng = np.random.RandomState(seed)
    out = np.zeros((n, CHANNELS, size, size), bool)
    for i in range(n):
        for c in range(CHANNELS):
            if by_class[c] and (c == 0 or (i // 8 + c) % 3 == 0):
                out[i, c] = by_class[c][i % len(by_class[c])]
            out[i, c] |= rng.rand(size, size) < p
    return out


def device_stack(planes, dev):
    import torch
    n = planes.shape[0]
    stack = torch.empty((n, planes.shape[2], planes.shape[3], CHANNELS), dtype=torch.float32, device=dev)
    for i in range(n):
        stack[i] = torch.from_numpy(planes[i]).to(dev).permute(1, 2, 0).to(torch.float32)
    return stack


def _clean_packed(args):
    """Worker: one plane as packed bits in, the cleaned plane as packed bits out (numpy and scipy only)."""
    import cleanup_ref as R
    packed, size = args
    plane = np.unpackbits(packed)[:size * size].reshape(size, size)
    return np.packbits(R.clean(plane))


def run_kernel(args):
    import torch
    from oct_segmentation_amd import cleanup
    dev = _need_gpu()
    stack = device_stack(host_planes(), dev)
    for _ in range(args.reps + WARMUP):
        cleanup.clean_stack(stack)
    torch.cuda.synchronize()
    print(json.dumps({'reps': args.reps, 'stack_bytes': int(stack.numel() * 4)}))


def run_compare(args):
    import torch
    from oct_segmentation_amd import cleanup
    dev = _need_gpu()
    planes = host_planes(args.slices)
    n = planes.shape[0]
    stack = device_stack(planes, dev)
    for _ in range(WARMUP):
        cleanup.clean_stack(stack)
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        got = cleanup.clean_stack(stack)
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    out = {'slices': n, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'reps': args.reps, 'stack_bytes': int(stack.numel() * 4),
           'smooth_k': cleanup.smooth_kernel_size(SIZE, SIZE), 'keep': 3, 'fill_holes': True, 'scratch_budget_bytes': cleanup.DEFAULT_SCRATCH,
           'set_pixels_in': int((stack != 0).sum()), 'set_pixels_out': int(got.sum()),
           'clean_stack_events_ms': {'median': round(statistics.median(ev), 3), 'min': round(min(ev), 3), 'max': round(max(ev), 3)},
           'clean_stack_wall_ms': {'median': round(statistics.median(wall), 3), 'min': round(min(wall), 3), 'max': round(max(wall), 3)}}
    # the host comparator, timed once: the copy the device path avoids, then scipy over 16 processes that never touch the GPU
    t0 = time.perf_counter()
    host = stack.cpu().numpy()
    t1 = time.perf_counter()
    jobs = [(np.packbits(host[i, :, :, c] != 0), SIZE) for i in range(n) for c in range(CHANNELS)]
    t2 = time.perf_counter()
    with mp.get_context('spawn').Pool(WORKERS) as pool:
        pool.map(_clean_packed, jobs[:WORKERS])                                    # workers started and their imports done
        t3 = time.perf_counter()
        res = pool.map(_clean_packed, jobs, chunksize=4)
        t4 = time.perf_counter()
    out['host_path'] = {'d2h_stack_s_pageable': round(t1 - t0, 3), 'pack_s': round(t2 - t1, 3), 'scipy_s': round(t4 - t3, 3), 'workers': WORKERS}
    out['host_end_to_end_s'] = round((t1 - t0) + (t2 - t1) + (t4 - t3), 3)
    out['device_faster_end_to_end'] = bool(statistics.median(wall) / 1e3 < out['host_end_to_end_s'])
    equal = True
    for i in range(n):
        want = np.stack([np.unpackbits(res[i * CHANNELS + c])[:SIZE * SIZE].reshape(SIZE, SIZE) for c in range(CHANNELS)], axis=-1)
        equal = equal and bool(torch.equal(got[i], torch.from_numpy(want).to(dev).to(torch.float32)))
    out['equal'] = equal
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not equal:
        raise SystemExit('kernels and host comparator disagree')


def _kernel_rows(prof_dir):
    dbs = sorted(glob.glob(os.path.join(prof_dir, '**', '*.db'), recursive=True), key=os.path.getmtime)
    if dbs:
        try:
            return sqlite3.connect(dbs[-1]).execute('select name, start, end from kernels order by start').fetchall()
        except sqlite3.Error:
            pass
    import csv
    files = sorted(glob.glob(os.path.join(prof_dir, '**', '*kernel_trace.csv'), recursive=True), key=os.path.getmtime)
    if not files:
        raise SystemExit(f'no rocprofv3 .db or kernel_trace.csv under {prof_dir}')
    with open(files[-1], newline='') as f:
        return sorted(((r['Kernel_Name'], int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in csv.DictReader(f)), key=lambda r: r[1])


def run_record(args):
    rows = _kernel_rows(args.prof)
    total = {k: 0.0 for k in KERNELS}
    launches = {k: 0 for k in KERNELS}
    for name, start, end in rows:
        for k in KERNELS:
            if re.search(r'(^|[^a-z_])' + k + r'\b', name):               # a name must not take the launches of one it is the tail of
                total[k] += (end - start) / 1e3
                launches[k] += 1
    calls = args.reps + WARMUP
    rec = {'commit': args.commit, 'device': 'MI355X (gfx950)', 'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS,
           'masks': 'golden demo planes tiled to the frame + salt noise p = 0.002 from a seed (tools/bench_cleanup.py host_planes)',
           'method': 'per kernel: rocprofv3 --kernel-trace in a run of its own, the sum of its launches over all clean_stack calls divided by '
                     'the number of calls (warm-up calls included); measured once',
           'kernel_us_per_clean_stack': {k: round(total[k] / calls, 1) for k in KERNELS if launches[k]},
           'launches_per_clean_stack': {k: launches[k] // calls for k in KERNELS if launches[k]}}
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
    k = sub.add_parser('kernel'); k.add_argument('--reps', type=int, default=5)
    c = sub.add_parser('compare'); c.add_argument('--reps', type=int, default=20); c.add_argument('--slices', type=int, default=N)
    c.add_argument('--out', default=None)
    r = sub.add_parser('record'); r.add_argument('--prof', required=True); r.add_argument('--compare', default=None)
    r.add_argument('--reps', type=int, default=5); r.add_argument('--commit', default='unknown'); r.add_argument('--out', required=True)
    args = ap.parse_args()
    {'kernel': run_kernel, 'compare': run_compare, 'record': run_record}[args.cmd](args)


if __name__ == '__main__':
    main()
