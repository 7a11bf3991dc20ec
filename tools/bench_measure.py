"""Measurements of the pullback-measurement kernels (csrc/measure.hip, oct_segmentation_amd/analysis.py).  Needs an MI355X.

  kernel   octseg_stack_measure at N = 186, 750 x 750, four classes (the size of the reference's demo pullback; the float32 stack is 1.67 GB),
           filled-ellipse masks from a seed; run it under the profiler, in a run of its own:
               rocprofv3 --kernel-trace --stats -d out/measure_prof -- python tools/bench_measure.py kernel
  compare  in ONE process: the call with events (clear + both kernels), analyze_stack end to end, and the host path for the record --
           device-to-host copy of the stack plus tests/analysis_ref.py on the CPU share of the box, timed once; checks that both agree:
               python tools/bench_measure.py compare --out out/measure_compare.json
  record   merge both into profiles/measure_750.json:
               python tools/bench_measure.py record --prof out/measure_prof --compare out/measure_compare.json --commit <id> \\
                   --out profiles/measure_750.json
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

N, SIZE, CHANNELS = 186, 750, 4
HBM_ACHIEVABLE_TBS = 6.3
WARMUP = 3


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_measure: no GPU visible; there is nothing to measure without one')
    return torch.device('cuda:0')


def ellipse_params(n=N, size=SIZE, seed=186):
    """Per slice and class (present, cy, cx, ry, rx): a lumen around the centre in every slice, a cap and a core beside it in runs, a small
    vasa vasorum now and then -- the shape of the demo pullback, from a seed."""
    rng = np.random.default_rng(seed)
    s = size / 750.0
    p = np.zeros((n, CHANNELS, 5))
    run = np.zeros(CHANNELS, bool)
    for i in range(n):
        for c, (cy, cx, ry, rx, jit, p_on, p_off) in enumerate([(375, 375, 150, 170, 25, 1.0, 0.0), (300, 470, 70, 110, 30, 0.15, 0.25),
                                                                (430, 290, 60, 45, 30, 0.15, 0.25), (110, 620, 22, 15, 60, 0.2, 0.9)]):
            run[c] = (rng.random() < p_on) if not run[c] else (rng.random() >= p_off)
            j = rng.uniform(-jit, jit, 2)
            g = rng.uniform(0.8, 1.2, 2)
            p[i, c] = (run[c], (cy + j[0]) * s, (cx + j[1]) * s, ry * g[0] * s, rx * g[1] * s)
    return p


def elliptic_stack(dev, n=N, size=SIZE):
    """float32 [n, size, size, 4] of 0 / 1 on the device (made there slice by slice: the host never holds the 1.67 GB)."""
    import torch
    p = torch.from_numpy(ellipse_params(n, size)).to(dev)
    yy = torch.arange(size, device=dev, dtype=torch.float64).view(size, 1, 1)
    xx = torch.arange(size, device=dev, dtype=torch.float64).view(1, size, 1)
    stack = torch.empty((n, size, size, CHANNELS), dtype=torch.float32, device=dev)
    for i in range(n):
        on, cy, cx, ry, rx = (p[i, :, k].view(1, 1, CHANNELS) for k in range(5))
        stack[i] = ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0) & (on > 0)).to(torch.float32)
    return stack


def stack_bytes(n=N, size=SIZE):
    return n * size * size * CHANNELS * 4


def table_bytes(size=SIZE):
    from oct_segmentation_amd import analysis
    pix, length = analysis.ray_table(size, size)
    return int(pix.nbytes + length.nbytes)


def run_kernel(args):
    import torch
    from oct_segmentation_amd import analysis
    dev = _need_gpu()
    stack = elliptic_stack(dev)
    for _ in range(args.reps + WARMUP):            # the record drops the first WARMUP calls (code-object load, cold caches)
        analysis.measure_stack(stack)
    torch.cuda.synchronize()
    print(json.dumps({'reps': args.reps, 'stack_bytes': stack_bytes()}))


def _events_ms(fn, reps, warmup=WARMUP):
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
    import analysis_ref as R
    from oct_segmentation_amd import analysis
    dev = _need_gpu()
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    stack = elliptic_stack(dev)
    names = [f'{i:03d}' for i in range(N)]
    t = _events_ms(lambda: analysis.measure_stack(stack), args.reps)
    out = {'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'reps': args.reps, 'stack_bytes': stack_bytes(),
           'measure_stack_events_ms': {'median': round(statistics.median(t), 4), 'min': round(min(t), 4), 'max': round(max(t), 4)}}
    analysis.analyze_stack(stack, names)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    data = analysis.analyze_stack(stack, names)
    out['analyze_stack_s'] = round(time.perf_counter() - t0, 4)
    out['present_slice_classes'] = sum(len(o['slice']) for o in data['objects'].values())
    # the host path, for the record only, timed once: the copy the device path avoids, then the numpy restatement of the kernel
    t0 = time.perf_counter()
    host = stack.cpu().numpy()
    t1 = time.perf_counter()
    counts, radii = R.measure(host)
    t2 = time.perf_counter()
    want = analysis.build_analysis(counts, radii, SIZE, SIZE, names)
    out['host_path'] = {'d2h_stack_s_pageable': round(t1 - t0, 3), 'restatement_numpy_s': round(t2 - t1, 3), 'cpu_threads': torch.get_num_threads()}
    got_counts, got_radii = analysis.measure_stack(stack)
    out['equal'] = bool(np.array_equal(got_counts.cpu().numpy(), counts) and np.array_equal(got_radii.cpu().numpy(), radii) and data == want)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not out['equal']:
        raise SystemExit('kernel and host restatement disagree')


def _kernel_times(prof_dir):
    """{kernel: durations in microseconds, in launch order} of the two measure kernels, from rocprofv3's database or its kernel-trace csv."""
    dbs = sorted(glob.glob(os.path.join(prof_dir, '**', '*.db'), recursive=True), key=os.path.getmtime)
    rows = None
    if dbs:
        try:
            rows = sqlite3.connect(dbs[-1]).execute('select name, start, end from kernels order by start').fetchall()
        except sqlite3.Error:
            rows = None
    if rows is None:
        import csv
        files = sorted(glob.glob(os.path.join(prof_dir, '**', '*kernel_trace.csv'), recursive=True), key=os.path.getmtime)
        if not files:
            raise SystemExit(f'no rocprofv3 .db or kernel_trace.csv under {prof_dir}')
        with open(files[-1], newline='') as f:
            rows = sorted(((r['Kernel_Name'], int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in csv.DictReader(f)), key=lambda r: r[1])
    out = {'count_kernel': [], 'ray_kernel': []}
    for name, start, end in rows:
        for k in out:
            if k in name:
                out[k].append((end - start) / 1e3)
    return out


def run_record(args):
    us = _kernel_times(args.prof)
    nbytes, tbytes = stack_bytes(), table_bytes()
    rec = {'commit': args.commit, 'device': 'MI355X (gfx950)', 'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS,
           'masks': 'filled ellipses from a seed (tools/bench_measure.py elliptic_stack)',
           'method': f'kernel times: rocprofv3 --kernel-trace --stats in a run of its own, first {WARMUP} calls dropped, median of the rest; '
                     'bytes from the shapes; TB/s = bytes / median time',
           'hbm_achievable_tbs': HBM_ACHIEVABLE_TBS, 'stack_bytes': nbytes, 'ray_table_bytes': tbytes, 'kernel': {}}
    for k, t in us.items():
        t = t[WARMUP:]
        if not t:
            raise SystemExit(f'no {k} launches in {args.prof}')
        med = statistics.median(t)
        rec['kernel'][k] = {'calls': len(t), 'median_us': round(med, 2), 'min_us': round(min(t), 2), 'max_us': round(max(t), 2)}
        if k == 'count_kernel':
            floor = nbytes / HBM_ACHIEVABLE_TBS / 1e6
            rec['kernel'][k].update({'bytes': nbytes, 'tb_per_s': round(nbytes / med / 1e6, 3), 'floor_us_at_achievable_hbm': round(floor, 2),
                                     'time_over_floor': round(med / floor, 3)})
        else:
            rec['kernel'][k].update({'waves': N * 360, 'samples_upper_bound': N * int(tbytes - 1440) // 4,
                                     'note': 'gathers of 16 B per sample; the samples actually read depend on where the rays resolve'})
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
    c = sub.add_parser('compare'); c.add_argument('--reps', type=int, default=20); c.add_argument('--out', default=None)
    r = sub.add_parser('record'); r.add_argument('--prof', required=True); r.add_argument('--compare', default=None)
    r.add_argument('--commit', default='unknown'); r.add_argument('--out', required=True)
    args = ap.parse_args()
    {'kernel': run_kernel, 'compare': run_compare, 'record': run_record}[args.cmd](args)


if __name__ == '__main__':
    main()
