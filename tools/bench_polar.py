"""Measurements of the polar profile kernels (csrc/polar.hip, oct_segmentation_amd/polar.py).  Needs an MI355X.

  kernel   octseg_stack_polar without and with the label map, and octseg_stack_measure on the same stack, at N = 186, 750 x 750, four classes
           (the workload of tools/bench_measure.py: filled-ellipse masks from a seed); run it under the profiler, in a run of its own:
               rocprofv3 --kernel-trace --stats -d out/polar_prof -- python tools/bench_polar.py kernel
  compare  in ONE process: the calls with events around them (median of 20 after warm-up), plaque_report end to end, the yardsticks --
           octseg_stack_measure on the same stack (its early-exit walk is the floor a full-length walk is compared with) and the host
           comparator on the CPU share of the box, timed once: device-to-host copy of the stack plus tests/polar_ref.py; checks that all agree:
               python tools/bench_polar.py compare --out out/polar_compare.json
  record   merge both into profiles/polar_186.json:
               python tools/bench_polar.py record --prof out/polar_prof --compare out/polar_compare.json --commit <id> \\
                   --out profiles/polar_186.json
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import bench_measure as BM  # noqa: E402

N, SIZE, CHANNELS, WARMUP = BM.N, BM.SIZE, BM.CHANNELS, BM.WARMUP


def run_kernel(args):
    """reps + WARMUP calls each of: the profile without the map, the profile with it, measure_stack -- in that order, so the record can tell
    the two halves of the profile_kernel launches apart."""
    import torch
    from oct_segmentation_amd import analysis, polar
    dev = BM._need_gpu()
    stack = BM.elliptic_stack(dev)
    for fn in (lambda: polar.polar_profile(stack), lambda: polar.polar_profile(stack, want_map=True), lambda: analysis.measure_stack(stack)):
        for _ in range(args.reps + WARMUP):
            fn()
        torch.cuda.synchronize()
    print(json.dumps({'reps': args.reps, 'stack_bytes': BM.stack_bytes()}))


def _stats(t):
    return {'median': round(statistics.median(t), 4), 'min': round(min(t), 4), 'max': round(max(t), 4)}


def run_compare(args):
    import torch
    import polar_ref as P
    from oct_segmentation_amd import analysis, polar
    dev = BM._need_gpu()
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    stack = BM.elliptic_stack(dev)
    names = [f'{i:03d}' for i in range(N)]
    out = {'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'reps': args.reps, 'stack_bytes': BM.stack_bytes(),
           'polar_profile_events_ms': _stats(BM._events_ms(lambda: polar.polar_profile(stack), args.reps)),
           'polar_profile_with_map_events_ms': _stats(BM._events_ms(lambda: polar.polar_profile(stack, want_map=True), args.reps)),
           'measure_stack_events_ms': _stats(BM._events_ms(lambda: analysis.measure_stack(stack), args.reps))}
    polar.plaque_report(stack, names)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    report = polar.plaque_report(stack, names)
    out['plaque_report_s'] = round(time.perf_counter() - t0, 4)
    prof, labels = polar.polar_profile(stack, want_map=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prof_host = prof.cpu().numpy()
    out['d2h_prof_s'] = round(time.perf_counter() - t0, 5)
    out['prof_bytes'] = int(prof_host.nbytes)
    out['map_bytes'] = int(labels.numel())
    out['cap_over_lipid_slices'] = len(report['cap_over_lipid']['slice'])
    # the host comparator, timed once: the copy the device path avoids, then the numpy restatement of the kernel
    t0 = time.perf_counter()
    host = stack.cpu().numpy()
    t1 = time.perf_counter()
    want, want_map = P.profile(host)
    t2 = time.perf_counter()
    out['host_path'] = {'d2h_stack_s_pageable': round(t1 - t0, 3), 'restatement_numpy_s': round(t2 - t1, 3), 'cpu_threads': torch.get_num_threads()}
    _, radii = analysis.measure_stack(stack)
    out['equal'] = bool(np.array_equal(prof_host, want) and np.array_equal(labels.cpu().numpy(), want_map)
                        and np.array_equal(radii.cpu().numpy(), want[..., 1]) and report == polar.build_report(want, SIZE, names))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not out['equal']:
        raise SystemExit('kernel and host restatement disagree')


def _kernel_rows(prof_dir):
    """(name, microseconds) of every kernel launch in start order, from rocprofv3's database or its kernel-trace csv."""
    import glob
    import sqlite3
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
    return [(name, (end - start) / 1e3) for name, start, end in rows]


def run_record(args):
    rows = _kernel_rows(args.prof)
    prof_us = [us for name, us in rows if 'profile_kernel' in name]
    if len(prof_us) % 2 or not prof_us:
        raise SystemExit(f'{len(prof_us)} profile_kernel launches in {args.prof}: expected two equal halves (without and with the map)')
    half = len(prof_us) // 2
    groups = {'profile_kernel': prof_us[:half], 'profile_kernel_with_map': prof_us[half:],
              'ray_kernel': [us for name, us in rows if 'ray_kernel' in name], 'count_kernel': [us for name, us in rows if 'count_kernel' in name]}
    tbytes = BM.table_bytes()
    rec = {'commit': args.commit, 'device': 'MI355X (gfx950)', 'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS,
           'masks': 'filled ellipses from a seed (tools/bench_measure.py elliptic_stack)',
           'method': f'kernel times: rocprofv3 --kernel-trace --stats in a run of its own, first {WARMUP} calls of each group dropped, median of '
                     'the rest; call times: HIP events around the call in one process, median after warm-up; measured once',
           'stack_bytes': BM.stack_bytes(), 'ray_table_bytes': tbytes, 'samples_per_slice': int(tbytes - 1440) // 4, 'kernel': {}}
    for k, t in groups.items():
        t = t[WARMUP:]
        if not t:
            raise SystemExit(f'no {k} launches in {args.prof}')
        rec['kernel'][k] = {'calls': len(t), 'median_us': round(statistics.median(t), 2), 'min_us': round(min(t), 2), 'max_us': round(max(t), 2)}
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
