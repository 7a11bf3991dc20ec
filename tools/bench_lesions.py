"""Measurements of the 3-D lesion kernels (csrc/lesions.hip, oct_segmentation_amd/lesions.py).  Needs an MI355X.

  kernel   lesion_table(profile=True) or clean_volume(min_slices=2) at N = 186, 750 x 750, four classes: the filled-ellipse stack of
           tools/bench_measure.py (1.67 GB; its sparsity flatters both sides); run it under the profiler, in a run of its own per call:
               rocprofv3 --kernel-trace --stats -d out/lesions_prof_table -- python tools/bench_lesions.py kernel --call table
               rocprofv3 --kernel-trace --stats -d out/lesions_prof_clean -- python tools/bench_lesions.py kernel --call clean
  compare  in ONE process: events around lesion_table, clean_volume, label_volume and cleanup.label_stack on the same stack (median of 20 after
           warm-up; the 3-D labelling does the 2-D labelling's work plus one merge, so their ratio is reported), and the host comparator, timed
           once -- device-to-host copy of the stack, then tests/lesions_ref.py with one worker process per class (four volumes: four of the 16
           CPUs can work) that never touches the GPU; checks that both give the same integers:
               python tools/bench_lesions.py compare --out out/lesions_compare.json
  record   merge all into profiles/lesions_186.json:
               python tools/bench_lesions.py record --prof-table out/lesions_prof_table --prof-clean out/lesions_prof_clean \\
                   --compare out/lesions_compare.json --commit <id> --out profiles/lesions_186.json
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

if os.environ.get('OCTSEG_LIB'):   # an experimental build of the library (timing experiments)
    from oct_segmentation_amd import _lib as _L
    _L.LIB_PATH = os.path.abspath(os.environ['OCTSEG_LIB'])

N, SIZE, CHANNELS = 186, 750, 4
WARMUP = 3
WORKERS = 16
ACROSS = 'overlap'
KERNELS = ('bits_pack_kernel', 'ccl_init_kernel', 'ccl_merge_kernel', 'vol_across_kernel', 'ccl_flatten_kernel', 'vol_count_kernel',
           'vol_select_kernel', 'vol_extent_kernel', 'ccl_keep_kernel', 'bits_unpack_kernel', 'ccl_labels_kernel')


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_lesions: no GPU visible; there is nothing to measure without one')
    return torch.device('cuda:0')


def _stack(dev, n=N):
    from bench_measure import elliptic_stack
    return elliptic_stack(dev, n, SIZE)


def _calls(across):
    from oct_segmentation_amd import cleanup, lesions
    return {'table': lambda s: lesions.lesion_table(s, across=across, profile=True),
            'clean': lambda s: lesions.clean_volume(s, min_slices=2, across=across),
            'label_volume': lambda s: lesions.label_volume(s, across=across),
            'label_stack_2d': lambda s: cleanup.label_stack(s)}


def run_kernel(args):
    import torch
    dev = _need_gpu()
    stack = _stack(dev)
    fn = _calls(args.across)[args.call]
    for _ in range(args.reps + WARMUP):
        fn(stack)
    torch.cuda.synchronize()
    print(json.dumps({'call': args.call, 'across': args.across, 'reps': args.reps, 'stack_bytes': int(stack.numel() * 4)}))


def _analyse_packed(job):
    """Worker: one class's volume as packed bits in; (nles, top, profile, the flicker-filtered volume as packed bits) out (numpy and scipy only)."""
    import lesions_ref as R
    packed, shape, across = job
    vol = np.unpackbits(packed)[:int(np.prod(shape))].reshape(shape)
    _, nles, top, prof = R.analyse(vol, across)
    return nles, top, prof, np.packbits(R.clean(vol, 2, 0, 0, across))


def _warm(_):
    import lesions_ref  # noqa: F401
    return 0


def run_compare(args):
    import torch
    dev = _need_gpu()
    stack = _stack(dev, args.slices)
    n = int(stack.shape[0])
    calls = _calls(args.across)
    out = {'slices': n, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'across': args.across, 'reps': args.reps,
           'stack_bytes': int(stack.numel() * 4), 'set_voxels': int((stack != 0).sum())}
    from oct_segmentation_amd import _lib as L
    out['scratch_bytes'] = int(L.lib().octseg_lesions_scratch_bytes(CHANNELS, n, SIZE, SIZE))
    results = {}
    for name, fn in calls.items():
        for _ in range(WARMUP):
            fn(stack)
        torch.cuda.synchronize()
        ev = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            results[name] = fn(stack)
            b.record()
            b.synchronize()
            ev.append(a.elapsed_time(b))
        out[f'{name}_events_ms'] = {'median': round(statistics.median(ev), 3), 'min': round(min(ev), 3), 'max': round(max(ev), 3)}
        if name.startswith('label'):
            results[name] = None                                                    # 1.67 GB of labels each: not needed below
            torch.cuda.empty_cache()
    out['label_volume_over_label_stack_2d'] = round(out['label_volume_events_ms']['median'] / out['label_stack_2d_events_ms']['median'], 3)
    nles, top, prof = results['table']
    out['nles'] = [int(v) for v in nles.cpu()]
    # the host comparator, timed once: the copy the device path avoids, then scipy, one worker process per class
    t0 = time.perf_counter()
    host = stack.cpu().numpy()
    t1 = time.perf_counter()
    shape = (n, SIZE, SIZE)
    jobs = [(np.packbits(host[..., c] != 0), shape, args.across) for c in range(CHANNELS)]
    t2 = time.perf_counter()
    with mp.get_context('spawn').Pool(min(WORKERS, CHANNELS)) as pool:
        pool.map(_warm, range(CHANNELS))                                            # workers started and their imports done
        t3 = time.perf_counter()
        res = pool.map(_analyse_packed, jobs, chunksize=1)
        t4 = time.perf_counter()
    out['host_path'] = {'d2h_stack_s_pageable': round(t1 - t0, 3), 'pack_s': round(t2 - t1, 3), 'scipy_table_and_clean_s': round(t4 - t3, 3),
                        'workers': min(WORKERS, CHANNELS), 'cpus': WORKERS}
    out['host_end_to_end_s'] = round((t1 - t0) + (t2 - t1) + (t4 - t3), 3)
    equal = True
    cleaned = results['clean']
    for c in range(CHANNELS):
        wn, wt, wp, wclean = res[c]
        equal = equal and int(nles[c]) == wn and np.array_equal(top[c].cpu().numpy(), wt) and np.array_equal(prof[c].cpu().numpy(), wp)
        want = torch.from_numpy(np.unpackbits(wclean)[:n * SIZE * SIZE].reshape(shape)).to(dev).to(torch.float32)
        equal = equal and bool(torch.equal(cleaned[..., c], want))
    out['equal'] = bool(equal)
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
            con = sqlite3.connect(dbs[-1])
            tables = [r[0] for r in con.execute("select name from sqlite_master where type in ('table', 'view')")]
            for t in ('kernels',) + tuple(x for x in tables if x.startswith('kernels')):
                if t in tables:
                    return con.execute(f'select name, start, end from {t} order by start').fetchall()
        except sqlite3.Error:
            pass
    import csv
    files = sorted(glob.glob(os.path.join(prof_dir, '**', '*kernel_trace.csv'), recursive=True), key=os.path.getmtime)
    if not files:
        raise SystemExit(f'no rocprofv3 .db or kernel_trace.csv under {prof_dir}')
    with open(files[-1], newline='') as f:
        return sorted(((r['Kernel_Name'], int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in csv.DictReader(f)), key=lambda r: r[1])


def _per_call(prof_dir, calls):
    total = {k: 0.0 for k in KERNELS}
    launches = {k: 0 for k in KERNELS}
    for name, start, end in _kernel_rows(prof_dir):
        for k in KERNELS:
            if re.search(r'(^|[^a-z_])' + k + r'\b', name):
                total[k] += (end - start) / 1e3
                launches[k] += 1
    return ({k: round(total[k] / calls, 1) for k in KERNELS if launches[k]}, {k: launches[k] // calls for k in KERNELS if launches[k]})


def run_record(args):
    calls = args.reps + WARMUP
    rec = {'commit': args.commit, 'device': 'MI355X (gfx950)', 'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS,
           'masks': 'filled ellipses from a seed (tools/bench_measure.py elliptic_stack); sparse beyond the lumen, which flatters both sides',
           'method': 'per kernel: rocprofv3 --kernel-trace in a run of its own per call, the sum of its launches over all calls divided by the '
                     'number of calls (warm-up calls included); measured once; no counter was collected'}
    for key, prof in (('lesion_table', args.prof_table), ('clean_volume', args.prof_clean)):
        if prof:
            us, launches = _per_call(prof, calls)
            rec[f'kernel_us_per_{key}'] = us
            rec[f'launches_per_{key}'] = launches
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
    k = sub.add_parser('kernel'); k.add_argument('--reps', type=int, default=5); k.add_argument('--across', default=ACROSS)
    k.add_argument('--call', choices=('table', 'clean'), default='table')
    c = sub.add_parser('compare'); c.add_argument('--reps', type=int, default=20); c.add_argument('--slices', type=int, default=N)
    c.add_argument('--across', default=ACROSS); c.add_argument('--out', default=None)
    r = sub.add_parser('record'); r.add_argument('--prof-table', default=None); r.add_argument('--prof-clean', default=None)
    r.add_argument('--compare', default=None); r.add_argument('--reps', type=int, default=5); r.add_argument('--commit', default='unknown')
    r.add_argument('--out', required=True)
    args = ap.parse_args()
    {'kernel': run_kernel, 'compare': run_compare, 'record': run_record}[args.cmd](args)


if __name__ == '__main__':
    main()
