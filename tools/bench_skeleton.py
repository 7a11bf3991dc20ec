"""Measurements of the thinning and census kernels (csrc/skeleton.hip, oct_segmentation_amd/skeleton.py).  Needs an MI355X.

  kernel   skeleton_stack(with_census=True) at N = 186, 750 x 750, four classes: the filled-ellipse stack of tools/bench_measure.py (1.67 GB;
           744 planes, the lumen ellipses the deep ones); run it under the profiler, in a run of its own:
               rocprofv3 --kernel-trace --stats -d out/skeleton_prof -- python tools/bench_skeleton.py kernel
  compare  in ONE process: events around skeleton_stack(with_census=True), the same on the forced global path, census_stack and
           thickness_report on the same stack (median of 20 after warm-up), and as CONTEXT, not as a bar, the numpy restatement
           tests/skeleton_ref.py timed once on the planes of the first --host-slices slices; checks that both give the same skeletons there:
               python tools/bench_skeleton.py compare --out out/skeleton_compare.json
  record   merge both into profiles/skeleton_186.json:
               python tools/bench_skeleton.py record --prof out/skeleton_prof --compare out/skeleton_compare.json --commit <id> \\
                   --out profiles/skeleton_186.json
"""
import argparse
import json
import os
import re
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
KERNELS = ('bits_pack_kernel', 'skel_thin_lds_kernel', 'skel_thin_global_kernel', 'skel_census_kernel', 'bits_unpack_kernel')


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_skeleton: no GPU visible; there is nothing to measure without one')
    return torch.device('cuda:0')


def _stack(dev, n=N):
    from bench_measure import elliptic_stack
    return elliptic_stack(dev, n, SIZE)


def run_kernel(args):
    import torch
    from oct_segmentation_amd import skeleton
    dev = _need_gpu()
    stack = _stack(dev)
    for _ in range(args.reps + WARMUP):
        skeleton.skeleton_stack(stack, with_census=True, scratch_bytes=args.scratch)
    torch.cuda.synchronize()
    print(json.dumps({'call': 'skeleton_stack(with_census=True)', 'reps': args.reps, 'stack_bytes': int(stack.numel() * 4)}))


def run_compare(args):
    import torch
    import skeleton_ref as R
    from oct_segmentation_amd import _lib as L
    from oct_segmentation_amd import skeleton
    dev = _need_gpu()
    stack = _stack(dev, args.slices)
    n = int(stack.shape[0])
    out = {'slices': n, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'planes': n * CHANNELS, 'reps': args.reps,
           'stack_bytes': int(stack.numel() * 4), 'set_pixels': int((stack != 0).sum()),
           'scratch_bytes': int(L.lib().octseg_skeleton_scratch_bytes(n, SIZE, SIZE, CHANNELS))}
    calls = {'skeleton_census': lambda s: skeleton.skeleton_stack(s, with_census=True, scratch_bytes=args.scratch),
             'skeleton_census_global_path': lambda s: skeleton.skeleton_stack(s, with_census=True, path='global', scratch_bytes=args.scratch),
             'census_only': lambda s: skeleton.census_stack(s, scratch_bytes=args.scratch),
             'thickness_report': lambda s: skeleton.thickness_report(s, scratch_bytes=args.scratch)}
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
    skel, cen = results['skeleton_census']
    cen = cen.cpu().numpy()
    out['paths_equal'] = bool(torch.equal(skel, results['skeleton_census_global_path'][0]) and
                              np.array_equal(cen, results['skeleton_census_global_path'][1].cpu().numpy()))
    out['passes'] = {'max': int(cen[:, :, 5].max()), 'sum': int(cen[:, :, 5].sum()), 'max_per_class': [int(v) for v in cen[:, :, 5].max(axis=0)]}
    out['skeleton_pixels'] = int(cen[:, :, 1].sum())
    # context: the numpy restatement on the first slices, one process, timed once
    k = min(args.host_slices, n)
    host = stack[:k].cpu().numpy()
    t0 = time.perf_counter()
    want, wcen = R.skeleton_stack(host)
    t1 = time.perf_counter()
    out['numpy_restatement'] = {'slices': k, 'planes': k * CHANNELS, 'seconds': round(t1 - t0, 3), 'passes_sum': int(wcen[:, :, 5].sum())}
    equal = bool(np.array_equal(skel[:k].cpu().numpy(), want) and np.array_equal(cen[:k], wcen))
    out['equal'] = equal and out['paths_equal']
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not out['equal']:
        raise SystemExit('kernels and restatement, or the two paths, disagree')


def run_record(args):
    from bench_lesions import _kernel_rows
    calls = args.reps + WARMUP
    rec = {'commit': args.commit, 'device': 'MI355X (gfx950)', 'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS,
           'masks': 'filled ellipses from a seed (tools/bench_measure.py elliptic_stack)',
           'method': 'per kernel: rocprofv3 --kernel-trace in a run of its own, the sum of its launches over all calls divided by the number of '
                     'calls (warm-up calls included); measured once; no counter was collected'}
    if args.prof:
        total = {k: 0.0 for k in KERNELS}
        launches = {k: 0 for k in KERNELS}
        for name, start, end in _kernel_rows(args.prof):
            for k in KERNELS:
                if re.search(r'(^|[^a-z_])' + k + r'\b', name):
                    total[k] += (end - start) / 1e3
                    launches[k] += 1
        rec['kernel_us_per_skeleton_stack'] = {k: round(total[k] / calls, 1) for k in KERNELS if launches[k]}
        rec['launches_per_skeleton_stack'] = {k: launches[k] // calls for k in KERNELS if launches[k]}
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
    k = sub.add_parser('kernel'); k.add_argument('--reps', type=int, default=5); k.add_argument('--scratch', type=int, default=512 << 20)
    c = sub.add_parser('compare'); c.add_argument('--reps', type=int, default=20); c.add_argument('--slices', type=int, default=N)
    c.add_argument('--host-slices', type=int, default=4); c.add_argument('--scratch', type=int, default=512 << 20); c.add_argument('--out', default=None)
    r = sub.add_parser('record'); r.add_argument('--prof', default=None); r.add_argument('--compare', default=None)
    r.add_argument('--reps', type=int, default=5); r.add_argument('--commit', default='unknown'); r.add_argument('--out', required=True)
    args = ap.parse_args()
    {'kernel': run_kernel, 'compare': run_compare, 'record': run_record}[args.cmd](args)


if __name__ == '__main__':
    main()
