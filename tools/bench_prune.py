"""Measurements of the centreline pruning and census kernels (csrc/prune.hip, oct_segmentation_amd/skeleton.py).  Needs an MI355X.

  kernel   prune_stack(skeleton, spur=10, trim=20, with_census=True) at N = 186, 750 x 750, four classes: the skeleton of the filled-ellipse
           stack of tools/bench_measure.py (744 planes), thinned once outside the measured calls; run it under the profiler, in a run of its own:
               rocprofv3 --kernel-trace --stats -d out/prune_prof -- python tools/bench_prune.py kernel
  compare  in ONE process: events around that call, the same on the forced global path, and as CONTEXT thickness_report with and without
           pruning on the same stack (median of 20 after 3 warm-ups), and the numpy restatement tests/prune_ref.py timed once on the planes of
           the first --host-slices slices; checks that both give the same planes and census there:
               python tools/bench_prune.py compare --out out/prune_compare.json
  record   merge both into profiles/prune_186.json:
               python tools/bench_prune.py record --prof out/prune_prof --compare out/prune_compare.json --commit <id> --out profiles/prune_186.json
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
SPUR, TRIM = 10, 20
WARMUP = 3
KERNELS = ('bits_pack_kernel', 'prune_lds_kernel', 'prune_global_kernel', 'prune_census_kernel', 'bits_unpack_kernel')


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_prune: no GPU visible; there is nothing to measure without one')
    return torch.device('cuda:0')


def _stack(dev, n=N):
    from bench_measure import elliptic_stack
    return elliptic_stack(dev, n, SIZE)


def run_kernel(args):
    import torch
    from oct_segmentation_amd import skeleton
    dev = _need_gpu()
    skel = skeleton.skeleton_stack(_stack(dev), scratch_bytes=args.scratch)
    for _ in range(args.reps + WARMUP):
        skeleton.prune_stack(skel, SPUR, TRIM, with_census=True, scratch_bytes=args.scratch)
    torch.cuda.synchronize()
    print(json.dumps({'call': f'prune_stack(skeleton, spur={SPUR}, trim={TRIM}, with_census=True)', 'reps': args.reps,
                      'stack_bytes': int(skel.numel() * 4)}))


def run_compare(args):
    import torch
    import prune_ref as P
    from oct_segmentation_amd import _lib as L
    from oct_segmentation_amd import skeleton
    dev = _need_gpu()
    stack = _stack(dev, args.slices)
    skel = skeleton.skeleton_stack(stack, scratch_bytes=args.scratch)
    n = int(stack.shape[0])
    out = {'slices': n, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'planes': n * CHANNELS, 'reps': args.reps, 'warmup': WARMUP,
           'spur': SPUR, 'trim': TRIM, 'stack_bytes': int(stack.numel() * 4), 'skeleton_pixels': int((skel != 0).sum()),
           'scratch_bytes': int(L.lib().octseg_prune_scratch_bytes(n, SIZE, SIZE, CHANNELS))}
    calls = {'prune_census': lambda: skeleton.prune_stack(skel, SPUR, TRIM, with_census=True, scratch_bytes=args.scratch),
             'prune_census_global_path': lambda: skeleton.prune_stack(skel, SPUR, TRIM, with_census=True, path='global', scratch_bytes=args.scratch),
             'thickness_report': lambda: skeleton.thickness_report(stack, scratch_bytes=args.scratch),
             'thickness_report_pruned': lambda: skeleton.thickness_report(stack, scratch_bytes=args.scratch, spur=SPUR, trim=TRIM)}
    results = {}
    for name, fn in calls.items():
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        ev = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            results[name] = fn()
            b.record()
            b.synchronize()
            ev.append(a.elapsed_time(b))
        out[f'{name}_events_ms'] = {'median': round(statistics.median(ev), 3), 'min': round(min(ev), 3), 'max': round(max(ev), 3)}
    cut, cen = results['prune_census']
    cen = cen.cpu().numpy()
    out['paths_equal'] = bool(torch.equal(cut, results['prune_census_global_path'][0]) and
                              np.array_equal(cen, results['prune_census_global_path'][1].cpu().numpy()))
    out['census_sums'] = {k: int(cen[:, :, i].sum()) for i, k in enumerate(skeleton.PRUNE_COLUMNS)}
    out['length_sum_px'] = round(float(skeleton.centreline_length(cen).sum()), 3)
    # context: the numpy restatement on the first slices, one process, timed once
    k = min(args.host_slices, n)
    host = skel[:k].cpu().numpy()
    t0 = time.perf_counter()
    want, wcen = P.prune_stack(host, SPUR, TRIM)
    t1 = time.perf_counter()
    out['numpy_restatement'] = {'slices': k, 'planes': k * CHANNELS, 'seconds': round(t1 - t0, 3)}
    equal = bool(np.array_equal(cut[:k].cpu().numpy(), want) and np.array_equal(cen[:k], wcen))
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
           'masks': 'the skeletons of filled ellipses from a seed (tools/bench_measure.py elliptic_stack, skeleton_stack)',
           'call': f'prune_stack(skeleton, spur={SPUR}, trim={TRIM}, with_census=True)',
           'method': 'per kernel: rocprofv3 --kernel-trace --stats in a run of its own, the mean over its launches (one per prune_stack call, '
                     'warm-up calls included; bits_pack_kernel and bits_unpack_kernel also count the one skeleton_stack call that prepares the '
                     'input, a launch of the same size); call times: HIP events, median of 20 after 3 warm-ups, one process; measured once; no '
                     'counter was collected; the parent commit has no such call, so there is no threshold'}
    if args.prof:
        total = {k: 0.0 for k in KERNELS}
        launches = {k: 0 for k in KERNELS}
        for name, start, end in _kernel_rows(args.prof):
            for k in KERNELS:
                if re.search(r'(^|[^a-z_])' + k + r'\b', name):
                    total[k] += (end - start) / 1e3
                    launches[k] += 1
        # every kernel is launched once per prune_stack call; the thinning that prepares the input adds one pack and one unpack of the same size
        rec['kernel_us_per_prune_stack'] = {k: round(total[k] / launches[k], 1) for k in KERNELS if launches[k]}
        rec['launches_in_the_run'] = {k: launches[k] for k in KERNELS if launches[k]}
        rec['prune_stack_calls_in_the_run'] = calls
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
