"""Measurements of the contour kernels (csrc/contours.hip, oct_segmentation_amd/contours.py).  Needs an MI355X.  Timing is recorded, not promised.

  kernel   count_stack + trace_stack at N = 186, 704 x 704, four classes: the synthetic vessel masks of tests/synth.py (discs of falling radius
           around the frame centre); run it under the profiler, in a run of its own:
               rocprofv3 --kernel-trace --stats -d out/contours_prof -- python tools/bench_contours.py kernel
  compare  in ONE process: events around count_stack, trace_stack and cleanup.label_stack on the same stack (median of 10 after warm-up; the tracer
           does the labelling's pack / init / merge / flatten and then its own phases, so their ratio is reported), and the sequential crack
           follower of tests/contours_ref.py on the first slices, timed once; checks that both give the same integers:
               python tools/bench_contours.py compare --out out/contours_compare.json
  record   merge both into profiles/contours_704.json:
               python tools/bench_contours.py record --prof out/contours_prof --compare out/contours_compare.json --commit <id> \\
                   --out profiles/contours_704.json
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

if os.environ.get('OCTSEG_LIB'):   # an experimental build of the library (timing experiments)
    from oct_segmentation_amd import _lib as _L
    _L.LIB_PATH = os.path.abspath(os.environ['OCTSEG_LIB'])

N, SIZE, CHANNELS = 186, 704, 4
WARMUP = 2
HOST_SLICES = 4
KERNELS = ('contour_counts_kernel', 'bits_pack_kernel', 'ccl_init_kernel', 'ccl_merge_kernel', 'ccl_flatten_kernel', 'ccl_labels_kernel',
           'scan_sums_kernel', 'scan_partials_kernel', 'scan_tiles_kernel', 'contour_setup_kernel', 'contour_links_kernel', 'contour_jump_kernel',
           'contour_scatter_kernel', 'contour_emit_kernel', 'contour_finish_kernel')


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_contours: no GPU visible; there is nothing to measure without one')
    return torch.device('cuda:0')


def _stack(dev, n=N):
    """float32 [n, SIZE, SIZE, CHANNELS] on the device: synth.make_batch's masks, made 31 slices at a time."""
    import torch
    from synth import make_batch
    parts = []
    for i in range(0, n, 31):
        m = min(31, n - i)
        parts.append(make_batch(m, CHANNELS, SIZE, seed=704 + i)[1].permute(0, 2, 3, 1).contiguous())
    return torch.cat(parts).to(dev)


def _calls():
    from oct_segmentation_amd import cleanup, contours
    return {'count_stack': contours.count_stack, 'trace_stack': contours.trace_stack, 'label_stack': cleanup.label_stack}


def run_kernel(args):
    import torch
    dev = _need_gpu()
    stack = _stack(dev)
    calls = _calls()
    for _ in range(args.reps + WARMUP):
        calls['trace_stack'](stack)                     # (its first step is count_stack)
    torch.cuda.synchronize()
    print(json.dumps({'reps': args.reps, 'stack_bytes': int(stack.numel() * 4)}))


def run_compare(args):
    import torch
    import contours_ref as R
    dev = _need_gpu()
    stack = _stack(dev, args.slices)
    n = int(stack.shape[0])
    out = {'slices': n, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'reps': args.reps, 'stack_bytes': int(stack.numel() * 4),
           'set_pixels': int((stack != 0).sum())}
    results = {}
    for name, fn in _calls().items():
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
        if name == 'label_stack':
            results[name] = None
            torch.cuda.empty_cache()
    out['trace_stack_over_label_stack'] = round(out['trace_stack_events_ms']['median'] / out['label_stack_events_ms']['median'], 3)
    out['note'] = ('trace_stack includes its count_stack call, two host reads and the allocation of its buffers; label_stack is the labelling of '
                   'the clean-up (pack, init, merge, flatten, labels), unchanged by the contour work')
    cont, counts = results['trace_stack'], results['count_stack']
    out['edges'] = int(counts[..., 0].sum())
    out['contours'] = int(cont.table.shape[0])
    out['vertices'] = int(cont.vertices.shape[0])
    out['longest_cycle'] = int(cont.table[:, 4].max()) if cont.table.shape[0] else 0
    m = min(HOST_SLICES, n)
    t0 = time.perf_counter()
    want = R.trace_stack(stack[:m].cpu().numpy())
    out['host_follower'] = {'slices': m, 'seconds': round(time.perf_counter() - t0, 3)}
    k = int(want[1].shape[0])
    equal = (np.array_equal(cont.ncont[:m].cpu().numpy(), want[0]) and np.array_equal(cont.table[:k].cpu().numpy(), want[1])
             and np.array_equal(cont.vertices[:want[2].shape[0]].cpu().numpy(), want[2]) and np.array_equal(counts[:m].cpu().numpy(), want[3]))
    out['equal'] = bool(equal)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not equal:
        raise SystemExit('kernels and host follower disagree')


def _per_call(prof_dir, calls):
    import re
    from bench_lesions import _kernel_rows
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
           'masks': 'tests/synth.py make_batch: one disc per class around the frame centre, radius falling with the class',
           'method': 'per kernel: rocprofv3 --kernel-trace in a run of its own, the sum of its launches over all trace_stack calls divided by the '
                     'number of calls (warm-up calls included); measured once; no counter was collected'}
    if args.prof:
        rec['kernel_us_per_trace_stack'], rec['launches_per_trace_stack'] = _per_call(args.prof, calls)
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
    k = sub.add_parser('kernel'); k.add_argument('--reps', type=int, default=3)
    c = sub.add_parser('compare'); c.add_argument('--reps', type=int, default=10); c.add_argument('--slices', type=int, default=N)
    c.add_argument('--out', default=None)
    r = sub.add_parser('record'); r.add_argument('--prof', default=None); r.add_argument('--compare', default=None)
    r.add_argument('--reps', type=int, default=3); r.add_argument('--commit', default='unknown'); r.add_argument('--out', required=True)
    args = ap.parse_args()
    {'kernel': run_kernel, 'compare': run_compare, 'record': run_record}[args.cmd](args)


if __name__ == '__main__':
    main()
