"""Measurements of the slice interpolation (csrc/distance.hip's signed maps and blend, oct_segmentation_amd/interp.py).  Needs an MI355X.

  compare  in ONE process, on the N = 186, 750 x 750, four-class filled-ellipse stack of tools/bench_measure.py (1.67 GB; its sparsity flatters
           both sides): events around signed_distance_stack, bridge_gaps with every fifth slice rejected (frames 2, 7, 12, ...; max_gap = 1) and
           resample_stack(factor=4), median of 20 after warm-up; then the host comparator, timed once -- device-to-host copy of the stack, then
           tests/interp_ref.py over 16 worker processes that never touch the GPU, each on a run of consecutive key slices; checks that both
           give the same integers and bits:
               python tools/bench_interp.py compare --out out/interp_compare.json
  record   into profiles/interp_186.json:
               python tools/bench_interp.py record --compare out/interp_compare.json --commit <id> --out profiles/interp_186.json

No counter is collected and no share of a peak is claimed.
"""
import argparse
import json
import multiprocessing as mp
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

N, SIZE, CHANNELS = 186, 750, 4
WARMUP = 3
WORKERS = 16
FACTOR = 4


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_interp: no GPU visible; there is nothing to measure without one')
    return torch.device('cuda:0')


def _frames(n):
    return list(range(2, n - 1, 5))


def _warm(_):
    import interp_ref  # noqa: F401
    return 0


def _host_job(job):
    """Worker: key slices first .. last (inclusive) as packed bits in; their signed maps (int32) and the resampled slices first * FACTOR ..
    last * FACTOR - 1 (+ the last key when it ends the stack), packed."""
    import interp_ref as R
    packed, shape, first, n = job
    st = np.unpackbits(packed)[:int(np.prod(shape))].reshape(shape).astype(bool)
    sd2 = R.sd2_stack(st)
    res = []
    for i in range(shape[0] - 1):
        res.append(st[i])
        for j in range(1, FACTOR):
            res.append(np.stack([R.blend(sd2[i, c], sd2[i + 1, c], FACTOR - j, j) for c in range(shape[3])], axis=-1))
    if first + shape[0] - 1 == n - 1:
        res.append(st[-1])
    return first, sd2.astype(np.int32), np.packbits(np.stack(res))


def _blend_job(job):
    """Worker: one plan row's two maps and weights in; the plane made, packed."""
    import interp_ref as R
    a, b, wa, wb = job
    return np.packbits(R.blend(a, b, wa, wb))


def run_compare(args):
    import torch
    from bench_measure import elliptic_stack
    from oct_segmentation_amd import _lib as L
    from oct_segmentation_amd import interp
    import interp_ref as R
    dev = _need_gpu()
    stack = elliptic_stack(dev, args.slices, SIZE)
    n = int(stack.shape[0])
    frames = _frames(n)
    calls = {'signed_distance_stack': lambda s: interp.signed_distance_stack(s),
             'bridge_gaps': lambda s: interp.bridge_gaps(s, max_gap=1, frames=frames, return_plan=True),
             'resample_stack': lambda s: interp.resample_stack(s, FACTOR)}
    out = {'slices': n, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'reps': args.reps, 'warmup': WARMUP, 'factor': FACTOR,
           'rejected_frames': len(frames), 'stack_bytes': int(stack.numel() * 4), 'set_pixels': int((stack != 0).sum()),
           'scratch_bytes_whole_stack': int(L.lib().octseg_signed_distance_scratch_bytes(n, SIZE, SIZE, CHANNELS)),
           'scratch_budget': int(interp.DEFAULT_SCRATCH)}
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
        torch.cuda.empty_cache()
    bridged, plan, made = results['bridge_gaps']
    out['plan_rows'] = int(plan.shape[0])
    out['pixels_made'] = int(made.sum())
    # the host comparator, timed once: the copy the device path avoids, then scipy over the worker processes
    t0 = time.perf_counter()
    host = stack.cpu().numpy() != 0
    t1 = time.perf_counter()
    per = -(-(n - 1) // WORKERS)
    jobs = []
    for first in range(0, n - 1, per):
        last = min(first + per, n - 1)
        part = host[first:last + 1]
        jobs.append((np.packbits(part), part.shape, first, n))
    t2 = time.perf_counter()
    with mp.get_context('spawn').Pool(min(WORKERS, len(jobs))) as pool:
        pool.map(_warm, range(WORKERS))                                             # workers started and their imports done
        t3 = time.perf_counter()
        res = pool.map(_host_job, jobs, chunksize=1)
        maps = np.empty((n, CHANNELS, SIZE, SIZE), np.int32)
        for first, part, _ in res:
            maps[first:first + part.shape[0]] = part
        want_plan = R.gap_plan(host.any(axis=(1, 2)), 1, frames)
        planes = pool.map(_blend_job, [(maps[lo, c], maps[hi, c], wa, wb) for c, _, lo, hi, wa, wb in want_plan.tolist()], chunksize=4)
        t4 = time.perf_counter()
    out['host_path'] = {'d2h_stack_s_pageable': round(t1 - t0, 3), 'pack_s': round(t2 - t1, 3), 'scipy_maps_bridge_and_resample_s': round(t4 - t3, 3),
                        'workers': min(WORKERS, len(jobs)), 'cpus': WORKERS,
                        'note': 'one pass makes the signed maps once and takes all three results from them (the maps travel back from the '
                                'workers); the device calls each make their own'}
    out['host_end_to_end_s'] = round((t1 - t0) + (t2 - t1) + (t4 - t3), 3)
    equal = np.array_equal(plan, want_plan)
    sd2 = results['signed_distance_stack']
    dense = results['resample_stack']
    pixels = 0
    for (c, o, *_), bits in zip(want_plan.tolist(), planes):
        plane = torch.from_numpy(np.unpackbits(bits)[:SIZE * SIZE].reshape(SIZE, SIZE)).to(dev).to(torch.float32)
        equal = equal and bool(torch.equal(bridged[o, :, :, c], plane))
        pixels += int(plane.sum())
    for first, want_sd2, want_dense in res:
        k = want_sd2.shape[0]
        equal = equal and bool(torch.equal(sd2[first:first + k], torch.from_numpy(want_sd2).to(dev)))
        lo = first * FACTOR
        count = (k - 1) * FACTOR + (1 if first + k - 1 == n - 1 else 0)
        want = torch.from_numpy(np.unpackbits(want_dense)[:count * SIZE * SIZE * CHANNELS].reshape(count, SIZE, SIZE, CHANNELS)).to(dev)
        equal = equal and bool(torch.equal(dense[lo:lo + count], want.to(torch.float32)))
    equal = equal and pixels == out['pixels_made'] and int(dense.shape[0]) == (n - 1) * FACTOR + 1
    out['equal'] = bool(equal)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not equal:
        raise SystemExit('kernels and host comparator disagree')


def run_record(args):
    rec = {'commit': args.commit, 'device': 'MI355X (gfx950)', 'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS,
           'masks': 'filled ellipses from a seed (tools/bench_measure.py elliptic_stack); sparse beyond the lumen, which flatters both sides',
           'method': 'events around each call in one process, median of the repetitions after warm-up; the host comparator timed once; '
                     'no kernel trace and no counter was collected', 'runs': args.runs}
    with open(args.compare) as f:
        rec['same_process_comparison'] = json.load(f)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec, indent=1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    c = sub.add_parser('compare'); c.add_argument('--reps', type=int, default=20); c.add_argument('--slices', type=int, default=N)
    c.add_argument('--out', default=None)
    r = sub.add_parser('record'); r.add_argument('--compare', required=True); r.add_argument('--commit', default='unknown')
    r.add_argument('--runs', type=int, default=1); r.add_argument('--out', required=True)
    args = ap.parse_args()
    {'compare': run_compare, 'record': run_record}[args.cmd](args)


if __name__ == '__main__':
    main()
