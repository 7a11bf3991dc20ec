"""Measurements of the volume distance calls (csrc/distance.hip, the octseg_volume_* entry points).  Needs an MI355X.

One workload: a 4-class blob volume of 270 x 704 x 704 (each float32 stack is 2.14 GB) at slice_step 10 -- per class the union of three
ellipsoids from a seed as "truth", the same volume rolled by one slice and (3, 5) pixels as "prediction".  The call is what
volume_surface_metrics runs before its numpy: both directed 3-D boundary lists, sorted, with the overlap counts.

  kernel   the call 8 times; run it under the profiler, in a run of its own:
               rocprofv3 --kernel-trace --stats -d out/distance3d_prof -- python tools/bench_distance3d.py kernel
  compare  in ONE process: the call with events around it (median of 5 after 2 warm-up calls), the scratch it used, and the host comparator --
           the device-to-host copy of the stacks, then scipy.ndimage (binary_erosion with the 6-neighbour cross, distance_transform_edt with
           sampling=(10, 1, 1)) per class and direction over 8 worker processes of 2 threads' worth of the 16-CPU share that never touch the
           GPU; checks that both give the same integers:
               python tools/bench_distance3d.py compare --out out/distance3d_compare.json
  record   merge everything under out/ into profiles/distance3d_704.json:
               python tools/bench_distance3d.py record --dir out --commit <id> --out profiles/distance3d_704.json
"""
import argparse
import json
import multiprocessing as mp
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N, SIZE, CHANNELS, STEP = 270, 704, 4, 10
WARMUP, REPS = 2, 5
KERNEL_CALLS = 8
WORKERS = 8
NONE = 0x7fffffff
KERNELS = ('bits_pack_kernel', 'dist_part3_kernel', 'dist_column_band_kernel', 'dist_map_kernel', 'dist_count_kernel', 'dist_count_sum_kernel',
           'dist_query3_kernel')


def volumes(dev, n=N, size=SIZE):
    """(pred, truth) float32 [n, size, size, 4] on the device, made there slice by slice."""
    import torch
    rng = np.random.RandomState(5)
    yy = torch.arange(size, device=dev, dtype=torch.float32).view(size, 1)
    xx = torch.arange(size, device=dev, dtype=torch.float32).view(1, size)
    truth = torch.zeros((n, size, size, CHANNELS), dtype=torch.float32, device=dev)
    for c in range(CHANNELS):
        for _ in range(3):
            cz, cy, cx = rng.uniform(0.2, 0.8) * n, rng.uniform(0.3, 0.7) * size, rng.uniform(0.3, 0.7) * size
            rz, ry, rx = rng.uniform(0.15, 0.4) * n, rng.uniform(0.08, 0.2) * size, rng.uniform(0.08, 0.2) * size
            for z in range(n):
                rest = 1.0 - ((z - cz) / rz) ** 2
                if rest > 0:
                    truth[z, :, :, c] += ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= rest).to(torch.float32)
    truth.clamp_(max=1.0)
    pred = torch.roll(truth, shifts=(1, 3, 5), dims=(0, 1, 2))
    return pred, truth


def run_call(pred, truth):
    from oct_segmentation_amd import distance
    return distance._volume_surface_lists(pred, truth, [(c, c) for c in range(CHANNELS)], STEP)


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_distance3d: no GPU visible; there is nothing to measure without one')
    return torch.device('cuda:0')


def run_kernel(args):
    import torch
    dev = _need_gpu()
    pred, truth = volumes(dev, args.slices)
    for _ in range(KERNEL_CALLS):                    # the record drops the first WARMUP calls
        run_call(pred, truth)
    torch.cuda.synchronize()
    print(json.dumps({'calls': KERNEL_CALLS, 'slices': args.slices}))


# ---- the host comparator: numpy and scipy only, one (class, direction) per job
def _boundary(m):
    from scipy import ndimage
    return m & ~ndimage.binary_erosion(m, ndimage.generate_binary_structure(3, 1), border_value=0)


def _job(job):
    from scipy import ndimage
    shape, a, b = job
    a, b = (np.unpackbits(v)[:int(np.prod(shape))].reshape(shape).astype(bool) for v in (a, b))
    ea, eb = _boundary(a), _boundary(b)
    if not eb.any():
        return np.full((int(ea.sum()),), NONE, np.int64), (int((a & b).sum()), int(a.sum()), int(b.sum()))
    d = ndimage.distance_transform_edt(~eb, sampling=(STEP, 1, 1))
    d = d[ea]
    return np.sort(np.rint(d * d).astype(np.int64)), (int((a & b).sum()), int(a.sum()), int(b.sum()))


def run_compare(args):
    import torch
    from oct_segmentation_amd import distance
    dev = _need_gpu()
    pred, truth = volumes(dev, args.slices)
    n = int(truth.shape[0])
    for _ in range(WARMUP):
        run_call(pred, truth)
    torch.cuda.synchronize()
    ev = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        got = run_call(pred, truth)
        b.record()
        b.synchronize()
        ev.append(a.elapsed_time(b))
    rows, bands, nbytes = distance.volume_bands(n, SIZE, SIZE, CHANNELS, CHANNELS, CHANNELS)
    out = {'slices': n, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'slice_step': STEP, 'reps': REPS, 'stack_bytes_each': int(truth.numel() * 4),
           'call_events_ms': {'median': round(statistics.median(ev), 2), 'min': round(min(ev), 2), 'max': round(max(ev), 2)},
           'scratch': {'budget_bytes': distance.DEFAULT_SCRATCH, 'used_bytes': nbytes, 'band_rows': rows, 'bands': bands}}
    (d_ab, d_ba), (o_ab, o_ba), counts = got
    out['boundary_voxels'] = {'pred': int(o_ab[-1]), 'truth': int(o_ba[-1])}
    if not args.no_host:
        t0 = time.perf_counter()
        hp, ht = pred.cpu().numpy(), truth.cpu().numpy()
        t1 = time.perf_counter()
        shape = hp.shape[:3]
        pk = [[np.packbits(v[..., c] != 0) for c in range(CHANNELS)] for v in (hp, ht)]
        del hp, ht
        t2 = time.perf_counter()
        jobs = [(shape, pk[0][c], pk[1][c]) for c in range(CHANNELS)] + [(shape, pk[1][c], pk[0][c]) for c in range(CHANNELS)]
        with mp.get_context('spawn').Pool(WORKERS) as pool:
            pool.map(abs, range(WORKERS))                                          # workers started
            t3 = time.perf_counter()
            res = pool.map(_job, jobs, chunksize=1)
            t4 = time.perf_counter()
        out['host_path'] = {'d2h_stacks_s_pageable': round(t1 - t0, 2), 'pack_s': round(t2 - t1, 2), 'scipy_s': round(t4 - t3, 2), 'workers': WORKERS}
        out['host_end_to_end_s'] = round((t1 - t0) + (t2 - t1) + (t4 - t3), 2)
        equal = (np.array_equal(d_ab, np.concatenate([r[0] for r in res[:CHANNELS]])) and np.array_equal(d_ba, np.concatenate([r[0] for r in res[CHANNELS:]]))
                 and np.array_equal(np.diff(o_ab), [r[0].size for r in res[:CHANNELS]]) and np.array_equal(counts, np.array([r[1] for r in res[:CHANNELS]])))
        out['equal'] = bool(equal)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not out.get('equal', True):
        raise SystemExit('kernels and host comparator disagree')


def _per_call(prof_dir):
    """Per kernel the median over the calls after the warm-up of the time all its launches of ONE call take, in milliseconds."""
    from bench_cleanup import _kernel_rows
    groups = {k: [] for k in KERNELS + ('other',)}
    for name, start, end in _kernel_rows(prof_dir):
        key = next((k for k in KERNELS if re.search(r'(^|[^a-z_0-9])' + k + r'\b', name)), 'other')
        groups[key].append((end - start) / 1e6)
    out, launches = {}, {}
    for k, durs in groups.items():
        if not durs or len(durs) % KERNEL_CALLS:
            if durs:
                out[k + '_total_ms_all_calls'] = round(sum(durs), 2)
            continue
        per = len(durs) // KERNEL_CALLS
        out[k] = round(statistics.median([sum(durs[i * per:(i + 1) * per]) for i in range(KERNEL_CALLS)][WARMUP:]), 3)
        launches[k] = per
    return out, launches


def run_record(args):
    rec = {'commit': args.commit, 'device': 'MI355X (gfx950)', 'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'slice_step': STEP,
           'measured': 'once',
           'method': f'kernel times: rocprofv3 --kernel-trace in a run of its own, {KERNEL_CALLS} calls, the first {WARMUP} dropped, per kernel the '
                     f'median over the calls of the sum of its launches in one call; call time: events around {REPS} calls after {WARMUP} warm-up '
                     'calls in one process with the host comparator (device-to-host copy + scipy.ndimage over 8 processes), checked equal',
           'workload': 'per class the union of three ellipsoids from a seed as truth; rolled by one slice and (3, 5) pixels as prediction'}
    prof = os.path.join(args.dir, 'distance3d_prof')
    if os.path.isdir(prof):
        rec['kernel_ms_per_call'], rec['launches_per_call'] = _per_call(prof)
    cmp_path = os.path.join(args.dir, 'distance3d_compare.json')
    if os.path.exists(cmp_path):
        with open(cmp_path) as f:
            rec['same_process_comparison'] = json.load(f)
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec, indent=1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    k = sub.add_parser('kernel')
    k.add_argument('--slices', type=int, default=N)
    c = sub.add_parser('compare')
    c.add_argument('--slices', type=int, default=N)
    c.add_argument('--out', default=None)
    c.add_argument('--no-host', action='store_true')
    r = sub.add_parser('record')
    r.add_argument('--dir', required=True)
    r.add_argument('--commit', default='unknown')
    r.add_argument('--out', required=True)
    args = ap.parse_args()
    {'kernel': run_kernel, 'compare': run_compare, 'record': run_record}[args.cmd](args)


if __name__ == '__main__':
    main()
