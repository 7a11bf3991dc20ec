"""Measurements of the boundary-distance kernels (csrc/distance.hip, oct_segmentation_amd/distance.py).  Needs an MI355X.

Two workloads at N = 186, 750 x 750, four classes (each float32 stack is 1.67 GB):
  A  the filled-ellipse stack of tools/bench_measure.py as "truth" and the same stack shifted by (3, 5) pixels as "prediction";
  B  the adversarial case of the row search: one set pixel per plane, truth in the top-left corner and prediction in the bottom-right one.
Two calls: `surface` = surface_metrics(pred, truth) (both directed boundary lists, sorted, and the host statistics) and `map` =
distance_stack(truth, to='boundary') (the full squared-distance map, where every pixel of workload B searches its whole row).

  kernel   one call 23 times; run it under the profiler, in a run of its own:
               rocprofv3 --kernel-trace --stats -d out/distance_prof_A_surface -- python tools/bench_distance.py kernel --workload A --call surface
  compare  in ONE process: the call with events around it (median of 20 after 3 warm-up calls) and as wall time, and the host comparator -- the
           device-to-host copy of the stacks, then scipy.ndimage plane by plane over 16 worker processes that never touch the GPU; checks that
           both give the same integers:
               python tools/bench_distance.py compare --workload A --call surface --out out/distance_compare_A_surface.json
  record   merge everything under out/ into profiles/distance_750.json:
               python tools/bench_distance.py record --dir out --commit <id> --out profiles/distance_750.json
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

if os.environ.get('OCTSEG_LIB'):   # an experimental build of the library (timing experiments)
    from oct_segmentation_amd import _lib as _L
    _L.LIB_PATH = os.path.abspath(os.environ['OCTSEG_LIB'])

N, SIZE, CHANNELS = 186, 750, 4
HBM_ACHIEVABLE_TBS = 6.3
WARMUP, REPS = 3, 20
WORKERS = 16
NONE = 0x7fffffff
KERNELS = ('bits_pack_kernel', 'bits_unpack_kernel', 'dist_part_kernel', 'dist_column_kernel', 'dist_map_kernel', 'dist_count_kernel',
           'dist_query_kernel')


def stacks(workload, dev, n=N):
    """(pred, truth) float32 [n, 750, 750, 4] on the device."""
    import torch
    from bench_measure import elliptic_stack
    if workload == 'A':
        truth = elliptic_stack(dev, n, SIZE)
        pred = torch.roll(truth, shifts=(3, 5), dims=(1, 2))
        pred[:, :3] = 0
        pred[:, :, :5] = 0
        return pred, truth
    truth = torch.zeros((n, SIZE, SIZE, CHANNELS), dtype=torch.float32, device=dev)
    pred = torch.zeros_like(truth)
    truth[:, 0, 0, :] = 1
    pred[:, SIZE - 1, SIZE - 1, :] = 1
    return pred, truth


def run_call(call, pred, truth):
    from oct_segmentation_amd import distance
    if call == 'surface':
        return distance._surface_lists(pred, truth, [(c, c) for c in range(CHANNELS)])
    return distance.distance_stack(truth, to='boundary')


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_distance: no GPU visible; there is nothing to measure without one')
    return torch.device('cuda:0')


def run_kernel(args):
    import torch
    dev = _need_gpu()
    pred, truth = stacks(args.workload, dev)
    for _ in range(REPS + WARMUP):                  # the record drops the first WARMUP calls (code-object load, cold caches)
        run_call(args.call, pred, truth)
    torch.cuda.synchronize()
    print(json.dumps({'workload': args.workload, 'call': args.call, 'calls': REPS + WARMUP}))


# ---- the host comparator: numpy and scipy only, one plane (pair) per job
def _boundary(m):
    from scipy import ndimage
    return m & ~ndimage.binary_erosion(m, ndimage.generate_binary_structure(2, 1), border_value=0)


def _edt2(target):
    from scipy import ndimage
    if not target.any():
        return np.full(target.shape, NONE, np.int64)
    d = ndimage.distance_transform_edt(~target)
    return np.rint(d * d).astype(np.int64)


def _unpack(packed):
    return np.unpackbits(packed)[:SIZE * SIZE].reshape(SIZE, SIZE).astype(bool)


def _surface_job(job):
    a, b = _unpack(job[0]), _unpack(job[1])
    ea, eb = _boundary(a), _boundary(b)
    return (np.sort(_edt2(eb)[ea]), np.sort(_edt2(ea)[eb]), (int((a & b).sum()), int(a.sum()), int(b.sum())))


def _map_job(job):
    return _edt2(_boundary(_unpack(job[1]))).astype(np.int32)


def run_compare(args):
    import torch
    dev = _need_gpu()
    pred, truth = stacks(args.workload, dev, args.slices)
    n = int(truth.shape[0])
    for _ in range(WARMUP):
        run_call(args.call, pred, truth)
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        got = run_call(args.call, pred, truth)
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    out = {'workload': args.workload, 'call': args.call, 'slices': n, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'reps': REPS,
           'stack_bytes_each': int(truth.numel() * 4),
           'call_events_ms': {'median': round(statistics.median(ev), 3), 'min': round(min(ev), 3), 'max': round(max(ev), 3)},
           'call_wall_ms': {'median': round(statistics.median(wall), 3), 'min': round(min(wall), 3), 'max': round(max(wall), 3)}}
    # the host comparator, timed once: the copies the device path avoids, then scipy over 16 processes that never touch the GPU
    t0 = time.perf_counter()
    hp, ht = (pred.cpu().numpy() if args.call == 'surface' else None), truth.cpu().numpy()
    t1 = time.perf_counter()
    jobs = [(np.packbits(hp[i, :, :, c] != 0) if hp is not None else None, np.packbits(ht[i, :, :, c] != 0)) for i in range(n) for c in range(CHANNELS)]
    t2 = time.perf_counter()
    fn = _surface_job if args.call == 'surface' else _map_job
    with mp.get_context('spawn').Pool(WORKERS) as pool:
        pool.map(fn, jobs[:WORKERS])                                               # workers started and their imports done
        t3 = time.perf_counter()
        res = pool.map(fn, jobs, chunksize=4)
        t4 = time.perf_counter()
    out['host_path'] = {'d2h_stacks_s_pageable': round(t1 - t0, 3), 'pack_s': round(t2 - t1, 3), 'scipy_s': round(t4 - t3, 3), 'workers': WORKERS}
    out['host_end_to_end_s'] = round((t1 - t0) + (t2 - t1) + (t4 - t3), 3)
    if args.call == 'surface':
        (d_ab, d_ba), (o_ab, o_ba), counts = got
        equal = (np.array_equal(d_ab, np.concatenate([r[0] for r in res])) and np.array_equal(d_ba, np.concatenate([r[1] for r in res]))
                 and np.array_equal(np.diff(o_ab), [r[0].size for r in res]) and np.array_equal(np.diff(o_ba), [r[1].size for r in res])
                 and np.array_equal(counts.reshape(-1, 3), np.array([r[2] for r in res])))
        out['boundary_pixels'] = {'pred': int(o_ab[-1]), 'truth': int(o_ba[-1])}
    else:
        equal = all(bool(torch.equal(got[i, c], torch.from_numpy(res[i * CHANNELS + c]).to(dev))) for i in range(n) for c in range(CHANNELS))
    out['equal'] = bool(equal)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not equal:
        raise SystemExit('kernels and host comparator disagree')


def _per_call(prof_dir):
    """Per kernel the median over the last REPS calls of the time all its launches of ONE call take, in microseconds; every call makes the same
    launches, so the k-th call owns the k-th share of a kernel's launches in time order."""
    from bench_cleanup import _kernel_rows
    rows = _kernel_rows(prof_dir)
    calls = REPS + WARMUP
    out, launches = {}, {}
    groups = {k: [] for k in KERNELS + ('other',)}
    for name, start, end in rows:
        key = next((k for k in KERNELS if re.search(r'(^|[^a-z_])' + k + r'\b', name)), 'other')
        groups[key].append((end - start) / 1e3)
    for k, durs in groups.items():
        if not durs or len(durs) % calls:
            if durs:
                out[k + '_total_us_all_calls'] = round(sum(durs), 1)     # launches that do not divide into the calls (set-up work of torch)
            continue
        per = len(durs) // calls
        sums = [sum(durs[i * per:(i + 1) * per]) for i in range(calls)][WARMUP:]
        out[k] = round(statistics.median(sums), 1)
        launches[k] = per
    return out, launches


def run_record(args):
    rec = {'commit': args.commit, 'device': 'MI355X (gfx950)', 'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS,
           'measured': 'once; the box-to-box spread of the pool is +-2 %',
           'method': 'kernel times: rocprofv3 --kernel-trace in a run of its own per workload and call, 23 calls, the first 3 dropped, per kernel '
                     'the median over 20 calls of the sum of its launches in one call; call times: events and wall clock around 20 calls after 3 '
                     'warm-up calls in one process with the host comparator (device-to-host copy + scipy.ndimage on 16 processes), checked equal',
           'workloads': {'A': 'filled ellipses from a seed (tools/bench_measure.py) as truth, shifted by (3, 5) as prediction',
                         'B': 'one set pixel per plane: truth top-left, prediction bottom-right (the worst case of the row search)'},
           'column_pass_floor': {'bytes_per_pixel_and_plane': 2.125, 'planes': N * CHANNELS,
                                 'bytes': int(N * CHANNELS * SIZE * SIZE * 2.125),
                                 'ms_at_6.3_TBs': round(N * CHANNELS * SIZE * SIZE * 2.125 / (HBM_ACHIEVABLE_TBS * 1e12) * 1e3, 3)},
           'runs': {}}
    for wl in ('A', 'B'):
        for call in ('surface', 'map'):
            run = {}
            prof = os.path.join(args.dir, f'distance_prof_{wl}_{call}')
            if os.path.isdir(prof):
                run['kernel_us_per_call'], run['launches_per_call'] = _per_call(prof)
            cmp_path = os.path.join(args.dir, f'distance_compare_{wl}_{call}.json')
            if os.path.exists(cmp_path):
                with open(cmp_path) as f:
                    run['same_process_comparison'] = json.load(f)
            if run:
                rec['runs'][f'{wl}_{call}'] = run
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(rec, indent=1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='cmd', required=True)
    for name in ('kernel', 'compare'):
        p = sub.add_parser(name)
        p.add_argument('--workload', choices=('A', 'B'), required=True)
        p.add_argument('--call', choices=('surface', 'map'), required=True)
        if name == 'compare':
            p.add_argument('--slices', type=int, default=N)
            p.add_argument('--out', default=None)
    r = sub.add_parser('record')
    r.add_argument('--dir', required=True)
    r.add_argument('--commit', default='unknown')
    r.add_argument('--out', required=True)
    args = ap.parse_args()
    {'kernel': run_kernel, 'compare': run_compare, 'record': run_record}[args.cmd](args)


if __name__ == '__main__':
    main()
