"""Measurements of the lumen geometry kernels (csrc/shape.hip, oct_segmentation_amd/shape.py).  Needs an MI355X.

  kernel   octseg_stack_moments, octseg_stack_polar_at from the lumen's centroid (shared origins: one gather per step) and from every plane's
           own centroid (a walk per channel), then the yardsticks octseg_stack_polar and octseg_stack_measure on the same stack, at N = 186,
           750 x 750, four classes (the workload of tools/bench_measure.py: filled-ellipse masks from a seed); run it under the profiler, in a
           run of its own, with no counters in the same run:
               rocprofv3 --kernel-trace --stats -d out/shape_prof -- python tools/bench_shape.py kernel
  compare  in ONE process: the calls with events around them (median of 20 after warm-up), lumen_report end to end, and that moments, origins
           and profile of slices 0, 62, 124 and 185 equal tests/shape_ref.py:
               python tools/bench_shape.py compare --out out/shape_compare.json
  record   merge both into profiles/shape_750.json, with the moments kernel as a ratio to count_kernel (the same bytes, less arithmetic) and to
           the byte floor, and the walks as ratios to polar.hip's profile_kernel:
               python tools/bench_shape.py record --prof out/shape_prof --compare out/shape_compare.json --commit <id> --out profiles/shape_750.json
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

import bench_measure as BM  # noqa: E402
import bench_polar as BP  # noqa: E402

N, SIZE, CHANNELS, WARMUP = BM.N, BM.SIZE, BM.CHANNELS, BM.WARMUP


def run_kernel(args):
    """reps + WARMUP calls each of: moments, the walk from the lumen's centroid, the walk from own centroids, polar_profile, measure_stack --
    in that order, so the record can tell the two halves of the walk_kernel launches apart.  The origins are computed once, outside the loops."""
    import torch
    from oct_segmentation_amd import analysis, polar, shape
    dev = BM._need_gpu()
    stack = BM.elliptic_stack(dev)
    mom = shape.moments_stack(stack)
    shared, own = shape.origins(stack, mom, 'Lumen'), shape.origins(stack, mom)
    torch.cuda.synchronize()
    for fn in (lambda: shape.moments_stack(stack), lambda: shape.centred_profile(stack, shared), lambda: shape.centred_profile(stack, own),
               lambda: polar.polar_profile(stack), lambda: analysis.measure_stack(stack)):
        for _ in range(args.reps + WARMUP):
            fn()
        torch.cuda.synchronize()
    print(json.dumps({'reps': args.reps, 'stack_bytes': BM.stack_bytes()}))


def run_compare(args):
    import torch
    import shape_ref as S
    from oct_segmentation_amd import analysis, polar, shape
    from oct_segmentation_amd.model import CLASS_IDS
    dev = BM._need_gpu()
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    stack = BM.elliptic_stack(dev)
    names = [f'{i:03d}' for i in range(N)]
    mom = shape.moments_stack(stack)
    shared, own = shape.origins(stack, mom, 'Lumen'), shape.origins(stack, mom)
    out = {'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'reps': args.reps, 'stack_bytes': BM.stack_bytes(),
           'moments_stack_events_ms': BP._stats(BM._events_ms(lambda: shape.moments_stack(stack), args.reps)),
           'origins_events_ms': BP._stats(BM._events_ms(lambda: shape.origins(stack, mom, 'Lumen'), args.reps)),
           'centred_profile_shared_events_ms': BP._stats(BM._events_ms(lambda: shape.centred_profile(stack, shared), args.reps)),
           'centred_profile_own_events_ms': BP._stats(BM._events_ms(lambda: shape.centred_profile(stack, own), args.reps)),
           'polar_profile_events_ms': BP._stats(BM._events_ms(lambda: polar.polar_profile(stack), args.reps)),
           'measure_stack_events_ms': BP._stats(BM._events_ms(lambda: analysis.measure_stack(stack), args.reps)),
           'ray_offset_bytes': int(shape.ray_offsets(SIZE, SIZE).nbytes)}
    shape.lumen_report(stack, names)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    report = shape.lumen_report(stack, names)
    out['lumen_report_s'] = round(time.perf_counter() - t0, 4)
    out['mla'], out['area_stenosis'] = report['mla'], report['area_stenosis']
    pick = [0, 62, 124, 185]
    host = stack[pick].cpu().numpy()
    want_mom = S.moments(host)
    off = shape.ray_offsets(SIZE, SIZE)
    equal = bool(np.array_equal(mom[pick].cpu().numpy(), want_mom))
    lumen = CLASS_IDS['Lumen'] - 1
    for org, ref in ((shared, lumen), (own, -1)):
        want_org = S.origins(host, want_mom, ref)
        want, want_len = S.polar_at(host, want_org, off)
        prof, length, _ = shape.centred_profile(stack, org)
        equal = equal and bool(np.array_equal(org[pick].cpu().numpy(), want_org) and np.array_equal(prof[pick].cpu().numpy(), want)
                               and np.array_equal(length[pick].cpu().numpy(), want_len))
    out['equal'] = equal
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not equal:
        raise SystemExit('kernels and host restatement disagree')


def run_record(args):
    rows = BP._kernel_rows(args.prof)
    walk_us = [us for name, us in rows if 'walk_kernel' in name]
    if len(walk_us) % 2 or not walk_us:
        raise SystemExit(f'{len(walk_us)} walk_kernel launches in {args.prof}: expected two equal halves (shared and own origins)')
    half = len(walk_us) // 2
    groups = {'moments_kernel': [us for name, us in rows if 'moments_kernel' in name],
              'moments_init_kernel': [us for name, us in rows if 'moments_init_kernel' in name],
              'walk_kernel_shared_origin': walk_us[:half], 'walk_kernel_own_origins': walk_us[half:],
              'profile_kernel': [us for name, us in rows if 'profile_kernel' in name],
              'ray_kernel': [us for name, us in rows if 'ray_kernel' in name], 'count_kernel': [us for name, us in rows if 'count_kernel' in name]}
    floor_us = BM.stack_bytes() / (BM.HBM_ACHIEVABLE_TBS * 1e12) * 1e6
    rec = {'commit': args.commit, 'device': 'MI355X (gfx950)', 'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS,
           'masks': 'filled ellipses from a seed (tools/bench_measure.py elliptic_stack)',
           'method': f'kernel times: rocprofv3 --kernel-trace --stats in a run of its own (no counters), first {WARMUP} calls of each group '
                     'dropped, median of the rest; call times: HIP events around the call in one process, median after warm-up; measured once. '
                     'count_kernel, ray_kernel (csrc/measure.hip) and profile_kernel (csrc/polar.hip) are the parent commit\'s: this change does '
                     'not touch their sources or build flags, and they run in the same process on the same stack',
           'stack_bytes': BM.stack_bytes(), 'byte_floor_us': round(floor_us, 1), 'byte_floor_rule': f'stack_bytes / {BM.HBM_ACHIEVABLE_TBS} TB/s',
           'kernel': {}}
    for k, t in groups.items():
        t = t[WARMUP:]
        if not t:
            raise SystemExit(f'no {k} launches in {args.prof}')
        rec['kernel'][k] = {'calls': len(t), 'median_us': round(statistics.median(t), 2), 'min_us': round(min(t), 2), 'max_us': round(max(t), 2)}
    med = {k: v['median_us'] for k, v in rec['kernel'].items()}
    rec['ratios'] = {'moments_kernel / count_kernel': round(med['moments_kernel'] / med['count_kernel'], 3),
                     'moments_kernel / byte_floor': round(med['moments_kernel'] / floor_us, 3),
                     'count_kernel / byte_floor': round(med['count_kernel'] / floor_us, 3),
                     'walk_kernel_shared_origin / profile_kernel': round(med['walk_kernel_shared_origin'] / med['profile_kernel'], 3),
                     'walk_kernel_own_origins / profile_kernel': round(med['walk_kernel_own_origins'] / med['profile_kernel'], 3)}
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
