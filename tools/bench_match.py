"""Measurements of the lesion matching (csrc/match.hip, oct_segmentation_amd/match.py).  Needs an MI355X.

The workload: N = 186, 704 x 704, four classes.  truth = the stack of tools/bench_contours.py (tests/synth.py's disc masks); pred = the same moved by
3 pixels in x, without every fifth lesion of each class's ranked list (ranks 4, 9, 14, ...).

  kernel   match_volumes on the pair; run it under the profiler, in a run of its own:
               rocprofv3 --kernel-trace --stats -d out/match_prof -- python tools/bench_match.py kernel
  compare  in ONE process: events around match_volumes and around the yardstick, two lesions.lesion_table(profile=False) calls on the same two
           stacks (the labelling the match cannot avoid), median of 10 after warm-up; checks that the match's nles / top equal the yardstick's and
           that the table sums to the frames' intersections:
               python tools/bench_match.py compare --out out/match_compare.json
  record   merge both into profiles/match_704.json:
               python tools/bench_match.py record --prof out/match_prof --compare out/match_compare.json --commit <id> --out profiles/match_704.json
"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

if os.environ.get('OCTSEG_LIB'):   # an experimental build of the library (timing experiments)
    from oct_segmentation_amd import _lib as _L
    _L.LIB_PATH = os.path.abspath(os.environ['OCTSEG_LIB'])

N, SIZE, CHANNELS = 186, 704, 4
WARMUP = 3
ACROSS = 'overlap'
SHIFT = 3
KERNELS = ('bits_pack_kernel', 'ccl_init_kernel', 'ccl_merge_kernel', 'vol_across_kernel', 'ccl_flatten_kernel', 'vol_count_kernel',
           'vol_select_kernel', 'vol_extent_kernel', 'vol_match_kernel', 'vol_match_tables_kernel')


def _pair(dev, n=N):
    """(pred, truth) float32 [n, SIZE, SIZE, CHANNELS] on the device, and the lesions removed per class."""
    import torch
    from bench_contours import _stack
    from oct_segmentation_amd import lesions
    truth = _stack(dev, n)
    labels = lesions.label_volume(truth, across=ACROSS)                      # [channels, n, H, W]
    nles, top = lesions.lesion_table(truth, across=ACROSS)
    keep = torch.ones_like(labels, dtype=torch.bool)
    removed = []
    for c in range(CHANNELS):
        gone = [int(top[c, r, 1]) + 1 for r in range(4, min(int(nles[c]), 32), 5)]
        removed.append(len(gone))
        if gone:
            keep[c] &= ~torch.isin(labels[c], torch.tensor(gone, dtype=torch.int32, device=dev))
    del labels
    pred = torch.zeros_like(truth)
    pred[:, :, SHIFT:, :] = (truth * keep.permute(1, 2, 3, 0).to(truth.dtype))[:, :, :-SHIFT, :]
    del keep
    torch.cuda.empty_cache()
    return pred, truth, removed


def run_kernel(args):
    import torch
    from bench_contours import _need_gpu
    from oct_segmentation_amd import match
    dev = _need_gpu()
    pred, truth, _ = _pair(dev)
    for _ in range(args.reps + WARMUP):
        match.match_volumes(pred, truth, across=ACROSS)
    torch.cuda.synchronize()
    print(json.dumps({'reps': args.reps, 'stack_bytes': int(pred.numel() * 4)}))


def run_compare(args):
    import torch
    from bench_contours import _need_gpu
    from oct_segmentation_amd import _lib as L
    from oct_segmentation_amd import lesions, match
    dev = _need_gpu()
    pred, truth, removed = _pair(dev, args.slices)
    n = int(pred.shape[0])
    calls = {'match_volumes': lambda: match.match_volumes(pred, truth, across=ACROSS),
             'two_lesion_tables': lambda: (lesions.lesion_table(pred, across=ACROSS, profile=False),
                                           lesions.lesion_table(truth, across=ACROSS, profile=False))}
    out = {'slices': n, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS, 'across': ACROSS, 'reps': args.reps, 'warmup': WARMUP,
           'stack_bytes_each': int(pred.numel() * 4), 'lesions_removed_from_pred': removed,
           'match_scratch_bytes': int(L.lib().octseg_match_scratch_bytes(CHANNELS, n, SIZE, SIZE)),
           'lesions_scratch_bytes': int(L.lib().octseg_lesions_scratch_bytes(CHANNELS, n, SIZE, SIZE))}
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
    out['match_over_two_lesion_tables'] = round(out['match_volumes_events_ms']['median'] / out['two_lesion_tables_events_ms']['median'], 3)
    m = results['match_volumes']
    equal = True
    for side, (nles, top) in enumerate(results['two_lesion_tables']):
        equal = equal and bool(torch.equal(m.nles[:, side], nles)) and bool(torch.equal(m.top[:, side], top))
    equal = equal and bool(torch.equal(m.overlap.sum(dim=(1, 2)), m.frames[:, :, 0].sum(dim=1)))
    equal = equal and bool(torch.equal(m.frames[:, :, 2].sum(dim=1).to(torch.int64), (truth != 0).sum(dim=(0, 1, 2))))
    out['nles'] = m.nles.cpu().tolist()
    out['shared_voxels'] = m.overlap.sum(dim=(1, 2)).cpu().tolist()
    out['equal'] = bool(equal)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    if not equal:
        raise SystemExit('match_volumes and the yardstick disagree')


def _per_call(prof_dir, calls):
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
    rec = {'commit': args.commit, 'device': 'MI355X (gfx950)', 'slices': N, 'frame': f'{SIZE}x{SIZE}', 'channels': CHANNELS,
           'masks': 'truth: tests/synth.py make_batch as in tools/bench_contours.py; pred: truth moved 3 pixels in x without ranks 4, 9, 14, ... '
                    'of each class',
           'method': 'events round the calls in one process, median of 10 after 3 warm-up calls; per kernel: rocprofv3 --kernel-trace in a run of '
                     'its own, the sum of its launches over all match calls (warm-up calls included) divided by their number; measured once; no '
                     'counter was collected'}
    if args.prof:
        # the pair's construction labels truth once (label_volume + lesion_table): those launches carry the labelling kernels' names too, so only
        # the kernels the match alone launches are exact per call
        us, launches = _per_call(args.prof, args.reps + WARMUP)
        rec['kernel_us_per_match_call'] = {k: v for k, v in us.items() if k.startswith('vol_match')}
        rec['launches_per_match_call'] = {k: v for k, v in launches.items() if k.startswith('vol_match')}
        words = CHANNELS * N * SIZE * ((SIZE + 63) // 64)
        rec['vol_match_kernel_bit_plane_bytes_read'] = 2 * 8 * words
        t = rec['kernel_us_per_match_call'].get('vol_match_kernel')
        if t:
            rec['vol_match_kernel_bit_plane_gb_per_s'] = round(2 * 8 * words / t / 1e3, 1)
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
    k = sub.add_parser('kernel'); k.add_argument('--reps', type=int, default=5)
    c = sub.add_parser('compare'); c.add_argument('--reps', type=int, default=10); c.add_argument('--slices', type=int, default=N)
    c.add_argument('--out', default=None)
    r = sub.add_parser('record'); r.add_argument('--prof', default=None); r.add_argument('--compare', default=None)
    r.add_argument('--reps', type=int, default=5); r.add_argument('--commit', default='unknown'); r.add_argument('--out', required=True)
    args = ap.parse_args()
    {'kernel': run_kernel, 'compare': run_compare, 'record': run_record}[args.cmd](args)


if __name__ == '__main__':
    main()
