"""Measurements of the voted serving epilogue (csrc/vote.hip, oct_segmentation_amd/vote.py).  Needs an MI355X.

  kernel   octseg_vote_assemble at N = 16, 704 x 704 -> 1000 x 1000, M in {1, 5, 8, 40} members, the flips (codes 0..3) and all of D4 (0..7),
           soft vote, mask only and with every optional output; in the SAME process and alternating with it, M separate octseg_mask_assemble
           launches over the same logits -- the only way the library could read M logits tensors before.  HIP events, warm-up, median and
           spread of the repeats; bytes = the M logits planes read once + the outputs written.
  predict  frames/s of segment_stack_voted (tta='flips', one directory per class: M = 4) against segment_stack on the serving ensemble
           (U-Net++/resnet101, LinkNet/resnet50, U-Net/resnet50 at 704, bf16, random weights), 128 frames to 1000 x 1000; both calls load
           their checkpoints, as a predict run does, so loading the three networks is timed on its own and the ratio is given with and without it.

      python tools/bench_vote.py --out profiles/vote_704.json [--commit <id>] [--skip-predict]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, S, OUT = 16, 704, 1000
PREDICT_FRAMES = 128
MEMBERS = (1, 5, 8, 40)
VIEW_KINDS = {'flips': (0, 1, 2, 3), 'd4': (0, 1, 2, 3, 4, 5, 6, 7)}


def _ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _summary(times, nbytes):
    med = statistics.median(times)
    q = statistics.quantiles(times, n=4)
    return {'median_ms': round(med, 4), 'min_ms': round(min(times), 4), 'max_ms': round(max(times), 4), 'iqr_ms': round(q[2] - q[0], 4),
            'bytes': nbytes, 'tb_per_s': round(nbytes / med / 1e9, 3)}


def run_kernel(reps, warmup):
    import torch
    from oct_segmentation_amd import _lib as L, vote
    from oct_segmentation_amd.predict import cv2_nearest_index
    dev = torch.device('cuda:0')
    lib = L.lib()
    g = torch.Generator(device='cpu').manual_seed(0)
    pool = [(torch.randn((N, 1, S, S), generator=g) * 3).to(dev) for _ in range(max(MEMBERS))]
    rows = torch.from_numpy(cv2_nearest_index(S, OUT)).to(dev)
    out = torch.zeros((N, OUT, OUT, 4), dtype=torch.float32, device=dev)
    prob, dissent = torch.zeros_like(out), torch.zeros((N, OUT, OUT, 4), dtype=torch.uint8, device=dev)
    stats = torch.zeros((N, 4), dtype=torch.int32, device=dev)
    px_in, px_out = N * S * S, N * OUT * OUT
    results = []
    for kind, codes in VIEW_KINDS.items():
        for M in MEMBERS:
            zs, views = pool[:M], [codes[m % len(codes)] for m in range(M)]
            forms = {
                'fused_mask_only': (lambda: vote.vote_logits(zs, [0] * M, views, out, 0, rows, rows, 'soft'), M * px_in * 4 + px_out * 4),
                'fused_all_outputs': (lambda: vote.vote_logits(zs, [0] * M, views, out, 0, rows, rows, 'soft', prob=prob, dissent=dissent, stats=stats),
                                      M * px_in * 4 + px_out * 9 + N * 16),
                'separate_mask_assemble': (lambda: [L.check(lib.octseg_mask_assemble(L.ptr(z), N, 1, S, S, 0, L.ptr(out), OUT, OUT, 4, 0, L.ptr(rows),
                                                                                      L.ptr(rows), L.stream_ptr())) for z in zs],
                                           M * px_in * 4 + M * px_out * 4),
            }
            times = {k: [] for k in forms}
            for rep in range(warmup + reps):          # the forms alternate inside every repeat
                for k, (fn, _) in forms.items():
                    t = _ms(fn)
                    if rep >= warmup:
                        times[k].append(t)
            row = {'views': kind, 'M': M, **{k: _summary(times[k], forms[k][1]) for k in forms}}
            sep, fus = row['separate_mask_assemble'], row['fused_mask_only']
            row['fused_over_separate'] = round(fus['median_ms'] / sep['median_ms'], 3)
            row['fused_slower_than_separate_beyond_spread'] = bool(fus['median_ms'] - sep['median_ms'] > max(fus['iqr_ms'], sep['iqr_ms']))
            results.append(row)
            print(json.dumps(row), flush=True)
    return results


def run_predict(reps):
    import numpy as np
    import torch
    from oct_segmentation_amd import vote
    from oct_segmentation_amd.model import OCTSegmentationModel
    from oct_segmentation_amd.predict import load_model, segment_stack
    dev = torch.device('cuda:0')
    ensemble = {'LM': ('unetplusplus', 'resnet101', ['Lumen']), 'FC_LC': ('linknet', 'resnet50', ['Lipid core', 'Fibrous cap']),
                'VV': ('unet', 'resnet50', ['Vasa vasorum'])}
    classes = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (PREDICT_FRAMES, OUT, OUT, 3), dtype=np.uint8)).to(dev)
    with tempfile.TemporaryDirectory() as root:
        for i, (d, (arch, enc, cl)) in enumerate(ensemble.items()):
            os.makedirs(os.path.join(root, d))
            m = OCTSegmentationModel(arch, enc, f'{arch}_{enc}', 3, cl, device=dev, seed=40 + i, compute_dtype=torch.bfloat16)
            m.save_checkpoint(os.path.join(root, d, 'weights.ckpt'))
            with open(os.path.join(root, d, 'config.json'), 'w') as f:
                json.dump({'model_name': f'{arch}_{enc}', 'architecture': arch, 'encoder': enc, 'input_size': S, 'classes': cl}, f)
            del m
        forms = {'load_models_only': lambda: [load_model(os.path.join(root, d), dev, torch.bfloat16) for d in ensemble],
                 'unvoted': lambda: segment_stack(frames, [OUT, OUT], classes, root, batch_size=8, device_preprocess=True),
                 'voted_flips_M4': lambda: vote.segment_stack_voted(frames, [OUT, OUT], classes, root, tta='flips', folds=False, batch_size=8)}
        out = {'frames': PREDICT_FRAMES, 'batch_size': 8, 'dtype': 'bf16', 'includes': 'checkpoint loading, as a predict run does', 'reps': reps}
        for k, fn in forms.items():
            fn()
            torch.cuda.synchronize()
            secs = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
            out[k] = {'median_s': round(statistics.median(secs), 4), 'min_s': round(min(secs), 4), 'max_s': round(max(secs), 4),
                      'frames_per_s': round(PREDICT_FRAMES / statistics.median(secs), 2)}
        load = out['load_models_only']['median_s']
        del out['load_models_only']['frames_per_s']
        out['voted_over_unvoted_frames_per_s'] = round(out['voted_flips_M4']['frames_per_s'] / out['unvoted']['frames_per_s'], 3)
        out['voted_over_unvoted_net_of_loading'] = round((out['unvoted']['median_s'] - load) / (out['voted_flips_M4']['median_s'] - load), 3)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--predict-reps', type=int, default=3)
    ap.add_argument('--skip-predict', action='store_true')
    ap.add_argument('--commit', default='unknown')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_vote: no GPU visible; there is nothing to measure without one')
    if args.reps < 20:
        raise SystemExit('bench_vote: the record is the median of at least 20 repeats')
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    rec = {'commit': args.commit, 'device': 'MI355X (gfx950)', 'batch': N, 'logits': f'{S}x{S}', 'frame': f'{OUT}x{OUT}',
           'method': f'HIP events around one call, {args.warmup} warm-up repeats dropped, median / min / max / interquartile range of {args.reps}; the '
                     'three forms alternate inside every repeat of one process; bytes from the shapes (every logits plane read once, outputs '
                     'written once: 4 B mask, + 4 B prob + 1 B dissent + 16 B of counts per frame); TB/s = bytes / median',
           'kernel': run_kernel(args.reps, args.warmup)}
    if not args.skip_predict:
        rec['predict'] = run_predict(args.predict_reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
