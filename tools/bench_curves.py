"""Timing of the logit histograms (csrc/curves.hip, oct_segmentation_amd/curves.py).  Needs an MI355X.

octseg_logit_histogram (the clear of hist included) at (16, 1, 704, 704) and (16, 2, 704, 704) on two inputs -- `saturated`: logits N(0, 6^2), what
a trained network puts out, 36 % of the pixels in bin 0 or bin 255; `uniform`: logits whose probability is uniform in (0, 1), every bin alike, the
worst case for the LDS atomics -- against a torch composition that produces the same table in the same process: sigmoid -> ceil -> one bincount
over (plane, label, bin).  A sample is the device-event time of LAUNCHES back-to-back calls divided by LAUNCHES, each call on the next of POOL
input copies so that no call finds its input in the 256 MB last-level cache; the two forms alternate sample by sample; warm-up, then the
median and the spread of the samples.  bytes = 8 per pixel (logits and target read once) + the table.

      python tools/bench_curves.py --out profiles/curves_timing.txt [--commit <id>]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((16, 1, 704, 704), (16, 2, 704, 704))
POOL, LAUNCHES = 6, 12


def _inputs(kind, shape, dev):
    import torch
    g = torch.Generator(device='cpu').manual_seed(0)
    pool = []
    for _ in range(POOL):
        if kind == 'saturated':
            z = torch.randn(shape, generator=g) * 6
        else:
            u = torch.rand(shape, generator=g, dtype=torch.float64).clamp_(1e-6, 1 - 1e-6)
            z = torch.log(u / (1 - u)).float()
        t = (torch.rand(shape, generator=g) < 0.1).float()
        pool.append((z.to(dev), t.to(dev)))
    return pool


def torch_table(z, t):
    import torch
    N, C = z.shape[:2]
    b = (torch.ceil(torch.sigmoid(z) * 256.0) - 1).clamp_(0, 255).long()
    plane = torch.arange(N * C, device=z.device).view(N, C, 1, 1)
    idx = (plane * 2 + (t != 0).long()) * 256 + b
    return torch.bincount(idx.flatten(), minlength=N * C * 512).view(N, C, 2, 256)


def _sample(fn, pool, start):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(LAUNCHES):
        fn(*pool[(start + k) % POOL])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / LAUNCHES


def main():
    import torch
    from oct_segmentation_amd import curves
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--commit', default='')
    ap.add_argument('--samples', type=int, default=25)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_curves needs a GPU')
    if args.samples * LAUNCHES < 20:
        raise SystemExit('at least 20 launches per form')
    dev = torch.device('cuda:0')
    lines = [f'logit histograms, {torch.cuda.get_device_name(0)}, commit {args.commit or "(working tree)"}',
             f'sample = {LAUNCHES} back-to-back calls over {POOL} input copies / {LAUNCHES}; {args.samples} samples per form after {args.warmup} '
             f'warm-up samples, forms alternating; ms per call: median [min .. max] iqr',
             '']
    for shape in SHAPES:
        nbytes = 8 * shape[0] * shape[1] * shape[2] * shape[3] + shape[0] * shape[1] * 2048
        for kind in ('saturated', 'uniform'):
            pool = _inputs(kind, shape, dev)
            out = torch.empty(shape[:2] + (2, 256), dtype=torch.int32, device=dev)
            forms = {'octseg_logit_histogram': lambda z, t: curves.logit_histograms(z, t, out=out), 'torch sigmoid-ceil-bincount': torch_table}
            got, ref = curves.logit_histograms(*pool[0]).long(), torch_table(*pool[0])
            moved = int((got - ref).abs().sum()) // 2
            hot = float(got[:, :, :, [0, 255]].sum()) / float(got.sum())
            times = {name: [] for name in forms}
            for s in range(args.warmup + args.samples):
                for name, fn in forms.items():
                    ms = _sample(fn, pool, s)
                    if s >= args.warmup:
                        times[name].append(ms)
            lines.append(f'{shape} {kind}: {nbytes / 1e6:.1f} MB per call, {hot:.1%} of the pixels in bin 0 / 255; '
                         f'{moved} of {shape[0] * shape[1] * shape[2] * shape[3]} pixels in another bin than torch.sigmoid puts them')
            for name, ts in times.items():
                med, q = statistics.median(ts), statistics.quantiles(ts, n=4)
                lines.append(f'  {name:30s} {med:8.4f} [{min(ts):.4f} .. {max(ts):.4f}] iqr {q[2] - q[0]:.4f}   {nbytes / med / 1e6:8.1f} GB/s')
            k, t = (statistics.median(times[n]) for n in forms)
            lines.append(f'  kernel / torch = {k / t:.3f}')
            del pool
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
