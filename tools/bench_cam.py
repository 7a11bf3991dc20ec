"""Cost of one class activation map (oct_segmentation_amd/cam.py, csrc/cam.hip).  Needs an MI355X.

U-Net / resnet50, one 512 x 512 frame, one class, seeded weights: the frozen forward, the seeded data-only backward and the map kernels of
CAMProcessor.batch, timed with events; beside it the same map through torch on the CPU share of the same host (the oracle net in eval(),
autograd to encoder.layer4[-1], tests/cam_ref.py for the map), timed once per round.  Prints one JSON line.

    python tools/bench_cam.py [--method GradCAM] [--rounds 20] [--cpu-rounds 2] [--dtype fp32]
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

ARCH, ENCODER, S = 'unet', 'resnet50', 512


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--method', default='GradCAM')
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--cpu-rounds', type=int, default=2)
    ap.add_argument('--dtype', default='fp32', choices=['fp32', 'bf16'])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_cam: no GPU visible; there is nothing to measure without one')
    import cam_ref as R
    from oracle import create_model
    from oct_segmentation_amd import cam
    from oct_segmentation_amd.engine import SegNet
    dev = torch.device('cuda:0')
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    torch.manual_seed(0)
    ref = create_model(ARCH, ENCODER, classes=1).eval()
    net = SegNet(ARCH, ENCODER, classes=1, device=dev, compute_dtype=torch.float32 if a.dtype == 'fp32' else torch.bfloat16).eval()
    net.load_state_dict(ref.state_dict())
    g = torch.Generator().manual_seed(1)
    x = torch.floor(torch.rand(1, 3, S, S, generator=g) * 256)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing='ij')
    mask = (((yy - 200) ** 2 + (xx - 300) ** 2) < 120 ** 2).float()[None]
    proc = cam.CAMProcessor(net, dev, a.method, [net.encoder.layer4[-1]])
    xd, md = x.to(dev), mask.to(dev)
    for _ in range(3):
        m_gpu = proc.batch(xd, [0], md)['maps']
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m_gpu = proc.batch(xd, [0], md)['maps']
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    cpu = []
    for _ in range(a.cpu_rounds):
        t0 = time.perf_counter()
        kept = {}

        def keep(_m, _i, out):
            out.retain_grad()
            kept['A'] = out
        h = ref.encoder.layer4[-1].register_forward_hook(keep)
        logits = ref(x)
        h.remove()
        ref.zero_grad()
        (logits[:, 0] * mask).sum().backward()
        m_cpu = R.cam_map(kept['A'].detach()[0].numpy(), kept['A'].grad[0].numpy(), a.method, S, np.float32)
        cpu.append((time.perf_counter() - t0) * 1e3)
    gpu_ms, cpu_ms = statistics.median(ms), statistics.median(cpu)
    out = {'workload': f'{ARCH}/{ENCODER} {S}x{S} one class {a.method} {a.dtype}', 'gpu_ms_per_map': round(gpu_ms, 3), 'gpu_maps_per_s': round(1e3 / gpu_ms, 1),
           'cpu_ms_per_map': round(cpu_ms, 1), 'cpu_maps_per_s': round(1e3 / cpu_ms, 2), 'cpu_threads': torch.get_num_threads(),
           'max_abs_diff_gpu_vs_cpu': float(np.abs(m_gpu[0].cpu().numpy() - m_cpu).max()), 'rounds': a.rounds, 'cpu_rounds': a.cpu_rounds}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
