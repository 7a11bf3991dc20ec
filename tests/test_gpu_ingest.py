"""Device half of the input pipeline (csrc/ingest.hip through oct_segmentation_amd/ingest.py, dataset.py, predict.segment) against the
oracle's scalar restatement of OpenCV's resizes (oracle/cv2_resize.py).  The arithmetic is integer: every comparison is equality."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import ingest
from oracle.cv2_resize import resize_linear_u8, resize_nn

pytestmark = pytest.mark.gpu


def _image_oracle(frames, dh, dw, swap_rb):
    """dataset.py:110 + to_tensor_shape (swap_rb: data/utils.py:164 cvtColor(RGB2BGR) first): float32 [B,3,dh,dw]."""
    out = []
    for f in frames:
        f = np.ascontiguousarray(f[:, :, ::-1]) if swap_rb else f
        out.append(resize_linear_u8(f, (dw, dh)).transpose(2, 0, 1).astype(np.float32))
    return np.stack(out)


def _mask_oracle(masks, class_ids, dh, dw):
    """dataset.py:112-118,125 restated: INTER_NEAREST resize, channel class_id - 1 as bool, stacked, float, CHW."""
    out = []
    for m in masks:
        m = resize_nn(m, (dw, dh))
        sel = [np.array(m[:, :, cid - 1], dtype='bool') for cid in class_ids]
        out.append(np.stack(sel, axis=-1).astype('float').transpose(2, 0, 1).astype('float32'))
    return np.stack(out)


def _run_image(cuda, frames, dh, dw, swap_rb):
    got = ingest.resize_image_u8(torch.from_numpy(frames).to(cuda), (dh, dw), swap_rb=bool(swap_rb))
    assert got.dtype == torch.float32 and tuple(got.shape) == (frames.shape[0], 3, dh, dw)
    return got.cpu().numpy()


IMAGE_CASES = [(20, 30, 17, 23), (20, 30, 41, 37), (75, 75, 64, 64), (13, 7, 26, 14), (50, 50, 32, 32), (32, 32, 32, 32), (64, 48, 32, 24),
               (10, 6, 5, 3), (64, 48, 64, 24), (9, 9, 1, 1), (1, 1, 5, 7), (40, 40, 33, 31), (300, 200, 70, 130)]


@pytest.mark.parametrize('case', IMAGE_CASES, ids=lambda c: '%dx%d-%dx%d' % c)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('swap_rb', [0, 1])
def test_image_equals_cv2_oracle(cuda, case, B, swap_rb):
    hs, ws, hd, wd = case
    rng = np.random.default_rng(hs * 1000 + ws + hd + B)
    frames = rng.integers(0, 256, (B, hs, ws, 3), dtype=np.uint8)
    got = _run_image(cuda, frames, hd, wd, swap_rb)
    print(case, B, swap_rb, 'mismatches', int((got != _image_oracle(frames, hd, wd, swap_rb)).sum()))
    assert np.array_equal(got, _image_oracle(frames, hd, wd, swap_rb))
    if (hs, ws) == (hd, wd):                                   # equal sizes: a copy
        f = frames[:, :, :, ::-1] if swap_rb else frames
        assert np.array_equal(got, f.transpose(0, 3, 1, 2).astype(np.float32))
    if (hs, ws) == (2 * hd, 2 * wd):                           # exact 2x in both axes: INTER_AREA's block mean, the known answer
        s = (frames[:, :, :, ::-1] if swap_rb else frames).astype(np.int64)
        mean = (s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2] + 2) >> 2
        assert np.array_equal(got, mean.transpose(0, 3, 1, 2).astype(np.float32))


def test_image_area_rounding_and_constant_frames(cuda):
    # block means where the bilinear fixed-point kernel would round differently (tests/test_host.py's known answers)
    for blk, want in (([[0, 1], [1, 0]], 1), ([[1, 0], [0, 0]], 0), ([[255, 254], [254, 254]], 254)):
        f = np.repeat(np.array(blk, np.uint8)[None, :, :, None], 3, axis=3)
        assert (_run_image(cuda, f, 1, 1, 0) == want).all()
    for (hs, ws, hd, wd) in ((40, 40, 64, 64), (50, 70, 23, 31), (64, 64, 32, 32), (1000, 1000, 704, 704)):
        for v in (0, 200, 255):
            assert (_run_image(cuda, np.full((2, hs, ws, 3), v, np.uint8), hd, wd, 1) == v).all()


@pytest.mark.parametrize('src,dst', [(1000, 704), (1000, 512), (1024, 512)])
def test_image_realistic_sizes(cuda, src, dst):
    rng = np.random.default_rng(src + dst)
    frames = rng.integers(0, 256, (1, src, src, 3), dtype=np.uint8)
    got = _run_image(cuda, frames, dst, dst, 0)
    want = _image_oracle(frames, dst, dst, 0)
    print(src, dst, 'mismatches', int((got != want).sum()))
    assert np.array_equal(got, want)


MASK_CASES = [(64, 48, 100, 75), (37, 37, 100, 100), (100, 100, 33, 33), (1000, 1000, 704, 704), (750, 750, 704, 704), (30, 50, 21, 35)]


@pytest.mark.parametrize('case', MASK_CASES, ids=lambda c: '%dx%d-%dx%d' % c)
@pytest.mark.parametrize('class_ids', [[3], [2, 1], [4, 2, 1, 3]], ids=lambda c: 'ids' + ''.join(map(str, c)))
def test_mask_equals_cv2_oracle(cuda, case, class_ids):
    hs, ws, hd, wd = case
    rng = np.random.default_rng(hs + wd + len(class_ids))
    B = 1 if hs >= 750 else 3
    masks = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(B, hs, ws, 4))
    got = ingest.select_resize_mask(torch.from_numpy(masks).to(cuda), class_ids, (hd, wd))
    want = _mask_oracle(masks, class_ids, hd, wd)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    print(case, class_ids, 'mismatches', int((got.cpu().numpy() != want).sum()))
    assert np.array_equal(got.cpu().numpy(), want)


def test_mask_other_channel_counts(cuda):
    """Not the 4-channel TIFF layout: the byte path (3 and 5 source channels)."""
    rng = np.random.default_rng(5)
    for cs, ids in ((3, [3, 1]), (5, [5, 2, 4]), (1, [1])):
        masks = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(2, 40, 28, cs))
        got = ingest.select_resize_mask(torch.from_numpy(masks).to(cuda), ids, (33, 45))
        assert np.array_equal(got.cpu().numpy(), _mask_oracle(masks, ids, 33, 45))


def test_batch_of_16_equals_single_frames(cuda):
    """64-bit offsets and the tile / grid-stride loops: 16 frames 1000^2 -> 704^2 in one launch against one launch per frame (the
    single-frame result is pinned to the oracle above)."""
    rng = np.random.default_rng(16)
    frames = torch.from_numpy(rng.integers(0, 256, (16, 1000, 1000, 3), dtype=np.uint8)).to(cuda)
    masks = torch.from_numpy(rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(16, 1000, 1000, 4))).to(cuda)
    img = ingest.resize_image_u8(frames, 704)
    msk = ingest.select_resize_mask(masks, [2, 3], 704)
    for i in range(16):
        assert torch.equal(img[i:i + 1], ingest.resize_image_u8(frames[i:i + 1], 704)), i
        assert torch.equal(msk[i:i + 1], ingest.select_resize_mask(masks[i:i + 1], [2, 3], 704)), i


def test_gather_variant_and_unaligned_views_agree(cuda):
    """The per-pixel yardstick kernels give the shipped kernels' result; a source that does not start on a 4-byte boundary and an
    output slice of a larger batch tensor are handled."""
    rng = np.random.default_rng(3)
    flat = torch.from_numpy(rng.integers(0, 256, (1 + 2 * 90 * 70 * 3,), dtype=np.uint8)).to(cuda)
    frames = flat[1:].view(2, 90, 70, 3)                     # data_ptr % 4 == 1
    masks = torch.from_numpy(rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(2, 90, 70, 4))).to(cuda)
    want_i = _image_oracle(frames.cpu().numpy(), 47, 38, 1)
    want_m = _mask_oracle(masks.cpu().numpy(), [4, 1], 47, 38)
    batch = torch.zeros((5, 3, 47, 38), dtype=torch.float32, device=cuda)
    ingest.resize_image_u8(frames, (47, 38), swap_rb=True, out=batch[2:4])
    assert np.array_equal(batch[2:4].cpu().numpy(), want_i) and not batch[:2].any() and not batch[4:].any()
    try:
        L.check(L.lib().octseg_debug_set_ingest_variant(1))
        assert np.array_equal(ingest.resize_image_u8(frames, (47, 38), swap_rb=True).cpu().numpy(), want_i)
        assert np.array_equal(ingest.select_resize_mask(masks, [4, 1], (47, 38)).cpu().numpy(), want_m)
    finally:
        L.check(L.lib().octseg_debug_set_ingest_variant(0))
    assert np.array_equal(ingest.select_resize_mask(masks, [4, 1], (47, 38)).cpu().numpy(), want_m)
    # decimation too strong for a tile's window to fit LDS: the launch falls back to the gather kernel
    big = rng.integers(0, 256, (1, 700, 2100, 3), dtype=np.uint8)
    assert np.array_equal(_run_image(cuda, big, 9, 70, 0), _image_oracle(big, 9, 70, 0))


def _write_dataset(root, rng, sizes):
    os.makedirs(os.path.join(root, 'img'))
    os.makedirs(os.path.join(root, 'mask'))
    for k, (h, w) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, 'img', f'f{k:02d}.png'))
        m = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(h, w, 4))
        Image.fromarray(m, mode='RGBA').save(os.path.join(root, 'mask', f'f{k:02d}.tiff'))


def test_device_batches_end_to_end_and_fit(cuda, tmp_path):
    from oct_segmentation_amd.config import load_config
    from oct_segmentation_amd.dataset import DeviceBatches, OCTDataset, group_by_shape, train_batches
    from oct_segmentation_amd.train import fit
    rng = np.random.default_rng(9)
    root = os.path.join(str(tmp_path), 'fold', 'train')
    _write_dataset(root, rng, [(80, 80), (100, 90), (80, 80), (100, 90), (80, 80), (100, 90)])
    classes = ['Fibrous cap', 'Lumen']
    ds = OCTDataset(root, classes, input_size=64)
    assert len(ds) == 6
    batches = DeviceBatches(ds, 4, shuffle=True, seed=1, device=cuda)
    for epoch in range(2):                                  # re-iterable: a new permutation per pass
        order = batches.epoch_order(epoch)
        seen = 0
        for b, (img, mask) in enumerate(batches):
            idx = order[b * 4:(b + 1) * 4]
            assert img.is_cuda and img.dtype == torch.float32 and tuple(img.shape) == (len(idx), 3, 64, 64)
            assert tuple(mask.shape) == (len(idx), 2, 64, 64)
            samples = [ds[int(i)] for i in idx]
            # frames of one source size are together, sizes in order of first appearance
            pos = [p for _, ps in group_by_shape([s[0].shape for s in samples]) for p in ps]
            if b == 0:
                assert len({s[0].shape for s in samples}) == 2          # two source sizes in one batch
            for k, p in enumerate(pos):
                f, m = samples[p]
                assert np.array_equal(img[k].cpu().numpy(), _image_oracle(f[None], 64, 64, 0)[0])
                assert np.array_equal(mask[k].cpu().numpy(), _mask_oracle(m[None], ds.class_ids, 64, 64)[0])
            seen += len(idx)
        assert seen == 6
    cfg = load_config('train', ['architecture=unet', 'encoder=resnet18', 'epochs=1', 'input_size=64', 'batch_size=2', 'lr=0.001',
                                'compute_dtype=fp32', 'use_augmentation=false', 'data_dir=' + os.path.join(str(tmp_path), 'fold')])
    cfg['classes'] = classes
    train = train_batches(cfg, 'train', device=cuda)
    assert len(train) == 3
    model, hist = fit(cfg, train, device=cuda)
    assert len(hist) == 1 and np.isfinite(float(hist[0]['train']['loss']))


def test_segment_device_preprocess_equals_host_path(cuda, tmp_path):
    from oct_segmentation_amd.model import OCTSegmentationModel
    from oct_segmentation_amd.predict import segment
    specs = {'LM': ('unet', ['Lumen'], 64), 'FC_LC': ('linknet', ['Lipid core', 'Fibrous cap'], 96), 'VV': ('unet', ['Vasa vasorum'], 64)}
    for d, (arch, classes, size) in specs.items():
        os.makedirs(os.path.join(tmp_path, d))
        m = OCTSegmentationModel(arch, 'resnet18', f'{arch}_resnet18', 3, classes, device=cuda, seed=len(d) + 3, compute_dtype=torch.float32)
        m.save_checkpoint(os.path.join(tmp_path, d, 'weights.ckpt'))
        with open(os.path.join(tmp_path, d, 'config.json'), 'w') as f:
            json.dump({'model_name': f'{arch}_resnet18', 'architecture': arch, 'encoder': 'resnet18', 'input_size': size,
                       'classes': classes}, f)
    rng = np.random.default_rng(0)
    names = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    for sizes in ([(80, 80)] * 3, [(80, 80), (70, 90), (80, 80)]):         # one stacked upload / frames of different sizes
        images = [Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)) for h, w in sizes]
        for use_graph in (False, True):
            host = segment(images, [np.zeros((100, 100, 4)) for _ in images], [100, 100], names, str(tmp_path), device='cuda',
                           compute_dtype=torch.float32, batch_size=2, use_graph=use_graph)
            dev = segment(images, [np.zeros((100, 100, 4)) for _ in images], [100, 100], names, str(tmp_path), device='cuda',
                          compute_dtype=torch.float32, batch_size=2, use_graph=use_graph, device_preprocess=True)
            assert len(dev) == len(host) == 3
            for a, b in zip(dev, host):
                assert a.shape == (100, 100, 4) and np.array_equal(a, b)
            assert any(h.any() for h in host) and not all(h.all() for h in host)   # random weights still give a non-trivial mask


def test_abi_refuses_bad_arguments(cuda):
    lib = L.lib()
    u8 = torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device=cuda)
    out = torch.full((1, 3, 4, 4), -1.0, device=cuda)
    tab = torch.zeros((4, 4), dtype=torch.int32, device=cuda)
    ch = torch.zeros((1,), dtype=torch.int32, device=cuda)
    st = L.stream_ptr()
    p = L.ptr
    BAD_SHAPE, BAD_ARG = -1, -5
    assert lib.octseg_ingest_image(None, 1, 8, 8, 0, p(out), 4, 4, p(tab), p(tab), st) == BAD_ARG
    assert b'null' in lib.octseg_last_error()
    assert lib.octseg_ingest_image(p(u8), 1, 8, 8, 0, None, 4, 4, p(tab), p(tab), st) == BAD_ARG
    assert lib.octseg_ingest_image(p(u8), 1, 8, 8, 0, p(out), 4, 4, None, p(tab), st) == BAD_ARG
    assert lib.octseg_ingest_image(p(u8), 1, 8, 8, 0, p(out), 4, 4, p(tab), None, st) == BAD_ARG
    assert lib.octseg_ingest_image(p(u8), 0, 8, 8, 0, p(out), 4, 4, p(tab), p(tab), st) == BAD_SHAPE
    assert lib.octseg_ingest_image(p(u8), 1, 8, 8, 0, p(out), 0, 4, p(tab), p(tab), st) == BAD_SHAPE
    assert lib.octseg_ingest_image(p(u8), 1, 8, -1, 0, p(out), 4, 4, p(tab), p(tab), st) == BAD_SHAPE
    assert lib.octseg_ingest_mask(None, 1, 8, 8, 4, p(ch), 1, p(out), 4, 4, p(tab), p(tab), st) == BAD_ARG
    assert lib.octseg_ingest_mask(p(u8), 1, 8, 8, 4, None, 1, p(out), 4, 4, p(tab), p(tab), st) == BAD_ARG
    assert lib.octseg_ingest_mask(p(u8), 1, 8, 8, 4, p(ch), 1, p(out), 4, 4, None, p(tab), st) == BAD_ARG
    assert lib.octseg_ingest_mask(p(u8), 0, 8, 8, 4, p(ch), 1, p(out), 4, 4, p(tab), p(tab), st) == BAD_SHAPE
    assert lib.octseg_ingest_mask(p(u8), 1, 8, 8, 4, p(ch), 0, p(out), 4, 4, p(tab), p(tab), st) == BAD_SHAPE
    assert lib.octseg_ingest_mask(p(u8), 1, 8, 8, 0, p(ch), 1, p(out), 4, 4, p(tab), p(tab), st) == BAD_SHAPE
    assert lib.octseg_debug_set_ingest_variant(7) == BAD_ARG
    torch.cuda.synchronize()
    assert (out == -1.0).all()                                 # nothing was launched
    # the Python wrappers refuse what the kernels cannot take
    with pytest.raises(ValueError):
        ingest.resize_image_u8(u8, 4)                          # 4 channels
    with pytest.raises(ValueError):
        ingest.resize_image_u8(u8[..., :3].float(), 4)
    with pytest.raises(ValueError):
        ingest.select_resize_mask(u8, [5], 4)                  # class id beyond the mask's channels
    with pytest.raises(ValueError):
        ingest.select_resize_mask(u8, [], 4)
