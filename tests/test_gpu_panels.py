"""The per-epoch sample strips on the GPU (csrc/panels.hip through oct_segmentation_amd/postprocess.py, model.py and train.py) against the host
restatement of the reference's log_predict_model_on_epoch (tests/panels_ref.py) and against the reference's own run
(tests/golden/epoch_panel.npz).  Comparisons and integer moves only: every check is equality."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import panels_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import ingest, postprocess
from synth import make_batch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PIN = os.path.join(HERE, 'golden', 'epoch_panel.npz')
ALL = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
EDGE = np.array([0.0, -0.0, 1e-8, -1e-8, 1e-3, -1e-3], np.float32)       # logits around the threshold


def _logits(rng, shape, signs=None):
    """Seeded logits with the threshold's neighbourhood mixed in.  signs (0 / 1, same shape): the mask the logits must threshold to --
    set: 1e-3 or a value above it; clear: one of 0.0, -0.0, +-1e-8 (sigmoid is exactly 0.5 in fp32: not > 0.5), -1e-3 or a value below it."""
    z = rng.normal(0.0, 2.0, shape).astype(np.float32)
    pick = rng.integers(0, 3 * len(EDGE), shape)
    if signs is None:
        return np.where(pick < len(EDGE), EDGE[pick % len(EDGE)], z).astype(np.float32)
    hi = np.where(pick < len(EDGE), np.float32(1e-3), np.abs(z) + np.float32(1e-3))
    lo = np.where(pick < len(EDGE), np.array([0.0, -0.0, 1e-8, -1e-8, -1e-3, -1e-3], np.float32)[pick % len(EDGE)], -np.abs(z) - np.float32(1e-3))
    return np.where(np.asarray(signs) == 1, hi, lo).astype(np.float32)


def _planes(frames_bgr):
    """uint8 [N,S,S,3] BGR -> float32 [N,3,S,S], what octseg_ingest_image writes."""
    return np.ascontiguousarray(frames_bgr.transpose(0, 3, 1, 2)).astype(np.float32)


def _assemble(cuda, logits):
    """octseg_mask_assemble at identity size on the same logits: [N,S,S,C] of 0 / 1 -- what predict() thresholds to."""
    z = torch.from_numpy(logits).to(cuda)
    n, c, h, w = z.shape
    out = torch.empty((n, h, w, c), dtype=torch.float32, device=cuda)
    for ch in range(c):
        L.check(L.lib().octseg_mask_assemble(L.ptr(z), n, c, h, w, ch, L.ptr(out), h, w, c, ch, None, None, L.stream_ptr()))
    return out.cpu().numpy()


def _wrapper(cuda, frames_bgr, logits, gt, classes, labels=True):
    p, lab = postprocess.epoch_panels(torch.from_numpy(_planes(frames_bgr)).to(cuda), torch.from_numpy(logits).to(cuda),
                                      torch.from_numpy(gt).to(cuda), classes, labels=labels)
    n, s = frames_bgr.shape[:2]
    assert p.dtype == torch.uint8 and tuple(p.shape) == (n, s, 3 * s, 3)
    assert (lab is None) if not labels else (lab.dtype == torch.uint8 and tuple(lab.shape) == (n, 2, s, s))
    return p.cpu().numpy(), None if lab is None else lab.cpu().numpy()


def _case(rng, n, s, hs, ws, c, sc=4):
    frames = rng.integers(0, 256, (n, s, s, 3), dtype=np.uint8)
    gt = rng.choice(np.array([0, 1, 128, 254, 255], np.uint8), size=(n, hs, ws, sc), p=[0.2, 0.1, 0.15, 0.15, 0.4])
    return frames, gt, _logits(rng, (n, c, s, s))


def test_kernel_equals_the_reference_run(cuda):
    """Case 1: S = 24, N = 2, C = 3 -- the fixture's inputs in, what reached the reference's imwrite and wandb.Image out."""
    z = np.load(PIN)
    classes = [str(c) for c in z['classes']]
    pred = z['pred']
    logits = _logits(np.random.default_rng(1), (2, 3, 24, 24), signs=pred.transpose(0, 3, 1, 2))
    assert np.array_equal(_assemble(cuda, logits), pred.astype(np.float32))          # the pane cannot disagree with predict()
    got, lab = _wrapper(cuda, z['frames_bgr'], logits, z['gt'], classes)
    assert np.array_equal(got, z['res_bgr'][..., ::-1])
    assert np.array_equal(lab[:, 0], z['label_pred']) and np.array_equal(lab[:, 1], z['label_gt'])
    want, wlab = R.panels(z['frames_bgr'], z['gt'], pred, classes)
    assert np.array_equal(got, want) and np.array_equal(lab, wlab)


@pytest.mark.parametrize('s,n,hs,ws,classes', [
    (33, 3, 37, 29, ['Lipid core', 'Vasa vasorum', 'Lumen', 'Fibrous cap']),      # case 2: 297-byte rows, resampling down and up, non-square source
    (16, 1, 8, 8, ['Fibrous cap']),                                               # case 3: the smallest shape
    (20, 2, 20, 20, ['Lipid core', 'Lumen']),                                     # case 4's shape through the wrapper (labels skipped)
])
def test_kernel_equals_the_restatement(cuda, s, n, hs, ws, classes):
    rng = np.random.default_rng(100 * s + n)
    frames, gt, logits = _case(rng, n, s, hs, ws, len(classes))
    pred = _assemble(cuda, logits)
    assert pred.any() and not pred.all()
    want, wlab = R.panels(frames, gt, pred, classes, size=s)
    got, lab = _wrapper(cuda, frames, logits, gt, classes, labels=(s != 20))
    bad = np.argwhere(np.any(got != want, axis=-1))
    assert np.array_equal(got, want), (len(bad), bad[:5].tolist())
    if s != 20:
        assert np.array_equal(lab, wlab)
    # the prediction pane is the colouring of octseg_mask_assemble's mask
    for i in range(n):
        assert np.array_equal(got[i][:, 2 * s:], R.paint(np.zeros((s, s, 4), np.uint8), pred[i], classes)[1])


def _tables(cuda, hs, ws, s):
    return (torch.from_numpy(R.nearest_index(hs, s).astype(np.int32)).to(cuda), torch.from_numpy(R.nearest_index(ws, s).astype(np.int32)).to(cuda))


def test_null_labels_and_clamped_channels_through_the_c_entry(cuda):
    """Case 4: S = 20, N = 2, 20 x 20 source, C = 2; labels null; channel ids outside the source are clamped on the device."""
    rng = np.random.default_rng(4)
    n, s, classes = 2, 20, ['Lumen', 'Vasa vasorum']                  # channels 0 and 3 = what -2 and 7 clamp to in a 4-channel source
    frames, gt, logits = _case(rng, n, s, s, s, 2)
    want, _ = R.panels(frames, gt, _assemble(cuda, logits), classes)
    rows, cols = _tables(cuda, s, s, s)
    ch = torch.tensor([-2, 7], dtype=torch.int32, device=cuda)
    rgb = torch.tensor([R.CLASS_COLORS_RGB[c] for c in classes], dtype=torch.uint8, device=cuda)
    ids = torch.tensor([R.CLASS_IDS[c] for c in classes], dtype=torch.uint8, device=cuda)
    f, z, g = torch.from_numpy(_planes(frames)).to(cuda), torch.from_numpy(logits).to(cuda), torch.from_numpy(gt).to(cuda)
    out = torch.full((n, s, 3 * s, 3), 7, dtype=torch.uint8, device=cuda)
    rc = L.lib().octseg_epoch_panels(L.ptr(f), L.ptr(z), L.ptr(g), n, s, 2, s, s, 4, L.ptr(rows), L.ptr(cols), L.ptr(ch), L.ptr(rgb), L.ptr(ids),
                                     L.ptr(out), None, L.stream_ptr())
    assert rc == 0, L.lib().octseg_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize('s', [24, 33])
def test_unaligned_base_pointers(cuda, s):
    """Every tensor off its vector alignment, straight through the C entry: same strips, nothing written beside them."""
    rng = np.random.default_rng(50 + s)
    n, hs, ws, classes = 2, 31, 24, ['Fibrous cap', 'Lumen', 'Lipid core']
    frames, gt, logits = _case(rng, n, s, hs, ws, 3)
    want, wlab = R.panels(frames, gt, _assemble(cuda, logits), classes, size=s)
    planes = _planes(frames)
    fbuf = torch.zeros(planes.size + 8, dtype=torch.float32, device=cuda)
    fbuf[1:1 + planes.size] = torch.from_numpy(planes).to(cuda).flatten()
    zbuf = torch.zeros(logits.size + 8, dtype=torch.float32, device=cuda)
    zbuf[3:3 + logits.size] = torch.from_numpy(logits).to(cuda).flatten()
    gbuf = torch.zeros(gt.size + 8, dtype=torch.uint8, device=cuda)
    gbuf[1:1 + gt.size] = torch.from_numpy(gt).to(cuda).flatten()
    out = torch.full((want.size + 8,), 7, dtype=torch.uint8, device=cuda)
    lab = torch.full((wlab.size + 8,), 7, dtype=torch.uint8, device=cuda)
    rows, cols = _tables(cuda, hs, ws, s)
    ch = torch.tensor([R.CLASS_IDS[c] - 1 for c in classes], dtype=torch.int32, device=cuda)
    rgb = torch.tensor([R.CLASS_COLORS_RGB[c] for c in classes], dtype=torch.uint8, device=cuda)
    ids = torch.tensor([R.CLASS_IDS[c] for c in classes], dtype=torch.uint8, device=cuda)
    P = L.C.c_void_p
    rc = L.lib().octseg_epoch_panels(P(fbuf.data_ptr() + 4), P(zbuf.data_ptr() + 12), P(gbuf.data_ptr() + 1), n, s, 3, hs, ws, 4, L.ptr(rows),
                                     L.ptr(cols), L.ptr(ch), L.ptr(rgb), L.ptr(ids), P(out.data_ptr() + 3), P(lab.data_ptr() + 1), L.stream_ptr())
    assert rc == 0, L.lib().octseg_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(out[3:3 + want.size].cpu().numpy().reshape(want.shape), want)
    assert np.array_equal(lab[1:1 + wlab.size].cpu().numpy().reshape(wlab.shape), wlab)
    assert (out[:3] == 7).all() and (out[3 + want.size:] == 7).all() and (lab[:1] == 7).all() and (lab[1 + wlab.size:] == 7).all()


def test_abi_refuses_bad_arguments(cuda):
    lib, p, st = L.lib(), L.ptr, L.stream_ptr()
    n, s = 1, 8
    f = torch.zeros((n, 3, s, s), dtype=torch.float32, device=cuda)
    z = torch.zeros((n, 16, s, s), dtype=torch.float32, device=cuda)
    g = torch.zeros((n, s, s, 4), dtype=torch.uint8, device=cuda)
    idx = torch.arange(s, dtype=torch.int32, device=cuda)
    ch = torch.zeros((16,), dtype=torch.int32, device=cuda)
    rgb = torch.zeros((16, 3), dtype=torch.uint8, device=cuda)
    ids = torch.zeros((16,), dtype=torch.uint8, device=cuda)
    out = torch.full((n, s, 3 * s, 3), 9, dtype=torch.uint8, device=cuda)
    lab = torch.full((n, 2, s, s), 9, dtype=torch.uint8, device=cuda)
    BAD_SHAPE, BAD_ARG = -1, -5

    def call(frames=f, logits=z, gt=g, N=n, S=s, C=2, hs=s, ws=s, sc=4, rows=idx, cols=idx, chs=ch, col=rgb, cid=ids, o=out, lb=lab):
        return lib.octseg_epoch_panels(p(frames), p(logits), p(gt), N, S, C, hs, ws, sc, p(rows), p(cols), p(chs), p(col), p(cid), p(o), p(lb), st)

    for kw in ({'frames': None}, {'logits': None}, {'gt': None}, {'rows': None}, {'cols': None}, {'chs': None}, {'col': None}, {'cid': None},
               {'o': None}):
        assert call(**kw) == BAD_ARG, kw
        assert b'null' in lib.octseg_last_error()
    for kw in ({'N': 0}, {'S': 0}, {'S': -3}, {'C': 0}, {'C': 17}, {'hs': 0}, {'ws': -1}, {'sc': 0}):
        assert call(**kw) == BAD_SHAPE, kw
    torch.cuda.synchronize()
    assert (out == 9).all() and (lab == 9).all()                 # nothing was launched
    assert call(C=16) == 0 and call(lb=None) == 0
    torch.cuda.synchronize()
    assert (out[..., :s, :] == 0).all() and (out[..., s:, :] == 128).all()
    # the Python wrapper refuses what the kernel cannot take
    with pytest.raises(ValueError):
        postprocess.epoch_panels(f, z[:, :2], g.float(), ['Lumen', 'Fibrous cap'])
    with pytest.raises(ValueError):
        postprocess.epoch_panels(f, z[:, :3], g, ['Lumen', 'Fibrous cap'])            # one logit plane per class
    with pytest.raises(ValueError):
        postprocess.epoch_panels(f.double(), z[:, :1], g, ['Lumen'])
    with pytest.raises(ValueError):
        postprocess.epoch_panels(f, z[:, :1], g[..., :2], ['Lipid core'])             # needs channel 2
    with pytest.raises(ValueError):
        postprocess.epoch_panels(f, z[:, :1], g, ['Thrombus'])
    with pytest.raises(ValueError):
        postprocess.epoch_panels(f[:, :, :, :4], z[:, :1, :, :4], g, ['Lumen'])       # frames must be square


# ---- end to end: the vis/ tree through the model and through fit()
def _vis_tree(root, rng, sizes, names):
    """<root>/vis/img/<name>.png + <root>/vis/mask/<name>.tiff; returns {name: (bgr uint8 [h,w,3], mask uint8 [h,w,4])}."""
    os.makedirs(os.path.join(root, 'vis', 'img'))
    os.makedirs(os.path.join(root, 'vis', 'mask'))
    out = {}
    for name, (h, w) in zip(names, sizes):
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        m = rng.choice(np.array([0, 1, 254, 255], np.uint8), size=(-(-h // 8), -(-w // 8), 4), p=[0.3, 0.1, 0.1, 0.5])
        m = np.ascontiguousarray(np.repeat(np.repeat(m, 8, axis=0), 8, axis=1)[:h, :w])
        Image.fromarray(rgb).save(os.path.join(root, 'vis', 'img', f'{name}.png'))
        Image.fromarray(m, mode='RGBA').save(os.path.join(root, 'vis', 'mask', f'{name}.tiff'))
        out[name] = (np.ascontiguousarray(rgb[:, :, ::-1]), m)
    return out


def test_dump_end_to_end(cuda, tmp_path, monkeypatch):
    from oct_segmentation_amd.model import OCTSegmentationModel
    monkeypatch.chdir(tmp_path)      # relative paths, as the reference runs: vis_mask_path's string handling never sees the temporary folder's name
    rng = np.random.default_rng(21)
    classes, s, names = ['Lumen', 'Lipid core'], 64, ['a_first', 'b_second']
    data = 'data'
    src = _vis_tree(data, rng, [(80, 72), (64, 64)], names)
    with open(os.path.join(data, 'vis', 'img', 'notes.txt'), 'w') as f:      # not matched by the reference's pattern
        f.write('x')
    model = OCTSegmentationModel('unet', 'resnet18', 'unet_resnet18', 3, classes, data_dir=data, input_size=s, device=cuda,
                                 compute_dtype=torch.float32, seed=5)
    model.eval()
    out_dir = 'images_per_epoch'
    written = model.log_predict_model_on_epoch(out_dir=out_dir, epoch=3)
    assert written == [os.path.join(out_dir, f'{n}_epoch_003.png') for n in names] and sorted(os.listdir(out_dir)) == sorted(map(os.path.basename, written))
    assert not model.training and model.last_vis_labels == {}
    resized = [ingest.resize_image_u8(torch.from_numpy(src[n][0][None]).to(cuda), s)[0].cpu().numpy() for n in names]     # [3,S,S] f32 BGR
    frames = np.stack([r.transpose(1, 2, 0) for r in resized])                                                              # NHWC, as predict takes
    pred = model.predict(frames, 'cuda')                                                                                     # same chunking: one batch of 2
    files = []
    for i, n in enumerate(names):
        im = Image.open(written[i])
        assert im.mode == 'RGB'
        arr = np.asarray(im)
        assert arr.shape == (s, 3 * s, 3)
        assert np.array_equal(arr[:, :s], frames[i].astype(np.uint8)[:, :, ::-1])
        color_gt, color_pred, _, _ = R.paint(R.resize_nearest(src[n][1], s), pred[i], classes)
        assert np.array_equal(arr[:, s:2 * s], color_gt)
        assert np.array_equal(arr[:, 2 * s:], color_pred)
        assert (color_gt != 128).any()
        files.append(arr)
    # a second call reads no file again: the sources are gone
    for n in names:
        os.remove(os.path.join(data, 'vis', 'img', f'{n}.png'))
        os.remove(os.path.join(data, 'vis', 'mask', f'{n}.tiff'))
    model.save_wandb_media = True
    again = model.log_predict_model_on_epoch(out_dir=out_dir, epoch=4)
    assert again == [os.path.join(out_dir, f'{n}_epoch_004.png') for n in names] and len(os.listdir(out_dir)) == 4
    for i, n in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(again[i])), files[i])
        _, _, label_pred, label_gt = R.paint(R.resize_nearest(src[n][1], s), pred[i], classes)
        assert model.last_vis_labels[n].dtype == np.uint8
        assert np.array_equal(model.last_vis_labels[n], np.stack([label_pred, label_gt]))
    # another tree (the cache is keyed by data_dir): a frame without its mask, then a mask with too few channels
    bad = 'bad'
    _vis_tree(bad, rng, [(64, 64)], ['c'])
    os.remove(os.path.join(bad, 'vis', 'mask', 'c.tiff'))
    model.data_dir = bad
    with pytest.raises(FileNotFoundError) as e:
        model.log_predict_model_on_epoch(out_dir=out_dir, epoch=5)
    assert os.path.join(bad, 'vis', 'img', 'c.png') in str(e.value) and os.path.join(bad, 'vis', 'mask', 'c.tiff') in str(e.value)
    Image.fromarray(np.full((64, 64), 255, np.uint8)).save(os.path.join(bad, 'vis', 'mask', 'c.tiff'))      # one channel; 'Lipid core' needs three
    with pytest.raises(ValueError):
        model.log_predict_model_on_epoch(out_dir=out_dir, epoch=5)
    assert len(os.listdir(out_dir)) == 4


def test_fit_dumps_on_the_interval(cuda, tmp_path, monkeypatch):
    from oct_segmentation_amd.config import load_config
    from oct_segmentation_amd.train import fit
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(22)
    data = 'data'
    _vis_tree(data, rng, [(64, 64), (48, 56)], ['a', 'b'])
    cfg = load_config('train', ['architecture=unet', 'encoder=resnet18', 'epochs=3', 'input_size=64', 'batch_size=2', 'lr=0.001',
                                'compute_dtype=fp32', 'use_augmentation=false', 'img_save_interval=2'])
    cfg['classes'], cfg['data_dir'] = ['Lumen'], data
    batches = [tuple(t.to(cuda) for t in make_batch(2, 1, 64, seed=1))]
    d = 'run'
    model, hist = fit(cfg, batches, val_batches=batches, device=cuda, model_dir=d)
    assert len(hist) == 3 and model.epoch == 3 and model.data_dir == data and model.img_save_interval == 2
    assert sorted(os.listdir(os.path.join(d, 'images_per_epoch'))) == ['a_epoch_002.png', 'b_epoch_002.png']
    assert np.asarray(Image.open(os.path.join(d, 'images_per_epoch', 'a_epoch_002.png'))).shape == (64, 192, 3)
    # nothing without a validation loop, nothing (not even the folder) with the interval off
    d2 = 'no_val'
    fit(dict(cfg, epochs=1, img_save_interval=1), batches, val_batches=None, device=cuda, model_dir=d2)
    assert os.listdir(os.path.join(d2, 'images_per_epoch')) == []
    d3 = 'off'
    fit(dict(cfg, epochs=1, img_save_interval=None), batches, val_batches=batches, device=cuda, model_dir=d3)
    assert not os.path.exists(os.path.join(d3, 'images_per_epoch')) and os.path.exists(os.path.join(d3, 'metrics.csv'))
