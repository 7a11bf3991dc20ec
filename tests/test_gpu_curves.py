"""The logit histograms on the GPU: octseg_logit_histogram against tests/curves_ref.py on every case of tests/curves_cases.py (whole histograms by
equality: the CPU test pins that the f32 and the float64 rule bin every pixel of every case alike), the k = 128 counts against the Dice kernel's,
apply_thresholds through octseg_mask_assemble, and the tool and predict's thresholds key end to end on a small network."""
import json
import os

import numpy as np
import pytest
import torch

import curves_cases as CC
import curves_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import curves

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', CC.CASES, ids=CC.IDS)
def test_histogram_equals_the_reference(cuda, case):
    z, t = CC.inputs(case)
    N, C_, H, W = case.shape
    zd, td = torch.from_numpy(np.array(z)).to(cuda), torch.from_numpy(np.array(t)).to(cuda)
    out = torch.full((N, C_, 2, 256), -1, dtype=torch.int32, device=cuda)                # the call clears it on the stream
    got = curves.logit_histograms(zd, td, out=out)
    assert got is out
    hist = out.cpu().numpy().astype(np.int64)
    assert np.array_equal(hist, CC.reference(case))
    assert (hist.sum(axis=(2, 3)) == H * W).all()
    fresh = curves.logit_histograms(zd, td)
    assert fresh.dtype == torch.int32 and tuple(fresh.shape) == (N, C_, 2, 256) and torch.equal(fresh, out)


def test_unaligned_views_count_alike(cuda):
    """Logits and target at addresses that are 4, 8 and 12 bytes off a 16-byte boundary, congruent and not: the head / 16-byte / tail split and the
    4-byte path give the histogram of the same values in aligned tensors."""
    rng = np.random.default_rng(21)
    shape = (2, 2, 31, 41)
    n = int(np.prod(shape))
    z, t = CC.draw_logits(rng, shape), CC.draw_target(rng, shape)
    want = torch.from_numpy(R.histogram(z, t)).to(cuda)
    zb, tb = torch.zeros(n + 8, device=cuda), torch.zeros(n + 8, device=cuda)
    for oz, ot in ((1, 1), (2, 2), (3, 3), (0, 1), (3, 2)):
        zv, tv = zb[oz:oz + n].view(shape), tb[ot:ot + n].view(shape)
        zv.copy_(torch.from_numpy(z))
        tv.copy_(torch.from_numpy(t))
        assert zv.data_ptr() % 16 == 4 * oz and zv.is_contiguous()
        assert torch.equal(curves.logit_histograms(zv, tv).long(), want), (oz, ot)


def test_k128_counts_equal_the_dice_kernels_bit_for_bit(cuda):
    from oct_segmentation_amd.model import OCTSegmentationModel
    g = torch.Generator().manual_seed(3)
    z = (torch.randn((3, 2, 64, 64), generator=g) * 3).to(cuda)
    z[0, 1, :4] = torch.tensor([0.0, -0.0, 1e-9, -1e-9], device=cuda).repeat(16)          # the threshold itself: whatever the one sigmoid says
    z[2, 0, 60:] = torch.tensor([1e-9, 0.0, -1e-9, -0.0], device=cuda).repeat(16)
    t = (torch.rand((3, 2, 64, 64), generator=g) < 0.4).float().to(cuda)
    net = OCTSegmentationModel('unet', 'resnet18', 'tiny', 3, ['Lipid core', 'Fibrous cap'], device=cuda, compute_dtype=torch.float32).model
    net.eval()
    _, stats = net.dice(net._plan(3, 64, 64), z, t)                                       # int64 [3, 2, 4]: tp, fp, fn, tn
    hist = curves.logit_histograms(z, t).long()
    tp, fp = hist[:, :, 1, 128:].sum(-1), hist[:, :, 0, 128:].sum(-1)
    fn, tn = hist[:, :, 1, :128].sum(-1), hist[:, :, 0, :128].sum(-1)
    assert torch.equal(torch.stack([tp, fp, fn, tn], dim=-1), stats)
    assert int(hist[0, 1, :, 127].sum()) >= 64 and int(tp.sum()) > 0 and int(fp.sum()) > 0   # the +-0 and +-1e-9 pixels sit in bin 127, not set
    per_frame = curves._curves(hist.cpu().numpy())
    assert np.array_equal(np.stack([per_frame[k][..., 128] for k in ('tp', 'fp', 'fn', 'tn')], axis=-1), stats.cpu().numpy())


@pytest.mark.parametrize('t', [0.25, 0.5, 0.8])
def test_mask_assemble_after_apply_thresholds_cuts_at_t(cuda, t):
    rng = np.random.default_rng(31)
    shape = (2, 2, 37, 53)
    z = CC.draw_logits(rng, shape)
    cut = np.log(t / (1 - t))
    z[np.abs(z.astype(np.float64) - cut) < 1e-3] = CC.MID                                  # MID = -1.76 is itself 0.6 away from every cut here
    assert (np.abs(z.astype(np.float64) - cut) >= 1e-3).all()
    want = (R.sigmoid64(z) > t)
    zd = torch.from_numpy(z).to(cuda)
    curves.apply_thresholds(zd, [1], [t])
    assert torch.equal(zd[:, 0].cpu(), torch.from_numpy(z[:, 0]))                          # the other channel is left alone
    for ch, ref in ((1, want[:, 1]), (0, R.sigmoid64(z[:, 0]) > 0.5)):
        out = torch.full((2, 37, 53, 3), 7.0, dtype=torch.float32, device=cuda)
        L.check(L.lib().octseg_mask_assemble(L.ptr(zd), 2, 2, 37, 53, ch, L.ptr(out), 37, 53, 3, 2, None, None, L.stream_ptr()))
        assert np.array_equal(out[..., 2].cpu().numpy(), ref.astype(np.float32))
        assert 0 < ref.mean() < 1


def test_a_refused_call_leaves_hist_untouched(cuda):
    z = torch.zeros((2, 1, 8, 8), device=cuda)
    hist = torch.full((2, 1, 2, 256), 5, dtype=torch.int32, device=cuda)
    lib = L.lib()
    for args in ((None, L.ptr(z), 2, 1, 8, 8), (L.ptr(z), None, 2, 1, 8, 8), (L.ptr(z), L.ptr(z), 0, 1, 8, 8), (L.ptr(z), L.ptr(z), 2, 1, 8, -8),
                 (L.ptr(z), L.ptr(z), 2, 1, 65536, 32768), (L.ptr(z), L.ptr(z), 65536, 1, 8, 8)):
        assert lib.octseg_logit_histogram(*args, L.ptr(hist), L.stream_ptr()) in (-1, -5)
    torch.cuda.synchronize()
    assert (hist == 5).all()
    with pytest.raises(ValueError, match='differ'):
        curves.logit_histograms(z, torch.zeros((2, 1, 8, 4), device=cuda))
    with pytest.raises(ValueError, match='contiguous'):
        curves.logit_histograms(z.expand(2, 2, 8, 8), z.expand(2, 2, 8, 8))
    with pytest.raises(ValueError, match='out must'):
        curves.logit_histograms(z, z, out=torch.zeros((2, 1, 2, 256), dtype=torch.int64, device=cuda))
    assert (hist == 5).all()


# ------------------------------------------------------------------ end to end
CLASSES = ['Lipid core', 'Fibrous cap']


@pytest.fixture(scope='module')
def fold(cuda, tmp_path_factory):
    """A FC_LC checkpoint (random-init U-Net / resnet18 at 64 x 64, two classes) and a fold directory of five frames of two source sizes."""
    from PIL import Image
    from oct_segmentation_amd.model import OCTSegmentationModel
    root = tmp_path_factory.mktemp('curves')
    model_dir = str(root / 'models' / 'FC_LC')
    os.makedirs(model_dir)
    m = OCTSegmentationModel('unet', 'resnet18', 'unet_resnet18', 3, CLASSES, device=cuda, seed=41, compute_dtype=torch.float32)
    m.save_checkpoint(os.path.join(model_dir, 'weights.ckpt'))
    with open(os.path.join(model_dir, 'config.json'), 'w') as f:
        json.dump({'model_name': 'unet_resnet18', 'architecture': 'unet', 'encoder': 'resnet18', 'input_size': 64, 'classes': CLASSES}, f)
    data = str(root / 'fold' / 'test')
    os.makedirs(os.path.join(data, 'img'))
    os.makedirs(os.path.join(data, 'mask'))
    rng = np.random.default_rng(9)
    for k, (h, w) in enumerate([(80, 80), (100, 90), (80, 80), (100, 90), (80, 80)]):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(data, 'img', f'f{k:02d}.png'))
        mask = rng.choice(np.array([0, 255], np.uint8), size=(h, w, 4))
        Image.fromarray(mask, mode='RGBA').save(os.path.join(data, 'mask', f'f{k:02d}.tiff'))
    return model_dir, data


def test_tool_writes_curves_whose_k128_counts_are_the_models_validation_counts(cuda, fold, tmp_path):
    from oct_segmentation_amd.dataset import DeviceBatches, OCTDataset
    from oct_segmentation_amd.metrics import _metrics_from_numpy
    from oct_segmentation_amd.predict import load_model
    model_dir, data = fold
    out = str(tmp_path / 'out')
    assert curves.main([f'model_dir={model_dir}', f'data_dir={data}', 'batch_size=3', 'compute_dtype=fp32', f'save_dir={out}']) == 0
    assert sorted(os.listdir(out)) == ['curves.json', 'curves.png'] and os.path.getsize(os.path.join(out, 'curves.png')) > 10000
    rep = json.load(open(os.path.join(out, 'curves.json')))
    assert rep['frames'] == 5 and list(rep['classes']) == CLASSES
    # the model's own validation: the same batches through validation_step, the Dice kernel's counts
    model, cfg = load_model(model_dir, 'cuda', torch.float32)
    stats = []
    for batch in DeviceBatches(OCTDataset(data, CLASSES, 64), 3, shuffle=False, device=cuda):
        with torch.no_grad():
            stats.append(model._step(batch)[2])                                           # what validation_step records
    stats = torch.cat(stats).cpu().numpy()                                                # [5, 2, 4], frames in the batches' order
    order = ['f00', 'f02', 'f01', 'f03', 'f04']                                           # batch [f00, f01, f02]: the two 80 x 80 frames together
    pooled = stats.sum(axis=0)
    want = _metrics_from_numpy(pooled, np.float32(0))
    for c, cls in enumerate(CLASSES):
        e = rep['classes'][cls]
        assert [e['curves'][k][128] for k in ('tp', 'fp', 'fn', 'tn')] == pooled[c].tolist()
        assert e['dice_at_half'] == float(want['dice'][c]) and e['curves']['dice'][128] == e['dice_at_half']
        assert e['pixels'] == 5 * 64 * 64 and 0 < e['positive_pixels'] < e['pixels']
        assert e['dice_at_best'] >= e['dice_at_half'] and 1 <= e['best_k'] <= 255
        assert 0.0 <= e['auc'] <= 1.0 and 0.0 <= e['ap'] <= 1.0 and 0.0 <= e['ece'] <= 1.0
        frame_dice = _metrics_from_numpy(stats[:, c], np.float32(0))['dice']
        assert list(e['slices']) == order                                                 # the names follow the rows
        assert [e['slices'][n]['dice_at_half'] for n in order] == [float(d) for d in frame_dice]


def test_predict_thresholds_equals_cutting_the_logits_at_the_shifted_value(cuda, fold, tmp_path):
    from PIL import Image
    from oct_segmentation_amd import predict, vote
    from oct_segmentation_amd.model import CLASS_IDS
    model_dir, data = fold
    models = os.path.dirname(model_dir)
    paths = sorted(predict._image_paths(os.path.join(data, 'img')))[:3:2]                  # f00, f02: one source size
    frames = predict._frames_on_device(paths, [96, 96], 'cuda')
    kw = dict(device='cuda', compute_dtype=torch.float32, batch_size=2)
    plain = predict.segment_stack(frames, [96, 96], CLASSES, models, device_preprocess=True, **kw)
    # the logits, dumped: the same eager forward (bit-reproducible); thresholds at the 30 % and 70 % quantile of each class's probabilities,
    # so that whatever a random network puts out, the cut moves pixels
    net, cfg = predict.load_model(model_dir, 'cuda', torch.float32)
    z = net.predict_logits(predict._resize_frames_on_device(frames, 0, 2, 64))
    th = {name: float(np.clip(torch.sigmoid(z[:, predict.MODELS_META[name]['index']].flatten().double()).quantile(q).item(), 0.01, 0.99))
          for name, q in (('Fibrous cap', 0.7), ('Lipid core', 0.3))}
    got = predict.segment_stack(frames, [96, 96], CLASSES, models, device_preprocess=True, thresholds=th, **kw)
    assert torch.equal(predict.segment_stack(frames, [96, 96], CLASSES, models, device_preprocess=True, **kw), plain)      # absent: as before
    rows = torch.from_numpy(predict.cv2_nearest_index(64, 96)).to(cuda)
    want = torch.zeros_like(plain)
    for name, t in th.items():                                                             # the engine's cut of the logits at the shifted value
        ch, c = predict.MODELS_META[name]['index'], CLASS_IDS[name] - 1
        shifted = z.clone()
        shifted[:, ch] -= float(np.float32(np.log(t / (1 - t))))
        L.check(L.lib().octseg_mask_assemble(L.ptr(shifted), 2, 2, 64, 64, ch, L.ptr(want), 96, 96, 4, c, L.ptr(rows), L.ptr(rows), L.stream_ptr()))
        cut = (torch.sigmoid(z[:, ch].double()) > t).float()                               # ... which is p > t but for pixels within rounding of t
        assert (want[..., c] != cut[:, rows.long()][:, :, rows.long()]).float().mean() < 1e-3
    assert torch.equal(got, want) and not torch.equal(got, plain)
    voted = vote.segment_stack_voted(frames, [96, 96], CLASSES, models, tta='none', folds=False, thresholds=th, **kw)
    assert torch.equal(voted.stack, want)
    # the command line: thresholds as a dict and as the tool's curves.json
    src = tmp_path / 'in'
    src.mkdir()
    for p in paths:
        Image.open(p).save(str(src / os.path.basename(p)))
    common = [f'data_dir={src}', 'output_size=[96,96]', 'compute_dtype=fp32', f'classes={json.dumps(CLASSES)}', f'models_dir={models}']
    with pytest.raises(ValueError, match='unknown class'):
        predict.main(common + [f'save_dir={tmp_path / "bad"}', 'thresholds={"Media": 0.4}'])
    with pytest.raises(ValueError, match=r'\(0, 1\)'):
        predict.main(common + [f'save_dir={tmp_path / "bad"}', 'thresholds={"Lumen": 1.5}'])
    a, b = tmp_path / 'a', tmp_path / 'b'
    assert predict.main(common + [f'save_dir={a}']) == 0
    assert predict.main(common + [f'save_dir={b}', f'thresholds={json.dumps(th)}']) == 0
    names = [os.path.basename(p).split('.')[0] for p in paths]
    assert sorted(os.listdir(b)) == sorted(f'{n}_{k}.png' for n in names for k in ('mask', 'overlay'))
    differ = [n for n in names if not np.array_equal(np.asarray(Image.open(a / f'{n}_mask.png')), np.asarray(Image.open(b / f'{n}_mask.png')))]
    assert differ
