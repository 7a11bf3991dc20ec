"""The per-epoch sample strips as the REFERENCE's own code paints them (build container only; /root/reference never travels).

`log_predict_model_on_epoch` (src/models/smp/model.py:208-271) is loaded with importlib straight from /root/reference and EXECUTED, unmodified,
on a bare object; nothing of its text is copied.  The module imports cv2, tifffile, wandb, pytorch_lightning and segmentation_models_pytorch
at the top, none of which is installed here, so they are stubbed in `sys.modules`:
  * cv2 -- `imread` hands out this script's seeded BGR frame for the path, `resize` is an IDENTITY that insists on an input already at
    (S, S) (so only the reference's painting and stacking are pinned, not cv2's resampling: tests/test_ingest.py pins that), `imwrite`
    captures the array and the path, `cvtColor(COLOR_BGR2RGB)` reverses the last axis;
  * tifffile -- `imread` hands out the seeded 4-channel uint8 mask for the path;
  * wandb -- `Image` records its `masks` argument (the two label maps), `log` is a no-op;
  * pytorch_lightning -- `LightningModule` = object; segmentation_models_pytorch -- an empty module.
The object's `predict` returns a seeded 0 / 1 mask whatever it is handed: at the reference's HEAD the call passes a CHW frame that the
real `predict` transposes again, which the stub sidesteps.

The data: S = 24, two frames, classes ['Vasa vasorum', 'Lumen', 'Fibrous cap'] (list order differs from channel order, and the ground-truth
channel of a class differs from its prediction channel), ground-truth samples drawn from {0, 1, 128, 254, 255} in blocks (so `!= 0` instead of
`== 255` fails), predictions in blocks; the regions of different classes overlap, so the overwrite order shows.
Output: tests/golden/epoch_panel.npz = the inputs and what reached imwrite / wandb.Image.  Data only.

    python tests/golden/make_epoch_panel_fixture.py
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = '/root/reference'
REF_MODEL = os.path.join(REF_ROOT, 'src', 'models', 'smp', 'model.py')
S = 24
CLASSES = ['Vasa vasorum', 'Lumen', 'Fibrous cap']
STEMS = ['frame_a', 'frame_b']
EPOCH = 7


def blocks(rng, values, p, shape, cell):
    """Values drawn per cell x cell block of an [S, S, channels] array."""
    h, w, c = shape
    coarse = rng.choice(np.asarray(values), size=(-(-h // cell), -(-w // cell), c), p=p)
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, cell, axis=0), cell, axis=1)[:h, :w])


def make_data():
    rng = np.random.default_rng(20240921)
    frames = rng.integers(0, 256, (len(STEMS), S, S, 3), dtype=np.uint8)                      # BGR, as cv2.imread returns
    gt = np.stack([blocks(rng, [0, 1, 128, 254, 255], [0.2, 0.1, 0.15, 0.15, 0.4], (S, S, 4), cell).astype(np.uint8)
                   for cell in (3, 5)])
    pred = np.stack([blocks(rng, [0, 1], [0.55, 0.45], (S, S, len(CLASSES)), cell).astype(np.float32) for cell in (4, 7)])
    return frames, gt, pred


def load_reference(state):
    cv2 = types.ModuleType('cv2')
    cv2.INTER_NEAREST, cv2.COLOR_BGR2RGB = 0, 4

    def imread(path):
        state['current'] = os.path.splitext(os.path.basename(path))[0]
        return state['frames'][state['current']].copy()

    def resize(src, dsize, interpolation=None):
        assert tuple(dsize) == (S, S) and src.shape[:2] == (S, S), 'the identity stub takes inputs already at (S, S)'
        return src.copy()

    def imwrite(path, img):
        state['written'][state['current']] = (path, np.array(img))
        return True

    cv2.imread, cv2.resize, cv2.imwrite = imread, resize, imwrite
    cv2.cvtColor = lambda img, code: np.ascontiguousarray(img[:, :, ::-1])
    tifffile = types.ModuleType('tifffile')
    tifffile.imread = lambda path: state['masks'][os.path.splitext(os.path.basename(path))[0]].copy()
    wandb = types.ModuleType('wandb')
    wandb.run = types.SimpleNamespace(summary={})
    wandb.log = lambda *a, **k: None

    def wandb_image(img, masks=None, caption=None):
        state['labels'][state['current']] = (np.array(masks['predictions']['mask_data']), np.array(masks['ground_truth']['mask_data']))
        return (img, caption)

    wandb.Image = wandb_image
    pl = types.ModuleType('pytorch_lightning')
    pl.LightningModule = object
    smp = types.ModuleType('segmentation_models_pytorch')
    sys.modules.update({'cv2': cv2, 'tifffile': tifffile, 'wandb': wandb, 'pytorch_lightning': pl, 'segmentation_models_pytorch': smp})
    sys.path.insert(0, REF_ROOT)          # the module imports src.data.utils and src.models.smp.utils
    spec = importlib.util.spec_from_file_location('reference_smp_model', REF_MODEL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    frames, gt, pred = make_data()
    state = {'frames': dict(zip(STEMS, frames)), 'masks': dict(zip(STEMS, gt)), 'preds': dict(zip(STEMS, pred)), 'written': {}, 'labels': {},
             'current': None}
    ref = load_reference(state)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'data', 'vis', 'img'))
        for stem in STEMS:                                   # the call globs for the files; their bytes are never read (imread is the stub)
            open(os.path.join(tmp, 'data', 'vis', 'img', f'{stem}.png'), 'w').close()
        obj = types.SimpleNamespace(data_dir=os.path.join(tmp, 'data'), input_size=S, classes=list(CLASSES), model_name='fixture', epoch=EPOCH,
                                    save_wandb_media=True, to_tensor_shape=ref.OCTSegmentationModel.to_tensor_shape,
                                    predict=lambda images, device: state['preds'][state['current']][None].copy())
        os.chdir(tmp)
        try:
            ref.OCTSegmentationModel.log_predict_model_on_epoch(obj)
        finally:
            os.chdir(cwd)
    assert sorted(state['written']) == sorted(STEMS) == sorted(state['labels'])
    res = np.stack([state['written'][s][1] for s in STEMS])
    lab_pred = np.stack([state['labels'][s][0] for s in STEMS])
    lab_gt = np.stack([state['labels'][s][1] for s in STEMS])
    assert res.dtype == np.uint8 and res.shape == (len(STEMS), S, 3 * S, 3)
    assert np.array_equal(lab_pred, lab_pred.astype(np.uint8)) and np.array_equal(lab_gt, lab_gt.astype(np.uint8))
    np.savez_compressed(os.path.join(HERE, 'epoch_panel.npz'), stems=np.array(STEMS), classes=np.array(CLASSES), epoch=np.int64(EPOCH),
                        frames_bgr=frames, gt=gt, pred=pred.astype(np.uint8), res_bgr=res, label_pred=lab_pred.astype(np.uint8),
                        label_gt=lab_gt.astype(np.uint8), paths=np.array([state['written'][s][0] for s in STEMS]))
    print('wrote epoch_panel.npz:', res.shape, [state['written'][s][0] for s in STEMS], os.path.getsize(os.path.join(HERE, 'epoch_panel.npz')), 'bytes')


if __name__ == '__main__':
    main()
