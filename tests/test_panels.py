"""The per-epoch sample strips without a GPU: the host restatement (tests/panels_ref.py) against the reference's own run
(tests/golden/epoch_panel.npz, made by tests/golden/make_epoch_panel_fixture.py), the reference's mask-path string handling, and the parts of
the wiring that need no device."""
import os
import re
import types

import numpy as np
import pytest

import panels_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PIN = os.path.join(HERE, 'golden', 'epoch_panel.npz')


def load_pin():
    z = np.load(PIN)
    return {k: z[k] for k in z.files}


def test_restatement_equals_the_reference_run():
    z = load_pin()
    classes = [str(c) for c in z['classes']]
    assert classes == ['Vasa vasorum', 'Lumen', 'Fibrous cap'] and z['frames_bgr'].shape == (2, 24, 24, 3)
    got, labels = R.panels(z['frames_bgr'], z['gt'], z['pred'], classes)
    # the reference hands cv2.imwrite a BGR array: the written file decodes, as RGB, to every pixel reversed
    assert np.array_equal(got, z['res_bgr'][..., ::-1])
    assert np.array_equal(labels[:, 0], z['label_pred']) and np.array_equal(labels[:, 1], z['label_gt'])
    assert [os.path.basename(str(p)) for p in z['paths']] == [f'{s}_epoch_{int(z["epoch"]):03d}.png' for s in z['stems']]
    assert os.path.dirname(str(z['paths'][0])) == 'models/fixture/images_per_epoch'


def test_fixture_discriminates_the_rules():
    """What the pin must be able to tell apart: == 255 from != 0, the list order, the class's own channel."""
    z = load_pin()
    classes = [str(c) for c in z['classes']]
    want = z['res_bgr'][..., ::-1]
    chans = [R.CLASS_IDS[c] - 1 for c in classes]
    sel = z['gt'][..., chans]
    assert set(np.unique(z['gt'])) == {0, 1, 128, 254, 255}
    assert ((sel != 0) & (sel != 255)).any()                      # a `!= 0` test paints more
    nonzero = np.where(z['gt'] != 0, 255, 0).astype(np.uint8)
    assert not np.array_equal(R.panels(z['frames_bgr'], nonzero, z['pred'], classes)[0], want)
    assert ((sel == 255).sum(-1) >= 2).any() and (z['pred'].sum(-1) >= 2).any()      # classes overlap in both panes
    assert not np.array_equal(R.panels(z['frames_bgr'], z['gt'], z['pred'], classes[::-1])[0][:, :, 24:48], want[:, :, 24:48])
    assert chans != list(range(len(classes)))                     # ground-truth channel != prediction channel
    assert os.path.getsize(PIN) < 64 * 1024


def test_nearest_index_is_resizenn():
    assert R.nearest_index(8, 16).tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7]
    assert R.nearest_index(37, 33)[-1] <= 36 and R.nearest_index(29, 33)[-1] == 28
    from oct_segmentation_amd.predict import cv2_nearest_index
    for src, dst in ((37, 33), (29, 33), (8, 16), (20, 20), (80, 64), (72, 64), (1000, 512)):
        assert np.array_equal(R.nearest_index(src, dst), cv2_nearest_index(src, dst)), (src, dst)


def test_vis_mask_path_keeps_the_reference_string_handling():
    from oct_segmentation_amd.model import vis_mask_path
    assert vis_mask_path('data/cv/fold_1/vis/img/frame_001.png') == 'data/cv/fold_1/vis/mask/frame_001.tiff'
    # every 'img' is replaced, the one in the stem too
    assert vis_mask_path('data/vis/img/img_007.png') == 'data/vis/mask/mask_007.tiff'
    # the path is cut at its FIRST dot, a folder's included
    assert vis_mask_path('runs/v1.2/vis/img/a.png') == 'runs/v1.tiff'


def test_dump_returns_at_once_without_a_vis_folder(tmp_path):
    from oct_segmentation_amd.model import OCTSegmentationModel
    for data_dir in (None, str(tmp_path), os.path.join(tmp_path, 'missing')):
        stand_in = types.SimpleNamespace(data_dir=data_dir)       # nothing else may be touched
        assert OCTSegmentationModel.log_predict_model_on_epoch(stand_in) == []
    os.makedirs(os.path.join(tmp_path, 'vis', 'mask'))           # vis/ without vis/img
    assert OCTSegmentationModel.log_predict_model_on_epoch(types.SimpleNamespace(data_dir=str(tmp_path))) == []
    assert sorted(os.listdir(tmp_path)) == ['vis']


@pytest.mark.parametrize('bad', [0, -1, 1.5, '2', True])
def test_fit_rejects_a_bad_img_save_interval(bad):
    from oct_segmentation_amd.train import fit
    with pytest.raises(ValueError, match='img_save_interval'):
        fit({'img_save_interval': bad}, [])                       # before anything else of the config is looked at


def test_header_and_binding_declare_the_entry_point():
    from oct_segmentation_amd import _lib as L
    header = open(os.path.join(ROOT, 'include', 'octseg.h')).read()
    m = re.search(r'^int octseg_epoch_panels\(([^;]*)\);', header, re.M)
    assert m, 'octseg_epoch_panels is not declared in include/octseg.h'
    assert len(m.group(1).split(',')) == len(L.SYMBOLS['octseg_epoch_panels'][1]) == 17
    assert 'model.py:208-271' in header and header.count('octseg_epoch_panels') >= 2      # the table row and the declaration
