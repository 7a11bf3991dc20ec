"""CPU tests of the class-activation-map module: the float64 restatement tests/cam_ref.py on hand-made A, G with closed-form answers, the
metrics from integer counts against sklearn, the wrapper's refusals, config parsing, and file-name / CSV-row construction."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cam_ref as R  # noqa: E402

from oct_segmentation_amd import _lib as L  # noqa: E402
from oct_segmentation_amd import cam  # noqa: E402
from oct_segmentation_amd.engine import _TreeRef  # noqa: E402


def _rand(K=6, h=3, w=4, seed=0):
    rng = np.random.default_rng(seed)
    return np.abs(rng.standard_normal((K, h, w))), rng.standard_normal((K, h, w))


def test_ref_gradcam_constant_gradient_is_proportional_to_sum_of_activations():
    A, _ = _rand()
    G = np.full_like(A, 0.25)
    assert np.allclose(R.raw_map(A, G, 'GradCAM'), 0.25 * A.sum(axis=0), rtol=1e-13)
    # after scaling the constant drops out: the map of 0.25 equals the map of 3.0
    assert np.allclose(R.cam_map(A, G, 'GradCAM', 12), R.cam_map(A, np.full_like(A, 3.0), 'GradCAM', 12), atol=1e-12)


def test_ref_non_positive_gradient_gives_zero_maps():
    A, G = _rand(seed=1)
    G = -np.abs(G)
    G[0] = 0
    for method in ('LayerCAM', 'GradCAMElementWise', 'GradCAMPlusPlus'):
        assert (R.cam_map(A, G, method, 8) == 0).all(), method


def test_ref_dead_channel_contributes_nothing_in_xgradcam():
    A, G = _rand(seed=2)
    A[2] = 0
    keep = [0, 1, 3, 4, 5]
    assert np.allclose(R.raw_map(A, G, 'XGradCAM'), R.raw_map(A[keep], G[keep], 'XGradCAM'), rtol=1e-13, atol=1e-15)
    assert np.isfinite(R.cam_map(A, G, 'XGradCAM', 8)).all()


def test_ref_hirescam_and_layercam_closed_forms():
    A, G = _rand(seed=3)
    assert np.allclose(R.raw_map(A, G, 'HiResCAM'), np.einsum('khw,khw->hw', G, A))
    assert np.allclose(R.raw_map(A, G, 'LayerCAM'), np.einsum('khw,khw->hw', np.maximum(G, 0), A))
    assert np.allclose(R.raw_map(A, G, 'GradCAMElementWise'), np.maximum(G * A, 0).sum(0))
    g = G[0, 0, 0]
    one = R.raw_map(A[:1, :1, :1], G[:1, :1, :1], 'GradCAMPlusPlus')[0, 0]        # one channel, one pixel: w = max(g, 0) g^2 / (2 g^2 + A g^3 + 1e-6)
    a = A[0, 0, 0]
    assert one == pytest.approx(max(g, 0) * g * g / (2 * g * g + a * g ** 3 + 1e-6) * a)


def test_ref_one_pixel_map_is_all_zero():
    A, G = _rand(K=4, h=1, w=1, seed=4)
    for method in R.METHODS:
        m = R.cam_map(A, G, method, 32)
        assert m.shape == (32, 32) and (m == 0).all(), method


def test_ref_maps_span_zero_to_one_and_resize_is_identity_at_equal_size():
    A, G = _rand(K=8, h=5, w=5, seed=5)
    m = R.cam_map(A, G, 'HiResCAM', 40)
    assert m.min() == 0 and m.max() == pytest.approx(1.0, abs=1e-6)
    x = np.random.default_rng(0).random((7, 7))
    assert np.array_equal(R.resize_linear(x, 7), x)
    flat = np.full((3, 5), 0.7)
    assert np.allclose(R.resize_linear(flat, 16), 0.7)


@pytest.mark.parametrize('case', ['random', 'empty_pred', 'empty_gt', 'both_empty', 'full'])
def test_metrics_from_counts_equal_sklearn_micro(case):
    from sklearn.metrics import f1_score, jaccard_score, precision_score, recall_score
    rng = np.random.default_rng(11)
    pred = (rng.random((37, 41)) > 0.6).astype(np.uint8) * 255
    gt = (rng.random((37, 41)) > 0.5).astype(np.uint8) * 255
    if case in ('empty_pred', 'both_empty'):
        pred[:] = 0
    if case in ('empty_gt', 'both_empty'):
        gt[:] = 0
    if case == 'full':
        pred[:] = 255
    tp, p, t = int(((pred != 0) & (gt != 0)).sum()), int((pred != 0).sum()), int((gt != 0).sum())
    assert (tp, p, t) == R.counts(pred, gt)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want = {'Dice': f1_score(gt, pred, average='micro'), 'IoU': jaccard_score(gt, pred, average='micro'),
                'Precision': precision_score(gt, pred, average='micro'), 'Recall': recall_score(gt, pred, average='micro')}
    got = cam.metrics_from_counts(tp, p, t)
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-12, abs=1e-15), k
    assert got['F1'] == got['Dice'] and got == pytest.approx(R.metrics(tp, p, t))


def _fake_model(arch='unet', encoder='resnet18', dtype_code=L.F32):
    names = [f'encoder.layer4.{b}.conv1.weight' for b in (0, 1)] + ['encoder.layer3.0.conv1.weight', 'decoder.blocks.0.conv1.0.weight']
    if not encoder.startswith('resnet'):
        names = ['encoder.s4.b1.conv1.conv.weight']
    net = SimpleNamespace(param_table=[{'name': n} for n in names], arch=arch, encoder_name=encoder, dtype_code=dtype_code, classes=2,
                          device=torch.device('cpu'))
    net.encoder = _TreeRef(net, 'encoder')
    return SimpleNamespace(model=net, _mean=[0, 0, 0], _std=[1, 1, 1])


def test_wrapper_refusals():
    m = _fake_model()
    good = [m.model.encoder.layer4[-1]]
    p = cam.CAMProcessor(m, 'cuda', 'XGradCAM', good)
    assert p.method_id == 4 and list(cam.CAM_METHODS) == ['GradCAM', 'HiResCAM', 'GradCAMElementWise', 'GradCAMPlusPlus', 'XGradCAM', 'AblationCAM',
                                                         'EigenCAM', 'EigenGradCAM', 'LayerCAM']
    with pytest.raises(ValueError, match='Invalid CAM method: ScoreCAM'):
        cam.CAMProcessor(m, 'cuda', 'ScoreCAM', good)
    for name, word in (('AblationCAM', 're-executed'), ('EigenCAM', 'LAPACK'), ('EigenGradCAM', 'LAPACK')):
        with pytest.raises(NotImplementedError, match=word):
            cam.CAMProcessor(m, 'cuda', name, good)
    for bad in (None, [], [m.model.encoder.layer4[0]], [m.model.encoder.layer3[-1]], good * 2):
        with pytest.raises(NotImplementedError, match='target_layers'):
            cam.CAMProcessor(m, 'cuda', 'GradCAM', bad)
    assert cam.CAMProcessor(m, 'cuda', 'GradCAM', [m.model.encoder.layer4[-1].ref()]).method_id == 0     # the _LayerRef form of the same position
    img = np.zeros((32, 32, 3), np.uint8)
    tg = p.get_targets(1, np.zeros((32, 32), np.float32))
    assert tg[0].category == 1 and isinstance(tg[0], cam.SemanticSegmentationTarget)
    for kw in ({'eigen_smooth': True}, {'aug_smooth': True}):
        with pytest.raises(NotImplementedError, match='smooth'):
            p.extract_activation_map(img, tg, **kw)
    # host tensors are refused by the device-side calls, as in postprocess.py
    with pytest.raises(ValueError, match='CUDA'):
        p.activations(torch.zeros(1, 3, 32, 32), [0], torch.zeros(1, 32, 32))
    with pytest.raises(ValueError, match='CUDA'):
        p.maps_from(torch.zeros(1, 1, 1, 8), torch.zeros(1, 1, 1, 8), 32)
    with pytest.raises(ValueError, match='CUDA'):
        cam.overlay_on_device(torch.zeros(1, 3, 32, 32), torch.zeros(1, 32, 32))
    with pytest.raises(ValueError):
        p.extract_activation_map(torch.zeros(32, 32, 3), tg)
    # hooks stay refused, and say where to go
    with pytest.raises(NotImplementedError, match='no per-layer activations') as e:
        m.model.encoder.layer4[-1].register_forward_hook(lambda *a: None)
    assert 'oct_segmentation_amd.cam' in str(e.value)


@pytest.mark.parametrize('arch,enc,dt,word', [
    ('fpn', 'resnet18', L.F32, 'dropout'), ('pspnet', 'resnet34', L.F32, 'never runs'), ('deeplabv3', 'resnet18', L.F32, 'parity'),
    ('deeplabv3plus', 'resnet50', L.BF16, 'parity'), ('pan', 'resnet18', L.F32, 'parity'), ('unet', 'timm-regnetx_002', L.F32, 'no encoder.layer4'),
    ('unet', 'efficientnet-b0', L.F32, 'no encoder.layer4'), ('unet', 'resnet18', L.F16, 'no backward')])
def test_unsupported_graphs_say_why(arch, enc, dt, word):
    import ctypes as C
    assert word in cam.unsupported_reason(arch, enc, dt)
    with pytest.raises(NotImplementedError, match=word):
        m = _fake_model(arch, enc, dt)
        cam.CAMProcessor(m, 'cuda', 'GradCAM', None)
    # the library refuses the same pairs with the same reason (host-only calls: no GPU needed)
    lib = L.lib()
    d = L.NetDesc(arch.encode(), enc.encode(), 1, 1, 64, 64, dt)
    p = C.c_void_p()
    if lib.octseg_plan_create(C.byref(d), C.byref(p)) != 0:
        return      # a pair the builder itself does not build
    try:
        assert lib.octseg_plan_set_frozen_bn(p, 1) == (-2 if dt == L.F16 else -3)
        assert word in lib.octseg_last_error().decode()
        assert lib.octseg_plan_cam_target(p, None, None, None) != 0
        assert lib.octseg_net_backward_seeded(p, p, p, p, None) == -5 and 'frozen' in lib.octseg_last_error().decode()
        assert lib.octseg_plan_set_frozen_bn(p, 0) == 0
    finally:
        lib.octseg_plan_destroy(p)


@pytest.mark.parametrize('arch,enc,K', [('unet', 'resnet18', 512), ('unetplusplus', 'resnet50', 2048), ('linknet', 'resnet34', 512),
                                        ('manet', 'resnet18', 512), ('unet', 'resnet152', 2048)])
def test_cam_target_of_supported_graphs(arch, enc, K):
    import ctypes as C
    lib = L.lib()
    assert cam.unsupported_reason(arch, enc, L.BF16) is None
    d = L.NetDesc(arch.encode(), enc.encode(), 2, 3, 64, 96, L.BF16)
    p = C.c_void_p()
    assert lib.octseg_plan_create(C.byref(d), C.byref(p)) == 0
    try:
        assert lib.octseg_plan_set_frozen_bn(p, 1) == 0
        act, gr, dims = C.c_size_t(), C.c_size_t(), (C.c_int * 4)()
        assert lib.octseg_plan_cam_target(p, C.byref(act), C.byref(gr), dims) == 0
        assert list(dims) == [3, 2, 3, K] and act.value != gr.value
        n = 3 * 2 * 3 * K * 2
        assert max(act.value, gr.value) + n <= lib.octseg_plan_workspace_bytes(p)
    finally:
        lib.octseg_plan_destroy(p)


def test_abi_argument_checks_need_no_gpu():
    lib = L.lib()
    one = 1     # any non-null pointer value: every refusal below happens before a launch
    assert lib.octseg_plan_set_frozen_bn(None, 1) == -5 and lib.octseg_plan_cam_target(None, None, None, None) == -5
    assert lib.octseg_net_backward_seeded(None, None, None, None, None) == -5
    base = dict(dtype=L.F32, A=one, G=one, N=1, h=2, w=2, K=64, method=0, S=32, scratch=one, maps=one)

    def call(**kw):
        a = dict(base, **kw)
        return lib.octseg_cam_maps(a['dtype'], a['A'], a['G'], a['N'], a['h'], a['w'], a['K'], a['method'], a['S'], a['scratch'], a['maps'], 0.5,
                                   a.get('bin'), a.get('gt'), a.get('gh', 0), a.get('gw', 0), a.get('rows'), a.get('cols'), a.get('counts'),
                                   a.get('frames'), a.get('jet'), a.get('iw', 0.5), a.get('overlay'), None)
    for k in ('A', 'G', 'scratch', 'maps'):
        assert call(**{k: None}) == -5
    assert call(dtype=L.F16) == -2 and call(dtype=9) == -2
    assert call(method=6) == -5 and call(method=-1) == -5
    for kw in ({'N': 0}, {'h': 0}, {'w': -1}, {'K': 0}, {'K': 60}, {'S': 0}, {'S': 1 << 20}):
        assert call(**kw) == -1, kw
    assert call(counts=one) == -5 and call(counts=one, gt=one, rows=one, cols=one, gh=0, gw=5) == -1
    assert call(overlay=one) == -5 and call(overlay=one, frames=one, jet=one, iw=1.5) == -5
    assert lib.octseg_cam_scratch_bytes(0, 1, 1, 8) == 0 and lib.octseg_cam_scratch_bytes(2, 3, 4, 64) == 4 * (2 * 64 + 2 * 12 + 8)
    assert lib.octseg_cam_overlay(None, one, one, 1, 8, 0.5, one, one, None) == -5
    assert lib.octseg_cam_overlay(one, one, one, 0, 8, 0.5, one, one, None) == -1


def test_config_parsing_with_overrides():
    from oct_segmentation_amd.config import load_config
    cfg = load_config('visualize_activation_maps')
    assert set(cfg) >= {'model_dir', 'data_dir', 'cam_method', 'output_size', 'device', 'aug_smooth', 'eigen_smooth', 'map_threshold', 'save_dir'}
    assert cfg['cam_method'] in cam.CAM_METHODS and cam.CAM_METHODS[cfg['cam_method']] is not None
    assert cfg['aug_smooth'] is False and cfg['eigen_smooth'] is False and 0.0 < float(cfg['map_threshold']) < 1.0
    cfg = load_config('visualize_activation_maps', ['cam_method=LayerCAM', 'map_threshold=0.25', 'output_size=[80,80]', 'save_dir=/tmp/x', 'batch_size=2'])
    assert cfg['cam_method'] == 'LayerCAM' and cfg['map_threshold'] == 0.25 and cfg['output_size'] == [80, 80] and cfg['batch_size'] == 2


def test_file_names_and_csv_rows_mirror_the_class_index_quirk(tmp_path):
    assert cam.CSV_COLUMNS == ['Image path', 'Image name', 'Class', 'Class ID', 'CAM', 'Model', 'Dice', 'IoU', 'Precision', 'Recall', 'F1']
    # the class INDEX picks the name (and the TIFF channel), whatever the model's class list is: index 1 is 'Fibrous cap', index 2 'Lipid core'
    assert [cam.class_name_of(i) for i in range(4)] == ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    assert cam.output_names('f 1', 'Fibrous cap', 'XGradCAM') == ['f_1_input.png', 'f_1_Fibrous_cap_XGradCAM.png', 'f_1_Fibrous_cap_XGradCAM_mask.png',
                                                                 'f_1_Fibrous_cap_pred.png', 'f_1_Fibrous_cap_gt.png']
    row = cam.metrics_row(str(tmp_path / 'img' / 'a.png'), 2, 'GradCAM', 'Unet', (3, 4, 6), root=str(tmp_path))
    assert list(row) == cam.CSV_COLUMNS
    assert row['Image path'] == os.path.join('img', 'a.png') and row['Image name'] == 'a.png' and row['Class'] == 'Lipid core' and row['Class ID'] == 2
    assert row['Dice'] == pytest.approx(0.6) and row['IoU'] == pytest.approx(3 / 7) and row['Precision'] == 0.75 and row['Recall'] == 0.5


def test_jet_table_closed_form():
    t = cam.jet_table_bgr()
    assert t.shape == (256, 3) and t.dtype == np.uint8 and np.array_equal(t, R.jet_bgr())
    assert list(t[0]) == [128, 0, 0] and list(t[255]) == [0, 0, 128]          # BGR: dark blue at 0, dark red at 1
    assert t[:, 1].argmax() in range(96, 160) and t[128, 1] == 255


def test_saved_image_resize_rule():
    few = np.zeros((8, 8, 3), np.uint8)
    few[2:5, 3:6] = (10, 200, 30)
    up = cam._resize_for_save(few, [16, 16])
    assert up.shape == (16, 16, 3) and len(np.unique(up.reshape(-1, 3), axis=0)) == 2          # nearest: no new colours
    from oct_segmentation_amd.predict import cv2_resize_linear_u8
    many = np.random.default_rng(0).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    assert np.array_equal(cam._resize_for_save(many, [12, 10]), cv2_resize_linear_u8(many, 12, 10))
    plane = np.zeros((6, 6), np.uint8)
    plane[1:3] = 255
    assert np.array_equal(cam._resize_for_save(plane, [6, 6]), plane) and cam._resize_for_save(plane, None) is plane
