"""The rendering kernel (csrc/render.hip through oct_segmentation_amd/postprocess.py and predict.py) against the host restatement of the
reference's save_results (tests/postprocess_ref.py: morphology and blur from OpenCV's definitions, pastes by PIL itself) and against the
reference's own published run.  The arithmetic is integer: every comparison is equality of both outputs."""
import itertools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import postprocess_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import postprocess

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PIN = os.path.join(HERE, 'golden', 'demo_overlay_crop.npz')
ALL = R.ALL_CLASSES


def _blobs(rng, h, w, p=0.4, smooth=2):
    if h * w < 36:
        return rng.random((h, w)) < p
    a = rng.random((h + 2 * smooth, w + 2 * smooth))
    s = sum(a[i:i + h, j:j + w] for i in range(2 * smooth + 1) for j in range(2 * smooth + 1))
    return s > np.quantile(s, 1 - p)


def _blob_masks(rng, n, h, w, p=0.4):
    return np.stack([np.stack([_blobs(rng, h, w, p, smooth=1 + (c & 1)) for c in range(4)], axis=-1) for _ in range(n)]).astype(np.float32)


def _noise(rng, n, h, w):
    return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _gpu(cuda, frames, masks, classes, it):
    ov, cm = postprocess.render_results(torch.from_numpy(frames).to(cuda), torch.from_numpy(np.ascontiguousarray(masks, np.float32)).to(cuda),
                                        classes, close_iterations=it)
    assert ov.dtype == cm.dtype == torch.uint8 and tuple(ov.shape) == tuple(cm.shape) == frames.shape
    return ov.cpu().numpy(), cm.cpu().numpy()


def _check(cuda, frames, masks, classes=ALL, its=(1, 2, 3), what=''):
    for it in its:
        got_ov, got_cm = _gpu(cuda, frames, masks, classes, it)
        want_ov, want_cm = R.render_batch(frames, masks, classes, it)
        bad = np.argwhere(np.any(got_ov != want_ov, axis=-1))
        assert np.array_equal(got_cm, want_cm), (what, it, 'colour mask')
        assert np.array_equal(got_ov, want_ov), (what, it, 'overlay', len(bad), bad[:5].tolist())


@pytest.mark.parametrize('h,w', [(1, 1), (3, 5), (7, 40), (31, 31), (64, 64), (65, 130), (200, 300)])
@pytest.mark.parametrize('n', [1, 3])
def test_random_blobs_every_size(cuda, n, h, w):
    rng = np.random.default_rng(1000 * h + w + n)
    _check(cuda, _noise(rng, n, h, w), _blob_masks(rng, n, h, w), what=(n, h, w))


def test_borders_corners_full_empty_single_pixels(cuda):
    rng = np.random.default_rng(5)
    h, w = 70, 101
    cases = {}
    for name, (ys, xs) in {'top': (slice(0, 9), slice(30, 60)), 'bottom': (slice(h - 6, h), slice(20, 50)), 'left': (slice(20, 40), slice(0, 7)),
                           'right': (slice(25, 50), slice(w - 5, w)), 'tl': (slice(0, 8), slice(0, 8)), 'tr': (slice(0, 5), slice(w - 9, w)),
                           'bl': (slice(h - 9, h), slice(0, 4)), 'br': (slice(h - 3, h), slice(w - 3, w))}.items():
        m = np.zeros((h, w, 4), np.float32)
        m[ys, xs, :2] = 1
        m[ys, xs, 2 + (len(name) & 1)] = 1
        cases[name] = m
    cases['ones'] = np.ones((h, w, 4), np.float32)
    cases['zeros'] = np.zeros((h, w, 4), np.float32)
    for name, (y, x) in {'px00': (0, 0), 'pxlast': (h - 1, w - 1), 'pxmid': (h // 2, w // 2), 'px_near': (1, w - 2)}.items():
        m = np.zeros((h, w, 4), np.float32)
        m[y, x, :] = 1
        cases[name] = m
    # the complement of a border-touching shape: erosion at the border must see "outside = set"
    m = np.ones((h, w, 4), np.float32)
    m[0:6, 40:52] = 0; m[30:34, 0:3] = 0; m[h - 2:h, w - 2:w] = 0
    cases['holes_at_border'] = m
    frames = _noise(rng, 1, h, w)
    for name, m in cases.items():
        _check(cuda, frames, m[None], what=name)


def test_holes_gaps_and_thin_lines(cuda):
    rng = np.random.default_rng(6)
    h, w = 96, 160
    m = np.zeros((h, w, 4), np.float32)
    m[8:88, 8:152, 0] = 1
    for k in range(1, 8):                                  # square holes and slits of width 1..7: closing fills some, leaves others
        m[12:12 + k, 12 + 18 * k:12 + 18 * k + k, 0] = 0
        m[30:70, 14 + 18 * k:14 + 18 * k + k, 0] = 0
        m[74 + (k & 1) * 4:74 + (k & 1) * 4 + k, 10 + 18 * k:24 + 18 * k, 0] = 0
    x = 4
    for k in range(1, 8):                                  # bars separated by gaps of width 1..7
        m[10:40, x:x + 6, 1] = 1
        m[50 + x // 8:52 + x // 8, 4:150, 1] = (k & 1)
        x += 6 + k
    m[5, :, 2] = 1; m[:, 77, 2] = 1; m[60, 10:150, 2] = 1  # one-pixel lines, a cross
    yy, xx = np.mgrid[0:h, 0:w]
    m[:, :, 2] = np.maximum(m[:, :, 2], (yy == xx // 2 + 10))          # a thin diagonal
    m[:, :, 3] = ((yy + xx) % 5 == 0) & (yy > 40)                       # a dotted texture
    _check(cuda, _noise(rng, 1, h, w), m[None], what='holes')


def test_class_subsets_and_order(cuda):
    rng = np.random.default_rng(7)
    h, w = 48, 76
    frames, masks = _noise(rng, 2, h, w), _blob_masks(rng, 2, h, w, p=0.5)      # p = 0.5: the classes overlap
    assert (masks.sum(axis=-1) >= 2).any() and (masks.sum(axis=-1) == 4).any()
    for k in range(1, 5):
        for sub in itertools.combinations(ALL, k):
            _check(cuda, frames, masks, list(sub), its=(1,), what=sub)
    for order in (ALL[::-1], [ALL[2], ALL[0], ALL[3], ALL[1]]):
        _check(cuda, frames, masks, order, its=(1, 3), what=order)
    a, _ = _gpu(cuda, frames, masks, ALL, 1)
    b, _ = _gpu(cuda, frames, masks, ALL[::-1], 1)
    assert not np.array_equal(a, b)                        # order matters where classes overlap
    _check(cuda, frames, masks, [ALL[0], ALL[0], ALL[1]], its=(2,), what='a class twice')


def test_other_layouts_unaligned_and_five_channel_stack(cuda):
    """Paths beside the vector one: a stack that is not 4 channels wide (scalar loads), tensors at odd byte offsets (byte loads / stores)."""
    rng = np.random.default_rng(8)
    n, h, w = 2, 40, 64
    frames, masks = _noise(rng, n, h, w), _blob_masks(rng, n, h, w)
    want = R.render_batch(frames, masks, ALL, 2)
    m5 = np.concatenate([masks, np.ones((n, h, w, 1), np.float32)], axis=-1)
    got = postprocess.render_results(torch.from_numpy(frames).to(cuda), torch.from_numpy(m5).to(cuda), ALL, 2)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    # frames / outputs one byte past a dword boundary, the stack 4 bytes past a 16-byte one: straight through the C entry
    fbuf = torch.zeros(frames.size + 8, dtype=torch.uint8, device=cuda)
    fbuf[1:1 + frames.size] = torch.from_numpy(frames).to(cuda).flatten()
    sbuf = torch.zeros(masks.size + 8, dtype=torch.float32, device=cuda)
    sbuf[1:1 + masks.size] = torch.from_numpy(masks).to(cuda).flatten()
    ov = torch.full((frames.size + 8,), 7, dtype=torch.uint8, device=cuda)
    cm = torch.full((frames.size + 8,), 7, dtype=torch.uint8, device=cuda)
    ch = torch.tensor([R.CLASS_IDS[c] - 1 for c in ALL], dtype=torch.int32, device=cuda)
    rgb = torch.tensor([R.CLASS_COLORS_RGB[c] for c in ALL], dtype=torch.uint8, device=cuda)
    tab = torch.from_numpy(postprocess.alpha_table()).to(cuda)
    rc = L.lib().octseg_render_results(L.C.c_void_p(sbuf.data_ptr() + 4), L.C.c_void_p(fbuf.data_ptr() + 1), n, h, w, 4, L.ptr(ch),
                                       L.ptr(rgb), 4, L.ptr(tab), postprocess.RING_ALPHA, 2, L.C.c_void_p(ov.data_ptr() + 3),
                                       L.C.c_void_p(cm.data_ptr() + 2), L.stream_ptr())
    assert rc == 0, L.lib().octseg_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(ov[3:3 + frames.size].cpu().numpy().reshape(frames.shape), want[0])
    assert np.array_equal(cm[2:2 + frames.size].cpu().numpy().reshape(frames.shape), want[1])
    assert (ov[:3] == 7).all() and (ov[3 + frames.size:] == 7).all() and (cm[:2] == 7).all() and (cm[2 + frames.size:] == 7).all()
    # channel ids outside the stack are clamped on the device (as in octseg_ingest_mask), not read out of bounds
    ch_bad = torch.tensor([-3, 1, 2, 99], dtype=torch.int32, device=cuda)
    o2, c2 = torch.empty_like(fbuf[:frames.size]), torch.empty_like(fbuf[:frames.size])
    f0, s0 = torch.from_numpy(frames).to(cuda), torch.from_numpy(masks).to(cuda)
    assert L.lib().octseg_render_results(L.ptr(s0), L.ptr(f0), n, h, w, 4, L.ptr(ch_bad), L.ptr(rgb), 4, L.ptr(tab), postprocess.RING_ALPHA, 2,
                                         L.ptr(o2), L.ptr(c2), L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(o2.cpu().numpy().reshape(frames.shape), want[0])


def test_full_size_frames_with_elliptic_masks(cuda):
    rng = np.random.default_rng(9)
    n, s = 2, 1000
    yy, xx = np.mgrid[0:s, 0:s]
    masks = np.zeros((n, s, s, 4), np.float32)
    for i in range(n):
        for c, (cy, cx, ry, rx) in enumerate([(500, 480 + 30 * i, 300, 340), (420, 600, 120, 200), (560, 380, 90, 60), (30, 990, 45, 25)]):
            masks[i, :, :, c] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    _check(cuda, _noise(rng, n, s, s), masks, its=(1, 3), what='1000^2')


def test_kernel_equals_the_reference_run(cuda):
    """The reference pin through the kernel: the authors' frame and colour mask in, the authors' overlay out, on the compared set."""
    frame, masks, overlay, compared = R.load_pin(PIN)
    R.check_pin_coverage(frame, overlay, compared)
    for it in (1, 3):
        got_ov, got_cm = _gpu(cuda, frame[None], masks[None], ALL, it)
        assert np.array_equal(got_ov[0][compared], overlay[compared]), it
        assert np.array_equal(got_cm[0][compared], np.load(PIN)['mask'][compared]), it


def test_save_results_end_to_end(cuda, tmp_path):
    rng = np.random.default_rng(10)
    n, h, w = 3, 50, 68
    frames, masks = _noise(rng, n, h, w), _blob_masks(rng, n, h, w)
    images = [Image.fromarray(f) for f in frames]
    names = [f'frame{i}' for i in range(n)]
    classes = ['Lumen', 'Lipid core', 'Vasa vasorum']
    a, b = os.path.join(tmp_path, 'from_numpy'), os.path.join(tmp_path, 'from_stack')
    postprocess.save_results(images, [m.astype(np.float64) for m in masks], names, classes, a)
    postprocess.save_results(images, torch.from_numpy(masks).to(cuda), names, classes, b)
    want_ov, want_cm = R.render_batch(frames, masks, classes, 1)
    for d in (a, b):
        assert sorted(os.listdir(d)) == sorted([f'{x}_mask.png' for x in names] + [f'{x}_overlay.png' for x in names])
        for i, name in enumerate(names):
            ov, cm = Image.open(os.path.join(d, f'{name}_overlay.png')), Image.open(os.path.join(d, f'{name}_mask.png'))
            assert ov.mode == cm.mode == 'RGB'
            assert np.array_equal(np.asarray(ov), want_ov[i]) and np.array_equal(np.asarray(cm), want_cm[i])
    c = os.path.join(tmp_path, 'three_iterations')
    postprocess.save_results(images[:1], masks[:1], names[:1], classes, c, close_iterations=3)
    assert np.array_equal(np.asarray(Image.open(os.path.join(c, 'frame0_overlay.png'))), R.render_batch(frames[:1], masks[:1], classes, 3)[0][0])
    # grey frames are rendered as RGB
    d = os.path.join(tmp_path, 'grey')
    grey = Image.fromarray(frames[0, :, :, 0])
    postprocess.save_results([grey], masks[:1], ['g'], classes, d)
    assert np.array_equal(np.asarray(Image.open(os.path.join(d, 'g_overlay.png'))), R.render(grey.convert('RGB'), masks[0], classes, 1)[0])
    bad = masks.copy()
    bad[1, 3, 3, 0] = 0.5
    with pytest.raises(ValueError):
        postprocess.save_results(images, list(bad), names, classes, a)
    with pytest.raises(ValueError):
        postprocess.save_results(images, torch.from_numpy(bad).to(cuda), names, classes, a)
    with pytest.raises(ValueError):
        postprocess.save_results(images[:2], list(masks), names, classes, a)
    with pytest.raises(ValueError):
        postprocess.save_results([im.resize((w + 1, h)) for im in images], list(masks), names, classes, a)


def _models_dir(cuda, root):
    from oct_segmentation_amd.model import OCTSegmentationModel
    specs = {'LM': ('unet', ['Lumen'], 64), 'FC_LC': ('linknet', ['Lipid core', 'Fibrous cap'], 96), 'VV': ('unet', ['Vasa vasorum'], 64)}
    for d, (arch, classes, size) in specs.items():
        os.makedirs(os.path.join(root, d))
        m = OCTSegmentationModel(arch, 'resnet18', f'{arch}_resnet18', 3, classes, device=cuda, seed=len(d) + 3, compute_dtype=torch.float32)
        m.save_checkpoint(os.path.join(root, d, 'weights.ckpt'))
        with open(os.path.join(root, d, 'config.json'), 'w') as f:
            json.dump({'model_name': f'{arch}_resnet18', 'architecture': arch, 'encoder': 'resnet18', 'input_size': size, 'classes': classes}, f)
    return root


def test_segment_stack_is_what_segment_returns(cuda, tmp_path):
    from oct_segmentation_amd.predict import segment, segment_stack
    models = _models_dir(cuda, os.path.join(tmp_path, 'models'))
    rng = np.random.default_rng(11)
    images = [Image.fromarray(rng.integers(0, 255, (80, 80, 3), dtype=np.uint8)) for _ in range(3)]
    for classes in (ALL, ['Lipid core', 'Lumen']):
        for dp in (False, True):
            stack = segment_stack(images, [100, 100], classes, models, device='cuda', compute_dtype=torch.float32, batch_size=2, device_preprocess=dp)
            assert stack.is_cuda and stack.dtype == torch.float32 and tuple(stack.shape) == (3, 100, 100, 4)
            host = segment(images, [np.zeros((100, 100, 4)) for _ in images], [100, 100], classes, models, device='cuda',
                           compute_dtype=torch.float32, batch_size=2, device_preprocess=dp)
            s = stack.cpu().numpy()
            for i in range(3):
                for c in range(4):
                    assert np.array_equal(host[i][:, :, c], s[i, :, :, c]), (classes, dp, i, c)
            assert s.any() and not s.all()


def test_predict_main_writes_the_four_files(cuda, tmp_path):
    from oct_segmentation_amd import predict
    models = _models_dir(cuda, os.path.join(tmp_path, 'models'))
    rng = np.random.default_rng(12)
    data, save = os.path.join(tmp_path, 'input'), os.path.join(tmp_path, 'output')
    os.makedirs(data)
    for name in ('a', 'b'):
        Image.fromarray(rng.integers(0, 255, (90, 90, 3), dtype=np.uint8)).save(os.path.join(data, f'{name}.png'))
    with open(os.path.join(data, 'notes.txt'), 'w') as f:       # not matched by the reference's glob
        f.write('x')
    args = [f'data_dir={data}', f'models_dir={models}', f'save_dir={save}', 'output_size=[120,120]', 'compute_dtype=fp32']
    assert predict.main(args) == 0
    assert sorted(os.listdir(save)) == ['a_mask.png', 'a_overlay.png', 'b_mask.png', 'b_overlay.png']
    # the files are what the restatement makes of segment()'s masks
    images, masks = predict.data_processing([os.path.join(data, 'a.png')], [120, 120])
    masks = predict.segment(images, masks, [120, 120], ALL, models, device='cuda', compute_dtype=torch.float32, device_preprocess=True)
    want_ov, want_cm = R.render(images[0], masks[0], ALL, 1)
    assert np.array_equal(np.asarray(Image.open(os.path.join(save, 'a_overlay.png'))), want_ov)
    assert np.array_equal(np.asarray(Image.open(os.path.join(save, 'a_mask.png'))), want_cm)
    # a single file as data_dir
    save2 = os.path.join(tmp_path, 'output2')
    assert predict.main([f'data_dir={os.path.join(data, "b.png")}', f'models_dir={models}', f'save_dir={save2}', 'output_size=[64,64]',
                         'compute_dtype=fp32', 'classes=[Lumen]']) == 0
    assert sorted(os.listdir(save2)) == ['b_mask.png', 'b_overlay.png']


def test_abi_refuses_bad_arguments(cuda):
    lib = L.lib()
    f = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=cuda)
    s = torch.zeros((1, 8, 8, 4), dtype=torch.float32, device=cuda)
    ov = torch.full((1, 8, 8, 3), 9, dtype=torch.uint8, device=cuda)
    cm = torch.full((1, 8, 8, 3), 9, dtype=torch.uint8, device=cuda)
    ch = torch.zeros((16,), dtype=torch.int32, device=cuda)
    rgb = torch.zeros((16, 3), dtype=torch.uint8, device=cuda)
    tab = torch.zeros((257,), dtype=torch.uint8, device=cuda)
    st, p = L.stream_ptr(), L.ptr
    BAD_SHAPE, BAD_ARG = -1, -5

    def call(stack=s, frames=f, N=1, H=8, W=8, SC=4, chs=ch, col=rgb, C=4, table=tab, it=1, o=ov, m=cm):
        return lib.octseg_render_results(p(stack), p(frames), N, H, W, SC, p(chs), p(col), C, p(table), 231, it, p(o), p(m), st)

    for kw in ({'stack': None}, {'frames': None}, {'chs': None}, {'col': None}, {'table': None}, {'o': None}, {'m': None}):
        assert call(**kw) == BAD_ARG, kw
        assert b'null' in lib.octseg_last_error()
    for kw in ({'N': 0}, {'H': 0}, {'W': -1}, {'SC': 0}, {'C': 0}, {'C': 17}, {'it': 0}, {'it': 4}, {'it': -1}):
        assert call(**kw) == BAD_SHAPE, kw
    torch.cuda.synchronize()
    assert (ov == 9).all() and (cm == 9).all()                 # nothing was launched
    assert call(C=16) == 0 and call(it=3) == 0
    torch.cuda.synchronize()
    # the Python wrapper refuses what the kernel cannot take
    with pytest.raises(ValueError):
        postprocess.render_results(f, s, ALL, close_iterations=4)
    with pytest.raises(ValueError):
        postprocess.render_results(f, s[:, :4], ALL)
    with pytest.raises(ValueError):
        postprocess.render_results(f, s.double(), ALL)
    with pytest.raises(ValueError):
        postprocess.render_results(f.float(), s, ALL)
    with pytest.raises(ValueError):
        postprocess.render_results(f, s, [])
    with pytest.raises(ValueError):
        postprocess.render_results(f, s, ['Thrombus'])
    with pytest.raises(ValueError):
        postprocess.render_results(f, s[..., :2], ALL)             # Vasa vasorum needs channel 3
