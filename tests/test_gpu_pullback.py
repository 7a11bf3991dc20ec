"""The raw-volume kernels (csrc/volume.hip through oct_segmentation_amd/pullback.py, predict.py and postprocess.py): the normalisation against
its numpy restatement (tests/volume_ref.py), the resize against Pillow itself, and the chained calls against the staged host composition.
Everything is integer or exactly specified float32 arithmetic: every comparison is equality."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import volume_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import analysis, postprocess, predict, pullback
from oct_segmentation_amd.model import CLASS_IDS

pytestmark = pytest.mark.gpu

CLASSES = list(CLASS_IDS)
SHAPES = [((13, 9), (7, 21)), ((40, 64), (40, 37)), ((33, 17), (100, 5)), ((5, 5), (5, 5)), ((1, 3), (4, 2)), ((64, 48), (1, 1))]


def _same_bytes(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[got != want][:5].tolist(), want[got != want][:5].tolist())


def _check_normalize(vol, what, swaps=(True, False), tensor=False):
    for swap in swaps:
        src = torch.from_numpy(vol).cuda() if tensor else vol
        out, mm = pullback.normalize_volume(src, swap_rb=swap, return_minmax=True)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == tuple(vol.shape[:3]) + (3,)
        _same_bytes(mm, R.slice_minmax(vol), (what, 'minmax'))
        _same_bytes(out, R.normalize_ref(vol, swap_rb=swap), (what, swap))


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('h,w', [(1, 1), (2, 3), (17, 33), (64, 48), (97, 130)])
@pytest.mark.parametrize('s', [1, 3])
def test_normalize_equals_restatement(cuda, s, h, w, dtype):
    """Random slices, each with a range of its own; three and one channels, both channel orders.  (97, 130) x 3 x uint16 is more than one
    64 KiB workgroup range per slice; odd frame sizes put slice seams inside a lane's group of eight pixels and off the 16-byte grid."""
    rng = np.random.default_rng(1000 * h + 10 * w + s + (7 if dtype == np.uint16 else 0))
    top = np.iinfo(dtype).max
    for c in (3, 1):
        vol = np.empty((s, h, w, c), dtype)
        for k in range(s):
            lo = int(rng.integers(0, top // 2))
            vol[k] = rng.integers(lo, int(rng.integers(lo + 1, top + 1)) + 1, (h, w, c))
        _check_normalize(vol if c == 3 else vol[..., 0], (s, h, w, c, dtype.__name__))


def _designed(dtype, h, w):
    """Eight slices, each with its own range and its extremes in designed places; every other sample lies strictly inside the range."""
    top = np.iinfo(dtype).max
    big = dtype == np.uint16
    ranges = [(300, 50000) if big else (3, 250), (1000, 1255) if big else (40, 60), (17, 40000) if big else (17, 200), None,
              (40000, 65535) if big else (200, 255), (0, 255), (10, 11), (5, top - 5)]
    rng = np.random.default_rng(h * w + top)
    vol = np.empty((8, h, w, 3), dtype)
    for k, r in enumerate(ranges):
        if r is None:
            vol[k] = 1234 if big else 77                       # a constant slice between two ordinary ones
            continue
        lo, hi = r
        vol[k] = rng.integers(lo + 1, hi, (h, w, 3)) if hi - lo > 1 else lo
    flat = vol.reshape(8, -1)
    n = flat.shape[1]
    flat[0, 0], flat[0, n - 1] = ranges[0]                      # the minimum only in the first element, the maximum only in the LAST
    vol[1, h // 2, w // 3, 2], vol[1, h // 3, w // 2, 2] = ranges[1]      # both only in channel 2
    flat[2, n // 2], flat[2, n - 2] = ranges[2]                 # the maximum behind the last 16-byte vector (frames are no multiple of 16 bytes)
    flat[4, 7], flat[4, n // 3] = ranges[4]                     # uint16: everything above 32767, the maximum 65535
    flat[5, 11], flat[5, n - 5] = ranges[5]                     # spans 0..255 already: a = 1, b = 0
    flat[6, n // 2] = 11                                        # a range of one grey level
    flat[7, n // 4], flat[7, 3 * n // 4] = ranges[7]
    return vol, ranges


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
def test_normalize_designed_slices(cuda, dtype):
    h, w = 17, 33
    vol, ranges = _designed(dtype, h, w)
    assert (vol[0].size * vol.itemsize) % 16 != 0
    want_mm = [list(r) if r else [int(vol[3, 0, 0, 0])] * 2 for r in ranges]
    assert R.slice_minmax(vol).tolist() == want_mm
    _check_normalize(vol, ('designed', dtype.__name__))
    out = pullback.normalize_volume(vol, swap_rb=False).cpu().numpy()
    assert not out[3].any()                                                      # constant -> 0
    for k in (0, 1, 2, 4, 5, 6, 7):
        assert out[k].min() == 0 and out[k].max() == 255, k
    assert np.array_equal(out[5], vol[5].astype(np.uint8))                       # 0..255 comes out unchanged
    assert sorted(np.unique(out[6]).tolist()) == [0, 255]
    # a CUDA tensor of the same dtype is taken as it is
    _check_normalize(vol, ('designed tensor', dtype.__name__), swaps=(True,), tensor=True)


def test_normalize_tile_seams_and_unaligned_views(cuda):
    """uint16 (97, 130, 3): 75660 bytes a slice, two workgroup ranges; extremes on both sides of the 64 KiB seam, in the first element of
    a slice that starts off the 16-byte grid and in the last.  Then uint8 volumes that start one byte into their storage (the scalar path)."""
    rng = np.random.default_rng(42)
    vol = rng.integers(1000, 2000, (3, 97, 130, 3)).astype(np.uint16)
    flat = vol.reshape(3, -1)
    flat[0, 32767], flat[0, 32768] = 3, 60001                   # the last sample of range 0, the first of range 1
    flat[1, 0], flat[1, -1] = 999, 2000
    flat[2, 32760], flat[2, 32775] = 2500, 12
    _check_normalize(vol, 'seams', swaps=(True,))
    for c in (3, 1):
        v8 = rng.integers(20, 230, (3, 17, 33, c)).astype(np.uint8)
        v8[1, 0, 0, 0], v8[1, -1, -1, -1] = 1, 255
        buf = torch.zeros(v8.size + 32, dtype=torch.uint8, device=cuda)
        buf[1:1 + v8.size] = torch.from_numpy(v8).to(cuda).flatten()
        view = buf[1:1 + v8.size].view(v8.shape if c == 3 else v8.shape[:3])
        assert view.data_ptr() % 16 == 1
        out, mm = pullback.normalize_volume(view, return_minmax=True)
        _same_bytes(mm, R.slice_minmax(v8), ('view', c))
        _same_bytes(out, R.normalize_ref(v8 if c == 3 else v8[..., 0]), ('view', c))
    for bad in (vol.astype(np.int16), vol.astype(np.float32), vol[0, 0], vol[:0], np.zeros((1, 4, 4, 2), np.uint8)):
        with pytest.raises(ValueError):
            pullback.normalize_volume(bad)


def _frames(rng, n, h, w, c):
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for k in range(n):
        if k == 1:
            a = np.repeat(((((yy // 2) + (xx // 2)) & 1) * 255).astype(np.uint8)[:, :, None], c, axis=2)     # overshoot on both sides of the clamp
        else:
            a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        out.append(a)
    return np.stack(out)


def _pil_resize(batch, oh, ow):
    return np.stack([np.array(Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a).resize((ow, oh))).reshape(oh, ow, a.shape[2]) for a in batch])


@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('src,dst', SHAPES)
def test_resize_equals_pillow(cuda, src, dst, n, c):
    (h, w), (oh, ow) = src, dst
    batch = _frames(np.random.default_rng(100 * h + w + n), n, h, w, c)
    got = pullback.resize_pil_u8(torch.from_numpy(batch).to(cuda), (oh, ow))
    assert got.is_cuda and got.dtype == torch.uint8
    _same_bytes(got, _pil_resize(batch, oh, ow), (src, dst, n, c))


def test_resize_equals_pillow_at_the_demo_size(cuda):
    rng = np.random.default_rng(5)
    batch = rng.integers(0, 256, (1, 750, 750, 3), dtype=np.uint8)
    batch[0, 100:300, 100:300] = _frames(rng, 2, 200, 200, 3)[1]
    _same_bytes(pullback.resize_pil_u8(torch.from_numpy(batch).to(cuda), 1000), _pil_resize(batch, 1000, 1000), 'demo')
    for bad in (torch.zeros((1, 4, 4, 2), dtype=torch.uint8, device=cuda), torch.zeros((1, 4, 4, 3), device=cuda),
                torch.zeros((1, 4, 4, 3), dtype=torch.uint8), torch.zeros((0, 4, 4, 3), dtype=torch.uint8, device=cuda)):
        with pytest.raises(ValueError):
            pullback.resize_pil_u8(bad, 8)


@pytest.fixture(scope='module')
def models(cuda, tmp_path_factory):
    """Tiny resnet18 model dirs, as tests/test_gpu_analysis.py builds them."""
    from oct_segmentation_amd.model import OCTSegmentationModel
    root = str(tmp_path_factory.mktemp('models'))
    specs = {'LM': ('unet', ['Lumen'], 64), 'FC_LC': ('linknet', ['Lipid core', 'Fibrous cap'], 96), 'VV': ('unet', ['Vasa vasorum'], 64)}
    for d, (arch, classes, size) in specs.items():
        os.makedirs(os.path.join(root, d))
        m = OCTSegmentationModel(arch, 'resnet18', f'{arch}_resnet18', 3, classes, device=cuda, seed=len(d) + 3, compute_dtype=torch.float32)
        m.save_checkpoint(os.path.join(root, d, 'weights.ckpt'))
        with open(os.path.join(root, d, 'config.json'), 'w') as f:
            json.dump({'model_name': f'{arch}_resnet18', 'architecture': arch, 'encoder': 'resnet18', 'input_size': size, 'classes': classes}, f)
    return root


def _volume():
    rng = np.random.default_rng(21)
    vol = rng.integers(500, 4000, (3, 90, 90, 3)).astype(np.uint16)
    yy, xx = np.mgrid[0:90, 0:90]
    for k in range(3):                                          # some structure, and a range of its own per slice
        vol[k][(yy - 45) ** 2 + (xx - 40 - 3 * k) ** 2 < (15 + 5 * k) ** 2] += 20000 + 9000 * k
    return vol


def _staged(vol, models, names):
    """normalize_ref -> Image.resize -> segment_stack(PIL list) -> analyze_stack(ratio of the SOURCE height)."""
    images = [Image.fromarray(f).resize((120, 120)) for f in R.normalize_ref(vol)]
    stack = predict.segment_stack(images, [120, 120], CLASSES, models, device='cuda', compute_dtype=torch.float32, device_preprocess=True)
    return images, stack, analysis.analyze_stack(stack, names, ratio=13)


def test_analyze_pullback_equals_the_staged_composition(cuda, models):
    vol = _volume()
    images, stack, want = _staged(vol, models, ['001', '002', '003'])
    res = pullback.analyze_pullback(vol, models, CLASSES, output_size=(120, 120), render=True, compute_dtype=torch.float32)
    assert res.data['ratio'] == 13 == int(vol.shape[1] * 150 // 1000) and res.data['images'] == ['001', '002', '003']
    frames = np.stack([np.asarray(im) for im in images])
    _same_bytes(res.frames, frames, 'frames')
    assert torch.equal(res.stack, stack)
    assert json.loads(json.dumps(res.data)) == json.loads(json.dumps(want))
    assert any(len(o['slice']) for o in res.data['objects'].values())           # the nets found something to measure
    overlay, color_mask = postprocess.render_results(torch.from_numpy(frames).to(cuda), stack, CLASSES)
    assert torch.equal(res.overlay, overlay) and torch.equal(res.color_mask, color_mask)
    plain = pullback.analyze_pullback(vol, models, CLASSES, output_size=(120, 120), names=['a', 'b', 'c'], compute_dtype=torch.float32)
    assert plain.overlay is None and plain.color_mask is None and plain.data['images'] == ['a', 'b', 'c']
    assert torch.equal(plain.stack, stack)


def _files(d):
    out = {}
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), 'rb') as f:
            out[name] = f.read()
    return out


def test_predict_main_device_resize_is_byte_identical(cuda, models, tmp_path):
    rng = np.random.default_rng(31)
    data_dir = os.path.join(tmp_path, 'input')
    os.makedirs(data_dir)
    for name in ('b_rgb', 'a_rgb', 'c_rgb'):
        Image.fromarray(rng.integers(0, 256, (90, 90, 3), dtype=np.uint8)).save(os.path.join(data_dir, f'{name}.png'))
    Image.fromarray(rng.integers(0, 256, (90, 90), dtype=np.uint8)).save(os.path.join(data_dir, 'd_grey.png'))           # mode L: device path
    Image.fromarray(rng.integers(0, 256, (90, 90, 3), dtype=np.uint8)).quantize(16).save(os.path.join(data_dir, 'e_pal.png'))   # mode P: host
    assert Image.open(os.path.join(data_dir, 'd_grey.png')).mode == 'L' and Image.open(os.path.join(data_dir, 'e_pal.png')).mode == 'P'
    args = [f'data_dir={data_dir}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32', 'analysis=true']
    host, dev = os.path.join(tmp_path, 'host'), os.path.join(tmp_path, 'dev')
    assert predict.main(args + [f'save_dir={host}', 'device_resize=false']) == 0
    assert predict.main(args + [f'save_dir={dev}']) == 0
    a, b = _files(host), _files(dev)
    assert sorted(a) == sorted(['analysis.json'] + [f'{n}_{k}.png' for n in ('a_rgb', 'b_rgb', 'c_rgb', 'd_grey', 'e_pal') for k in ('mask', 'overlay')])
    assert sorted(a) == sorted(b)
    for name in a:
        assert a[name] == b[name], name
    # the frames the device path hands on are the host's, mode by mode
    frames = predict._frames_on_device([os.path.join(data_dir, f'{n}.png') for n in ('d_grey', 'e_pal', 'a_rgb')], [120, 120], cuda)
    want = np.stack([np.asarray(Image.open(os.path.join(data_dir, f'{n}.png')).resize((120, 120)).convert('RGB')) for n in ('d_grey', 'e_pal', 'a_rgb')])
    _same_bytes(frames, want, 'frames_on_device')


def test_predict_main_takes_a_raw_volume(cuda, models, tmp_path):
    vol = _volume()
    np.save(os.path.join(tmp_path, 'vol.npy'), vol)
    png_dir = os.path.join(tmp_path, 'png')
    os.makedirs(png_dir)
    names = [f'vol_{k + 1:03d}' for k in range(3)]
    for name, f in zip(names, R.normalize_ref(vol)):
        Image.fromarray(f).save(os.path.join(png_dir, f'{name}.png'))
    args = [f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32', 'analysis=true']
    out_v, out_p = os.path.join(tmp_path, 'out_v'), os.path.join(tmp_path, 'out_p')
    assert predict.main(args + [f'data_dir={os.path.join(tmp_path, "vol.npy")}', f'save_dir={out_v}']) == 0
    assert predict.main(args + [f'data_dir={png_dir}', f'save_dir={out_p}', 'device_resize=false']) == 0
    a, b = _files(out_v), _files(out_p)
    assert sorted(a) == sorted(['analysis.json'] + [f'{n}_{k}.png' for n in names for k in ('mask', 'overlay')]) == sorted(b)
    for name in a:
        if name.endswith('.png'):
            assert a[name] == b[name], name
    got, png = json.loads(a['analysis.json']), json.loads(b['analysis.json'])
    assert got['ratio'] == 13 and png['ratio'] == 18 and got['images'] == png['images'] == names
    for cl in CLASSES:
        for k in ('slice', 'object_id', 'img_name'):            # what does not depend on the ratio
            assert got['objects'][cl][k] == png['objects'][cl][k], (cl, k)
    # the PNG run's analysis, rebuilt with the volume's ratio
    _, _, want = _staged(vol, models, names)
    assert got == json.loads(json.dumps(want))
    # without the key no analysis is written
    out_n = os.path.join(tmp_path, 'out_n')
    assert predict.main([f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32', f'data_dir={os.path.join(tmp_path, "vol.npy")}',
                         f'save_dir={out_n}', 'classes=[Lumen]']) == 0
    assert sorted(os.listdir(out_n)) == sorted(f'{n}_{k}.png' for n in names for k in ('mask', 'overlay'))


def _clamped_pass(a, axis, out_len, bounds, kk):
    """One resample pass with the device's clamping of the table: first into [0, in - 1], count into [0, min(ksize, in - first)]."""
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    out = np.empty((out_len,) + a.shape[1:], np.int64)
    for i in range(out_len):
        first = min(max(int(bounds[i, 0]), 0), a.shape[0] - 1)
        n = min(max(int(bounds[i, 1]), 0), min(kk.shape[1], a.shape[0] - first))
        out[i] = np.clip(((1 << 21) + np.tensordot(kk[i, :n].astype(np.int64), a[first:first + n], axes=(0, 0))) >> 22, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def test_abi_refuses_bad_arguments(cuda):
    lib = L.lib()
    st, p = L.stream_ptr(), L.ptr
    BAD_SHAPE, BAD_DTYPE, BAD_ARG = -1, -2, -5
    S, H, W, C = 2, 6, 5, 3
    src = (torch.arange(S * H * W * C * 2, device=cuda) % 256).to(torch.uint8)
    mm = torch.full((S + 1, 2), 9, dtype=torch.int32, device=cuda)
    dst = torch.full((S * H * W * 3 + 8,), 9, dtype=torch.uint8, device=cuda)

    def norm(src_=src, dt=0, S_=S, H_=H, W_=W, C_=C, mm_=mm, dst_=dst, off=0):
        sp = None if src_ is None else L.C.c_void_p(src_.data_ptr() + off)
        return lib.octseg_volume_normalize(sp, dt, S_, H_, W_, C_, 1, p(mm_), p(dst_), st)

    for kw in ({'src_': None}, {'mm_': None}, {'dst_': None}, {'dt': 1, 'off': 1}):
        assert norm(**kw) == BAD_ARG, kw
    assert b'null' in lib.octseg_last_error() or b'aligned' in lib.octseg_last_error()
    for kw in ({'dt': 2}, {'dt': -1}):
        assert norm(**kw) == BAD_DTYPE, kw
    for kw in ({'S_': 0}, {'H_': 0}, {'W_': -1}, {'C_': 2}, {'C_': 4}, {'C_': 0}, {'H_': 32768, 'W_': 32768, 'C_': 1},
               {'H_': 32768, 'W_': 16384, 'C_': 3, 'dt': 1}):                # 3 GiB of uint16 a frame; its uint8 form would fit
        assert norm(**kw) == BAD_SHAPE, kw
    torch.cuda.synchronize()
    assert (mm == 9).all() and (dst == 9).all()                 # nothing was launched
    assert norm() == 0
    torch.cuda.synchronize()
    assert (mm[S] == 9).all() and (dst[S * H * W * 3:] == 9).all() and mm[:S].tolist() == [[0, 89], [90, 179]]

    oh, ow = 9, 8
    frames = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (S, H, W, C), dtype=np.uint8)).to(cuda)
    xb_np, xk_np = pullback.pil_resample_table(W, ow)
    yb_np, yk_np = pullback.pil_resample_table(H, oh)
    xb, xk, yb, yk = (torch.from_numpy(t).to(cuda) for t in (xb_np, xk_np, yb_np, yk_np))
    tmp = torch.full((S * H * ow * C + 8,), 9, dtype=torch.uint8, device=cuda)
    out = torch.full((S * oh * ow * C + 8,), 9, dtype=torch.uint8, device=cuda)

    def resize(src_=frames, S_=S, H_=H, W_=W, C_=C, tmp_=tmp, dst_=out, oh_=oh, ow_=ow, xb_=xb, xk_=xk, xks=xk_np.shape[1], yb_=yb, yk_=yk,
               yks=yk_np.shape[1]):
        return lib.octseg_resize_pil_u8(p(src_), S_, H_, W_, C_, p(tmp_), p(dst_), oh_, ow_, p(xb_), p(xk_), xks, p(yb_), p(yk_), yks, st)

    for kw in ({'src_': None}, {'dst_': None}, {'tmp_': None}, {'xb_': None}, {'xk_': None}, {'yb_': None}, {'yk_': None}):
        assert resize(**kw) == BAD_ARG, kw
    for kw in ({'S_': 0}, {'H_': 0}, {'W_': -1}, {'oh_': 0}, {'ow_': -2}, {'C_': 2}, {'C_': 4}, {'xks': 0}, {'yks': -1},
               {'H_': 65536, 'W_': 32768, 'C_': 1}, {'oh_': 65536, 'ow_': 32768, 'C_': 1}, {'H_': 32768, 'ow_': 32768}):
        assert resize(**kw) == BAD_SHAPE, kw
    torch.cuda.synchronize()
    assert (tmp == 9).all() and (out == 9).all()                # nothing was launched
    # a skipped axis needs neither its tables nor the intermediate
    assert resize(oh_=H, tmp_=None, yb_=None, yk_=None, yks=0) == 0
    torch.cuda.synchronize()
    _same_bytes(out[:S * H * ow * C].view(S, H, ow, C), _pil_resize(frames.cpu().numpy(), H, ow), 'x only')
    assert (out[S * H * ow * C:] == 9).all() and (tmp == 9).all()
    assert resize(ow_=W, tmp_=None, xb_=None, xk_=None, xks=0) == 0
    torch.cuda.synchronize()
    _same_bytes(out[:S * oh * W * C].view(S, oh, W, C), _pil_resize(frames.cpu().numpy(), oh, W), 'y only')
    # bounds outside the source and counts beyond ksize or the source's end are clamped on the device, not followed
    wx, wy = xb_np.copy(), yb_np.copy()
    wx[0] = (-5, 3); wx[1] = (2 ** 31 - 1, 2); wx[2] = (W - 1, 10 ** 6); wx[3] = (1, -4)
    wy[0] = (-(2 ** 31), 2 ** 31 - 1); wy[1] = (10 ** 6, 1); wy[2] = (H - 2, 5)
    out.fill_(9)
    assert resize(xb_=torch.from_numpy(wx).to(cuda), yb_=torch.from_numpy(wy).to(cuda)) == 0
    torch.cuda.synchronize()
    f = frames.cpu().numpy()
    want = np.stack([_clamped_pass(_clamped_pass(a, 1, ow, wx, xk_np), 0, oh, wy, yk_np) for a in f])
    _same_bytes(out[:S * oh * ow * C].view(S, oh, ow, C), want, 'wild tables')
    assert (out[S * oh * ow * C:] == 9).all()
