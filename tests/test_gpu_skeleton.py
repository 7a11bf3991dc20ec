"""Thinning, census and local thickness on the GPU against the numpy restatement (tests/skeleton_ref.py): EQUALITY, no tolerance -- the skeleton is
unique and everything is boolean or integer.  Both paths (LDS and forced global) on every case, the two agreeing with each other too."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import distance_ref
import skeleton_cases as K
import skeleton_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import skeleton
from oct_segmentation_amd.model import CLASS_IDS

pytestmark = pytest.mark.gpu


def up(stack, cuda):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(stack) != 0).astype(np.float32)).to(cuda)


def both_paths(stack, cuda, want=None):
    """The stack through both paths; each must equal the reference in skeleton and census (and so each other).  Returns the reference."""
    want = K.reference(stack) if want is None else want
    dev = stack if torch.is_tensor(stack) else up(stack, cuda)
    for path in ('auto', 'global'):
        out, cen = skeleton.skeleton_stack(dev, with_census=True, path=path)
        assert out.dtype == torch.float32 and out.shape == dev.shape and cen.dtype == torch.int32
        got, gcen = out.cpu().numpy(), cen.cpu().numpy()
        assert np.array_equal(gcen, want[1]), (path, gcen.tolist(), want[1].tolist())
        assert np.array_equal(got, want[0]), (path, int((got != want[0]).sum()))
    return want


# ---- 1. random planes around the 64-pixel word
@pytest.mark.parametrize('h,w', K.SHAPES)
def test_random_planes_equal_restatement(cuda, h, w):
    planes = [K.drawn(h, w, d, seed) for d in K.DENSITIES for seed in (0, 1)] + [K.blobs(h, w, 0), K.blobs(h, w, 1)]
    for n, c in ((1, 1), (3, 4), (1, 5)):
        st = np.stack([np.stack([planes[(i * c + k) % len(planes)] for k in range(c)], axis=-1) for i in range(n)])
        both_paths(st, cuda)


def test_four_channel_view_off_alignment(cuda):
    st = np.stack([K.blobs(33, 65, 0), K.drawn(33, 65, 0.6), K.drawn(33, 65, 0.9), K.blobs(33, 65, 2)], axis=-1)[None]
    flat = torch.zeros((st.size + 1,), device=cuda)
    view = flat[1:].view(st.shape)
    view.copy_(up(st, cuda))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    both_paths(view, cuda, K.reference(st))


# ---- 2. designed planes, each also transposed
@pytest.mark.parametrize('name', sorted(K.designed()))
def test_designed_planes_equal_restatement(cuda, name):
    m = K.designed()[name]
    for plane in (m, np.ascontiguousarray(m.T)):
        both_paths(plane[None, :, :, None], cuda)


def test_hand_values_on_the_device(cuda):
    for name, (m, pixels, passes) in K.hand_cases().items():
        out, cen = skeleton.skeleton_stack(up(m[None, :, :, None], cuda), with_census=True)
        s = out.cpu().numpy()[0, :, :, 0] != 0
        if pixels is not None:
            assert sorted(zip(*(v.tolist() for v in np.nonzero(s)))) == pixels, name
        if passes is not None:
            assert int(cen[0, 0, 5]) == passes, name
    m = K.hand_cases()['disc40'][0]                                      # depth: 40 passes in one launch
    assert skeleton.census_stack(up(m[None, :, :, None], cuda)).cpu().numpy()[0, 0].tolist() == [int(m.sum()), 3, 2, 0, 0, 40]


# ---- 3. beyond LDS
def test_sparse_large_plane_takes_the_global_path(cuda):
    assert skeleton.fits_lds(750, 750) and skeleton.fits_lds(1024, 1024) and not skeleton.fits_lds(1280, 1280)
    m = K.sparse_large()
    want = K.reference(m[None, :, :, None])
    assert 1 <= want[1][0, 0, 5] <= 8                                    # a few passes: the reference stays fast
    out, cen = skeleton.skeleton_stack(up(m[None, :, :, None], cuda), with_census=True)         # path='auto'
    assert np.array_equal(cen.cpu().numpy(), want[1])
    assert np.array_equal(out.cpu().numpy(), want[0])


def test_lds_path_at_1024(cuda):
    """1024 x 1024 is the largest power of two the LDS path holds (K = 17 words per thread): a sparse plane, so the reference stays fast."""
    m = K.sparse_large(1024, seed=9)
    both_paths(m[None, :, :, None], cuda)


@pytest.mark.parametrize('k', sorted(K.LADDER_SHAPES))
def test_every_register_tile_size_of_the_lds_kernel(cuda, k):
    """One plane per instantiation skel_thin_lds_kernel<K> that no other shape here reaches: thinning, census and passes on both paths."""
    h, w = K.LADDER_SHAPES[k]
    assert skeleton.fits_lds(h, w) and K.ladder_k(h, w) == k
    both_paths(K.ladder_plane(h, w)[None, :, :, None], cuda)


# ---- 4. bounds
def test_chunking_guard_bands_and_optional_outputs(cuda):
    st = np.stack([np.stack([K.blobs(33, 65, i * 4 + k) for k in range(4)], axis=-1) for i in range(3)])
    want = K.reference(st)
    dev = up(st, cuda)
    lib = L.lib()
    one = int(lib.octseg_skeleton_scratch_bytes(1, 33, 65, 4))
    out, cen = skeleton.skeleton_stack(dev, with_census=True, scratch_bytes=one)               # one slice per chunk
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(cen.cpu().numpy(), want[1])
    assert np.array_equal(skeleton.census_stack(dev, scratch_bytes=1).cpu().numpy(), want[1])
    # guard bands: one float / six ints either side (the float band also puts `out` 4 bytes off alignment)
    need = int(lib.octseg_skeleton_scratch_bytes(3, 33, 65, 4))
    scratch = torch.empty((need,), dtype=torch.uint8, device=cuda)
    for flags in (0, 1):
        obuf = torch.full((st.size + 2,), -7.0, device=cuda)
        cbuf = torch.full((3 * 4 * 6 + 12,), -7, dtype=torch.int32, device=cuda)
        o, c = obuf[1:-1], cbuf[6:-6]
        L.check(lib.octseg_stack_skeleton(L.ptr(dev), 3, 33, 65, 4, flags, L.ptr(scratch), need, L.ptr(o), L.ptr(c), L.stream_ptr()))
        assert np.array_equal(o.cpu().numpy().reshape(st.shape), want[0]) and np.array_equal(c.cpu().numpy().reshape(3, 4, 6), want[1])
        assert obuf[0].item() == -7.0 and obuf[-1].item() == -7.0
        assert (cbuf[:6] == -7).all().item() and (cbuf[-6:] == -7).all().item()
        # each output alone
        obuf.fill_(-7.0)
        cbuf.fill_(-7)
        L.check(lib.octseg_stack_skeleton(L.ptr(dev), 3, 33, 65, 4, flags, L.ptr(scratch), need, L.ptr(o), None, L.stream_ptr()))
        L.check(lib.octseg_stack_skeleton(L.ptr(dev), 3, 33, 65, 4, flags, L.ptr(scratch), need, None, L.ptr(c), L.stream_ptr()))
        assert np.array_equal(o.cpu().numpy().reshape(st.shape), want[0]) and np.array_equal(c.cpu().numpy().reshape(3, 4, 6), want[1])
        assert obuf[0].item() == -7.0 and obuf[-1].item() == -7.0 and (cbuf[:6] == -7).all().item() and (cbuf[-6:] == -7).all().item()
    assert np.array_equal(dev.cpu().numpy(), st.astype(np.float32))                            # the input is not modified


# ---- 5. width lists
def test_width_lists_equal_the_distance_restatement(cuda):
    disc = np.pad(K.hand_cases()['disc40'][0], ((0, 0), (0, 33)))
    st = np.stack([K.blobs(97, 130, 0), disc, np.ones((97, 130), bool), np.zeros((97, 130), bool)], axis=-1)[None]
    want_skel, want_cen = K.reference(st)
    d2, off, counts = skeleton.width_lists(up(st, cuda))
    wd2, woff, wcounts = R.width_lists(st, want_skel)
    assert np.array_equal(off, woff) and np.array_equal(d2, wd2) and np.array_equal(counts, wcounts)
    # the same from the squared transform itself, at the reference skeleton's pixels
    for ch in range(2):
        full = distance_ref.edt2(~st[0, :, :, ch])
        assert np.array_equal(d2[off[ch]:off[ch + 1]], np.sort(full[want_skel[0, :, :, ch] != 0]))
    assert (d2[off[2]:off[3]] == skeleton.DIST_NONE).all() and off[3] - off[2] == want_cen[0, 2, 1] > 0 and off[4] == off[3]
    rep = skeleton.thickness_report(up(st, cuda), classes=['blobs', 'disc', 'full', 'empty'], ratio=2)
    assert rep['full']['median'] == [None] and rep['full']['centreline'] == [int(want_cen[0, 2, 1])] and rep['empty']['slice'] == []
    assert rep['disc']['max'] == [(2 * np.sqrt(float(wd2[woff[2] - 1])) - 1) / 2] and rep['disc']['passes'] == [40] and rep['disc']['ends'] == [2]


# ---- 6. the demo excerpt at 750 x 750 on the LDS path
def test_demo_excerpt_equals_restatement(cuda):
    assert skeleton.fits_lds(750, 750)
    st = K.excerpt_stack()
    want = K.excerpt_reference()
    assert want[1][1, K.LUMEN, 5] > 170                                   # one launch, over 170 passes
    dev = up(st, cuda)
    out, cen = skeleton.skeleton_stack(dev, with_census=True)
    assert np.array_equal(cen.cpu().numpy(), want[1])
    assert np.array_equal(out.cpu().numpy(), want[0])
    assert cen[1, K.CAP].tolist() == [23456, 542, 4, 5, 0, 40] and cen[2, K.VASA].tolist()[:3] == [1045, 15, 2]
    rep = skeleton.thickness_report(dev, names=['113', '114', '115'])
    cap = rep['Fibrous cap']
    assert cap['image'] == ['113', '114', '115'] and cap['centreline'][1] == 542 and cap['median'][1] == 39.0
    assert cap['min'][1] == 2 * np.sqrt(17.0) - 1 and cap['max'][1] == 2 * np.sqrt(1090.0) - 1
    d2, off, _ = R.width_lists(st, want[0])
    assert rep == json.loads(json.dumps(skeleton.build_thickness(d2, off, want[1], list(CLASS_IDS), names=['113', '114', '115'])))


# ---- 7. predict ... medial=true
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


def _files(d):
    out = {}
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), 'rb') as f:
            out[name] = f.read()
    return out


def test_predict_main_writes_medial_thickness_json(cuda, tmp_path):
    """Both input kinds: a directory of files (sorted file-name order) and a .npy volume (analyze_pullback's stack)."""
    from oct_segmentation_amd import predict, pullback
    models = _models_dir(cuda, os.path.join(tmp_path, 'models'))
    rng = np.random.default_rng(23)
    data_dir = os.path.join(tmp_path, 'input')
    os.makedirs(data_dir)
    created = ['z_last', 'a_first']                                      # sorted order differs from creation order
    for name in created:
        Image.fromarray(rng.integers(0, 255, (90, 90, 3), dtype=np.uint8)).save(os.path.join(data_dir, f'{name}.png'))
    args = [f'data_dir={data_dir}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32']
    off, on = os.path.join(tmp_path, 'off'), os.path.join(tmp_path, 'on')
    assert predict.main(args + [f'save_dir={off}']) == 0
    assert predict.main(args + [f'save_dir={on}', 'medial=true']) == 0
    a, b = _files(off), _files(on)
    assert sorted(b) == sorted(list(a) + ['medial_thickness.json'])
    for name in a:                                                       # overlays and colour masks do not change
        assert a[name] == b[name], name
    names = sorted(created)
    images, _ = predict.data_processing([os.path.join(data_dir, f'{n}.png') for n in names], [120, 120])
    stack = predict.segment_stack(images, [120, 120], list(CLASS_IDS), models, device='cuda', compute_dtype=torch.float32, device_preprocess=True)
    got = json.loads(b['medial_thickness.json'])
    assert got == json.loads(json.dumps(skeleton.thickness_report(stack, names=names)))
    host = stack.cpu().numpy()
    skel, cen = K.reference(host)
    d2, woff, _ = R.width_lists(host, skel)
    assert got == json.loads(json.dumps(skeleton.build_thickness(d2, woff, cen, list(CLASS_IDS), names=names)))
    assert any(v['slice'] for v in got.values())                         # the nets found something to report
    # the volume path
    vol = rng.integers(0, 256, (2, 90, 90, 3), dtype=np.uint8)
    np.save(os.path.join(tmp_path, 'pull.npy'), vol)
    vargs = [f'data_dir={os.path.join(tmp_path, "pull.npy")}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32']
    voff, von = os.path.join(tmp_path, 'voff'), os.path.join(tmp_path, 'von')
    assert predict.main(vargs + [f'save_dir={voff}']) == 0
    assert predict.main(vargs + [f'save_dir={von}', 'medial=true']) == 0
    a, b = _files(voff), _files(von)
    assert sorted(b) == sorted(list(a) + ['medial_thickness.json'])
    for name in a:
        assert a[name] == b[name], name
    res = pullback.analyze_pullback(vol, models, list(CLASS_IDS), output_size=(120, 120), names=['pull_001', 'pull_002'], compute_dtype=torch.float32)
    assert json.loads(b['medial_thickness.json']) == json.loads(json.dumps(skeleton.thickness_report(res.stack, names=['pull_001', 'pull_002'])))
