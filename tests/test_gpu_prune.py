"""Centreline pruning on the GPU against the numpy restatement (tests/prune_ref.py): EQUALITY, no tolerance -- everything is boolean or integer.
Both paths (LDS and forced global) on every case, output and all nine census columns.  Every test runs under a watchdog of its own: a kernel
that did not return would otherwise hold the suite until the runner's limit."""
import faulthandler
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import distance_ref
import prune_cases as Q
import skeleton_cases as K
import skeleton_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import skeleton
from oct_segmentation_amd.model import CLASS_IDS

pytestmark = pytest.mark.gpu

STEP_LIMIT = 120                                             # seconds; a test here takes a few


@pytest.fixture(autouse=True)
def watchdog():
    """Ends the process (traceback of every thread, exit) when a test's GPU work does not return within the limit."""
    faulthandler.dump_traceback_later(STEP_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def up(stack, cuda):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(stack) != 0).astype(np.float32)).to(cuda)


def both_paths(stack, spur, trim, cuda, want=None):
    """The stack through both paths; each must equal the reference in output and census (and so each other).  Returns the reference."""
    want = Q.reference(stack, spur, trim) if want is None else want
    dev = stack if torch.is_tensor(stack) else up(stack, cuda)
    for path in ('auto', 'global'):
        out, cen = skeleton.prune_stack(dev, spur, trim, with_census=True, path=path)
        assert out.dtype == torch.float32 and out.shape == dev.shape and cen.dtype == torch.int32 and cen.shape == dev.shape[:1] + dev.shape[3:] + (9,)
        got, gcen = out.cpu().numpy(), cen.cpu().numpy()
        assert np.array_equal(gcen, want[1]), (path, spur, trim, gcen.tolist(), want[1].tolist())
        assert np.array_equal(got, want[0]), (path, spur, trim, int((got != want[0]).sum()))
    return want


# ---- 1. skeletons around the 64-pixel word
@pytest.mark.parametrize('h,w', [(1, 1), (1, 64), (33, 65), (64, 128), (70, 130)])
def test_skeletons_equal_restatement(cuda, h, w):
    planes = [Q.thinned(K.blobs(h, w, s)) for s in (0, 1, 2)] + [Q.thinned(K.drawn(h, w, d)) for d in K.DENSITIES]
    for (n, c), (spur, trim) in zip(((1, 1), (3, 4), (1, 5), (3, 1), (1, 4)), ((3, 0), (4, 3), (0, 6), (8, 0), (1, 2))):
        st = np.stack([np.stack([planes[(i * c + k) % len(planes)] for k in range(c)], axis=-1) for i in range(n)])
        both_paths(st, spur, trim, cuda)
    one = planes[0][None, :, :, None]
    want = both_paths(one, 0, 0, cuda)
    assert np.array_equal(want[0], one.astype(np.float32))                                  # (0, 0) is the identity


def test_four_channel_view_off_alignment(cuda):
    st = np.stack([Q.thinned(K.blobs(33, 65, 0)), Q.thinned(K.drawn(33, 65, 0.6)), Q.thinned(K.drawn(33, 65, 0.9)), Q.thinned(K.blobs(33, 65, 2))],
                  axis=-1)[None]
    flat = torch.zeros((st.size + 1,), device=cuda)
    view = flat[1:].view(st.shape)
    view.copy_(up(st, cuda))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    both_paths(view, 4, 3, cuda, Q.reference(st, 4, 3))


# ---- 2. designed planes, each also transposed: the hand cases, stubs and tips on columns 63 / 64 / 65 and on every frame edge, a raw plane,
# spur or trim larger than the object
@pytest.mark.parametrize('name', sorted(Q.designed()))
def test_designed_planes_equal_restatement(cuda, name):
    m, pairs = Q.designed()[name]
    for plane in (m, np.ascontiguousarray(m.T)):
        for spur, trim in pairs:
            both_paths(plane[None, :, :, None], spur, trim, cuda)


def test_hand_values_on_the_device(cuda):
    for name, m, spur, trim, pixels, tips, links, restored in Q.hand_values():
        for plane in (m, np.ascontiguousarray(m.T)):
            cen = skeleton.prune_stack(up(plane[None, :, :, None], cuda), spur, trim, with_census=True)[1].cpu().numpy()[0, 0]
            assert cen[0] == m.sum() and cen[1] == pixels and (cen[6], cen[7]) == links and cen[8] == restored, (name, spur, trim, cen.tolist())
            if tips is not None:
                assert cen[2] == tips, (name, spur, trim)
    ring = Q.thin_ring()
    out = skeleton.prune_stack(up(ring[None, :, :, None], cuda), 10, 10)
    assert np.array_equal(out.cpu().numpy()[0, :, :, 0] != 0, ring)
    cen = torch.tensor([[[0, 0, 0, 0, 0, 0, 3, 2, 0]]], dtype=torch.int32, device=cuda)
    assert skeleton.centreline_length(cen)[0, 0] == 3 + 2 * np.sqrt(2.0)


def test_spur_and_trim_larger_than_the_object(cuda):
    st = np.stack([Q.thinned(K.blobs(33, 65, 0)), Q.thinned(K.blobs(33, 65, 1))], axis=-1)[None]
    for spur, trim in ((200, 0), (0, 200), (8192, 8192)):
        want = both_paths(st, spur, trim, cuda)
        assert (want[1][:, :, 1] > 0).all()                                                  # a centreline is never lost


# ---- 3. bounds
def test_chunking_guard_bands_and_optional_outputs(cuda):
    st = np.stack([np.stack([Q.thinned(K.blobs(33, 65, i * 4 + k)) for k in range(4)], axis=-1) for i in range(3)])
    want = Q.reference(st, 4, 3)
    dev = up(st, cuda)
    lib = L.lib()
    one = int(lib.octseg_prune_scratch_bytes(1, 33, 65, 4))
    out, cen = skeleton.prune_stack(dev, 4, 3, with_census=True, scratch_bytes=one)            # one slice per chunk
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(cen.cpu().numpy(), want[1])
    out, cen = skeleton.prune_stack(dev, 4, 3, with_census=True, scratch_bytes=1)
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(cen.cpu().numpy(), want[1])
    # guard bands: one float / nine ints either side (the float band also puts `out` 4 bytes off alignment)
    need = int(lib.octseg_prune_scratch_bytes(3, 33, 65, 4))
    scratch = torch.empty((need,), dtype=torch.uint8, device=cuda)
    for flags in (0, 1):
        obuf = torch.full((st.size + 2,), -7.0, device=cuda)
        cbuf = torch.full((3 * 4 * 9 + 18,), -7, dtype=torch.int32, device=cuda)
        o, c = obuf[1:-1], cbuf[9:-9]
        L.check(lib.octseg_stack_prune(L.ptr(dev), 3, 33, 65, 4, 4, 3, flags, L.ptr(scratch), need, L.ptr(o), L.ptr(c), L.stream_ptr()))
        assert np.array_equal(o.cpu().numpy().reshape(st.shape), want[0]) and np.array_equal(c.cpu().numpy().reshape(3, 4, 9), want[1])
        assert obuf[0].item() == -7.0 and obuf[-1].item() == -7.0
        assert (cbuf[:9] == -7).all().item() and (cbuf[-9:] == -7).all().item()
        # each output alone
        obuf.fill_(-7.0)
        cbuf.fill_(-7)
        L.check(lib.octseg_stack_prune(L.ptr(dev), 3, 33, 65, 4, 4, 3, flags, L.ptr(scratch), need, L.ptr(o), None, L.stream_ptr()))
        L.check(lib.octseg_stack_prune(L.ptr(dev), 3, 33, 65, 4, 4, 3, flags, L.ptr(scratch), need, None, L.ptr(c), L.stream_ptr()))
        assert np.array_equal(o.cpu().numpy().reshape(st.shape), want[0]) and np.array_equal(c.cpu().numpy().reshape(3, 4, 9), want[1])
        assert obuf[0].item() == -7.0 and obuf[-1].item() == -7.0 and (cbuf[:9] == -7).all().item() and (cbuf[-9:] == -7).all().item()
    assert np.array_equal(dev.cpu().numpy(), st.astype(np.float32))                            # the input is not modified


# ---- 4. the demo excerpt's cap planes at 750 x 750 on the LDS path
def test_demo_excerpt_cap_planes(cuda):
    assert skeleton.fits_lds(750, 750)
    skel = Q.excerpt_skeleton()
    caps = np.ascontiguousarray(skel[:, :, :, K.CAP:K.CAP + 1])
    dev = up(caps, cuda)
    for spur, trim in ((0, 0), (0, 20), (10, 0), (10, 20)):
        both_paths(dev, spur, trim, cuda, Q.reference(caps, spur, trim))
    cen = skeleton.prune_stack(dev, 0, 0, with_census=True)[1].cpu().numpy()[:, 0]
    assert cen[:, 1].tolist() == [444, 542, 378] and cen[:, 6:8].tolist() == [[286, 157], [319, 222], [233, 144]]
    assert skeleton.prune_stack(dev, 0, 20, with_census=True)[1].cpu().numpy()[:, 0, 1].tolist() == [358, 464, 318]
    c10 = skeleton.prune_stack(dev, 10, 0, with_census=True)[1].cpu().numpy()[0, 0]
    assert c10[1] == 435 and c10[2] == 4


# ---- 5. at and beyond the LDS limit
def test_lds_path_at_1024(cuda):
    """1024 x 1024 is the largest power of two the LDS path holds (K = 17 words per thread): a sparse plane, so the reference stays fast."""
    assert skeleton.fits_lds(1024, 1024)
    s = Q.sparse_skeleton(1024, 9)
    both_paths(s[None, :, :, None], 6, 10, cuda)


@pytest.mark.parametrize('k', sorted(K.LADDER_SHAPES))
def test_every_register_tile_size_of_the_lds_kernel(cuda, k):
    """One skeleton per instantiation prune_lds_kernel<K> that no other shape here reaches: output and census on both paths."""
    h, w = K.LADDER_SHAPES[k]
    assert skeleton.fits_lds(h, w) and K.ladder_k(h, w) == k
    both_paths(Q.ladder_skeleton(k)[None, :, :, None], 3, 5, cuda)


def test_sparse_large_plane_takes_the_global_path(cuda):
    assert not skeleton.fits_lds(1280, 1280)
    s = Q.sparse_skeleton(1280, 5)
    want = Q.reference(s[None, :, :, None], 6, 10)
    out, cen = skeleton.prune_stack(up(s[None, :, :, None], cuda), 6, 10, with_census=True)     # path='auto'
    assert np.array_equal(cen.cpu().numpy(), want[1])
    assert np.array_equal(out.cpu().numpy(), want[0])


# ---- 6. the report
def test_thickness_report_with_pruning_equals_the_reference_lists(cuda):
    st = K.excerpt_stack()
    skel, cen = K.excerpt_reference()
    dev = up(st, cuda)
    names = ['113', '114', '115']
    plain = skeleton.thickness_report(dev, names=names)
    assert skeleton.thickness_report(dev, names=names, spur=0, trim=0) == plain
    assert list(plain['Fibrous cap']) == ['slice', 'image', 'centreline', 'ends', 'junctions', 'passes', 'median', 'mean', 'min', 'p5', 'max']
    rep = skeleton.thickness_report(dev, names=names, trim=20, ratio=2.0)
    cut, pc = Q.reference(skel, 0, 20)
    d2, off, _ = R.width_lists(st, cut)
    assert rep == json.loads(json.dumps(skeleton.build_pruned_thickness(d2, off, cen, pc, list(CLASS_IDS), names=names, ratio=2.0)))
    cap = rep['Fibrous cap']
    assert cap['centreline'] == [358, 464, 318] and cap['removed'] == [444 - 358, 542 - 464, 378 - 318] and cap['restored'] == [0, 0, 0]
    assert [2 * m for m in cap['min']] == pytest.approx([19.59, 19.59, 21.80], abs=5e-3)
    assert plain['Fibrous cap']['min'] == [2 * np.sqrt(17.0) - 1] * 3
    assert cap['length'] == [float(v) / 2.0 for v in skeleton.centreline_length(pc[:, K.CAP])]
    full = distance_ref.edt2(~st[1, :, :, K.CAP])                        # the same from the squared transform itself
    assert cap['min'][1] == (2 * np.sqrt(float(full[cut[1, :, :, K.CAP] != 0].min())) - 1) / 2.0


# ---- 7. predict ... medial=true medial_trim=20
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


def test_predict_main_passes_spur_and_trim_on(cuda, tmp_path):
    from oct_segmentation_amd import predict
    models = _models_dir(cuda, os.path.join(tmp_path, 'models'))
    rng = np.random.default_rng(23)
    data_dir = os.path.join(tmp_path, 'input')
    os.makedirs(data_dir)
    created = ['z_last', 'a_first']                                      # sorted order differs from creation order
    for name in created:
        Image.fromarray(rng.integers(0, 255, (90, 90, 3), dtype=np.uint8)).save(os.path.join(data_dir, f'{name}.png'))
    args = [f'data_dir={data_dir}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32']
    plain, zero, on = (os.path.join(tmp_path, d) for d in ('plain', 'zero', 'on'))
    assert predict.main(args + [f'save_dir={plain}', 'medial=true']) == 0
    assert predict.main(args + [f'save_dir={zero}', 'medial=true', 'medial_spur=0', 'medial_trim=0']) == 0
    assert predict.main(args + [f'save_dir={on}', 'medial=true', 'medial_trim=20', 'medial_spur=3']) == 0
    a, z, b = _files(plain), _files(zero), _files(on)
    assert sorted(a) == sorted(b) == sorted(z) and 'medial_thickness.json' in a
    for name in a:                                                       # without the new keys every file is byte for byte what it was
        assert a[name] == z[name], name
        if name != 'medial_thickness.json':
            assert a[name] == b[name], name
    names = sorted(created)
    images, _ = predict.data_processing([os.path.join(data_dir, f'{n}.png') for n in names], [120, 120])
    stack = predict.segment_stack(images, [120, 120], list(CLASS_IDS), models, device='cuda', compute_dtype=torch.float32, device_preprocess=True)
    assert a['medial_thickness.json'] == json.dumps(skeleton.thickness_report(stack, names=names)).encode()
    got = json.loads(b['medial_thickness.json'])
    assert got['spur'] == 3 and got['trim'] == 20 and list(got)[:2] == ['spur', 'trim']
    host = stack.cpu().numpy()
    skel, cen = K.reference(host)
    cut, pc = Q.reference(skel, 3, 20)
    d2, woff, _ = R.width_lists(host, cut)
    want = skeleton.build_pruned_thickness(d2, woff, cen, pc, list(CLASS_IDS), names=names)
    assert got == json.loads(json.dumps({'spur': 3, 'trim': 20, **want}))
    assert any(got[c]['slice'] for c in CLASS_IDS)                       # the nets found something to report
