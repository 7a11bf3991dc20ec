"""Thinning and local thickness without a GPU: the numpy restatement (tests/skeleton_ref.py) against scipy.ndimage's component and hole counts,
the hand cases and the demo excerpt; the ABI signatures and refusals, the host half of oct_segmentation_amd/skeleton.py and the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import skeleton_cases as K
import skeleton_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import skeleton


def components(m):
    return ndimage.label(m, structure=np.ones((3, 3), int))[1]


def holes(m):
    """4-connected components of the complement of the plane padded by one clear ring, minus the outside."""
    return ndimage.label(~np.pad(m, 1, constant_values=False))[1] - 1


def planes():
    for h, w in K.SHAPES:
        for d in K.DENSITIES:
            yield f'{h}x{w}@{d}', K.drawn(h, w, d)
        yield f'{h}x{w}@blobs', K.blobs(h, w)


# ---- 1. the restatement keeps what a skeleton must keep
@pytest.mark.parametrize('name,m', list(planes()), ids=[n for n, _ in planes()])
def test_restated_thinning_keeps_topology(name, m):
    s, passes = R.thin(m)
    assert s.dtype == bool and s.shape == m.shape
    assert not (s & ~m).any()                                           # a subset of the mask
    assert components(s) == components(m)
    assert holes(s) == holes(m)
    again, zero = R.thin(s)
    assert np.array_equal(again, s) and zero == 0                       # idempotent
    assert not R.deletable(s, 0).any() and not R.deletable(s, 1).any()
    assert (passes == 0) == np.array_equal(s, m)
    cen = R.census(m, (s, passes))
    assert cen[0] == m.sum() and cen[1] == s.sum() and cen[5] == passes
    k = ndimage.convolve(s.astype(np.int32), np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]]), mode='constant')
    assert cen[2:5].tolist() == [int((s & (k == 1)).sum()), int((s & (k >= 3)).sum()), int((s & (k == 0)).sum())]


# ---- 2. hand cases: the values of the run made while the feature was specified
def test_hand_cases():
    cases = K.hand_cases()
    for name, (m, pixels, passes) in cases.items():
        s, p = R.thin(m)
        if pixels is not None:
            assert sorted(zip(*(v.tolist() for v in np.nonzero(s)))) == pixels, name
        if passes is not None:
            assert p == passes, name
    assert R.thin(cases['square2'][0])[0].sum() == 1
    assert R.thin(cases['full3x70'][0])[0].sum() == 68
    ring = cases['ring'][0]
    s = R.thin(ring)[0]
    assert components(s) == 1 and holes(s) == 1 == holes(ring)
    cen = R.census(ring)
    assert cen[2] == 0 and cen[4] == 0                                   # a closed curve has no end
    assert R.census(np.zeros((5, 9), bool)).tolist() == [0] * 6
    assert R.census(cases['bar5'][0]).tolist() == [100, 16, 2, 0, 0, 2]
    assert R.census(cases['full9'][0]).tolist() == [81, 1, 0, 0, 1, 4]


def test_even_and_odd_bars_give_the_documented_width():
    """Width 2 sqrt(d2) - 1 along the straight part of a bar: exact for 5, one short for 4."""
    for rows, want in ((5, 5.0), (4, 3.0)):
        m = np.zeros((12, 40), bool)
        m[3:3 + rows, 2:38] = True
        d2 = R.width_lists(m[None, :, :, None])[0]
        assert R.widths(d2).max() == want


# ---- 3. the demo excerpt
def test_demo_excerpt_values():
    out, cen = K.excerpt_reference()
    stack = K.excerpt_stack()
    assert cen[1, K.CAP].tolist()[:3] == [23456, 542, 4] and cen[1, K.CAP, 5] == 40
    assert cen[2, K.VASA, 1] == 15 and cen[2, K.VASA, 2] == 2
    assert cen[1, K.LUMEN, 5] > 170                                      # the deep case of the GPU test
    assert cen[0, K.VASA].tolist() == [0] * 6
    d2, off, counts = R.width_lists(stack, out)
    s = 1 * 4 + K.CAP
    cap = d2[off[s]:off[s + 1]]
    assert cap.size == 542 and cap.min() == 17 and cap.max() == 1090
    assert np.median(R.widths(cap)) == 39.0
    assert R.widths(cap).min() == pytest.approx(2 * np.sqrt(17) - 1)
    rep = skeleton.build_thickness(d2, off, cen, ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum'], names=['a', 'b', 'c'])
    capr = rep['Fibrous cap']
    assert capr['slice'] == [0, 1, 2] and capr['image'] == ['a', 'b', 'c'] and capr['centreline'][1] == 542 and capr['ends'][1] == 4
    assert capr['passes'][1] == 40 and capr['median'][1] == 39.0 and capr['min'][1] == pytest.approx(7.2462, abs=1e-4)
    assert rep['Vasa vasorum']['slice'] == [2] and rep['Vasa vasorum']['centreline'] == [15] and rep['Vasa vasorum']['ends'] == [2]
    assert rep['Lipid core']['slice'] == [1] and rep['Lumen']['slice'] == [1]
    json.dumps(rep)


# ---- 4. ABI
def test_symbols_of_the_skeleton_entry_points():
    i, p, z = C.c_int, C.c_void_p, C.c_size_t
    want = {'octseg_skeleton_scratch_bytes': (z, [i] * 4),
            'octseg_stack_skeleton': (i, [p, i, i, i, i, i, p, z, p, p, p])}
    for name, sig in want.items():
        assert L.SYMBOLS[name] == sig, name
        assert hasattr(L.lib(), name)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'octseg.h')).read()
    assert '#define OCTSEG_SKEL_GLOBAL 1' in header and skeleton.PATHS == {'auto': 0, 'global': 1}
    assert 'size_t octseg_skeleton_scratch_bytes(int N, int H, int W, int channels);' in header


def test_library_refuses_before_any_launch():
    lib = L.lib()
    fn, size = lib.octseg_stack_skeleton, lib.octseg_skeleton_scratch_bytes
    for bad in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 4097, 8, 1), (1, 8, 4097, 1), (1, 8, 8, 0), (1, 8, 8, 17), (-1, 8, 8, 1)):
        assert size(*bad) == 0, bad
    # three sets of bit planes at least: raw, skeleton, and the second image of the global path
    for n, h, w, c in ((2, 33, 65, 4), (1, 750, 750, 4), (1, 4096, 4096, 16), (3, 1, 1, 1)):
        assert size(n, h, w, c) >= 3 * n * c * h * ((w + 63) // 64) * 8
    assert size(4, 33, 65, 4) >= 2 * size(2, 33, 65, 4) - 3 * 256             # linear in the slices up to the carver's alignment
    buf = (C.c_char * 4096)()                                # a host buffer: the calls below must return before they touch a pointer
    a = C.cast(buf, C.c_void_p)
    b = C.c_void_p(a.value + 256)
    odd = C.c_void_p(a.value + 4)
    big = 1 << 40
    BAD_SHAPE, BAD_ARG = -1, -5
    assert fn(None, 1, 8, 8, 1, 0, a, big, b, b, None) == BAD_ARG
    assert fn(a, 1, 8, 8, 1, 0, None, big, b, b, None) == BAD_ARG
    assert fn(a, 1, 8, 8, 1, 0, a, big, None, None, None) == BAD_ARG
    assert b'both null' in lib.octseg_last_error()
    assert fn(a, 1, 8, 8, 1, 0, b, big, a, None, None) == BAD_ARG           # out aliases the stack
    assert b'alias' in lib.octseg_last_error()
    assert fn(a, 1, 8, 8, 1, 0, odd, big, b, None, None) == BAD_ARG
    assert b'aligned' in lib.octseg_last_error()
    assert fn(a, 1, 8, 8, 1, 0, a, 16, b, None, None) == BAD_ARG
    assert b'scratch is smaller' in lib.octseg_last_error()
    assert fn(a, 1, 8, 8, 1, 0, a, size(1, 8, 8, 1) - 1, b, None, None) == BAD_ARG
    for flags in (2, 3, 4, -1, 1 << 30):
        assert fn(a, 1, 8, 8, 1, flags, a, big, b, None, None) == BAD_ARG
        assert b'flag' in lib.octseg_last_error()
    for n, h, w, c in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, -1, 1), (1, 4097, 8, 1), (1, 8, 4097, 1), (1, 8, 8, 0), (1, 8, 8, 17)):
        assert fn(a, n, h, w, c, 0, a, big, b, None, None) == BAD_SHAPE, (n, h, w, c)
    assert not any(buf.raw)


# ---- 5. the wrappers' refusals and the host half
def test_wrappers_refuse_host_tensors_and_unknown_paths():
    cpu = torch.zeros((1, 4, 4, 4))
    for bad in (cpu, cpu.numpy(), cpu.double(), cpu[0]):
        for fn in (skeleton.skeleton_stack, skeleton.census_stack, skeleton.width_lists, skeleton.thickness_report):
            with pytest.raises(ValueError, match='float32 CUDA tensor'):
                fn(bad)
    with pytest.raises(ValueError, match='path'):
        skeleton.skeleton_stack(cpu, path='lds')
    with pytest.raises(ValueError, match='path'):
        skeleton.census_stack(cpu, path=1)


def test_build_thickness_on_hand_written_lists():
    # slice 0: class a = an odd bar (16 centreline pixels at d2 = 9 -> width 5), class b absent.
    # slice 1: class a fills its frame (no clear pixel: DIST_NONE), class b = an even bar (d2 = 4 -> 3) with one tip pixel at d2 = 1 -> 1.
    none = skeleton.DIST_NONE
    d2 = [9] * 16 + [] + [none] + [1, 4, 4, 4]
    offsets = [0, 16, 16, 17, 21]
    census = [[[100, 16, 2, 0, 0, 2], [0, 0, 0, 0, 0, 0]], [[81, 1, 0, 0, 1, 4], [20, 4, 2, 0, 0, 1]]]
    rep = skeleton.build_thickness(d2, offsets, census, ['a', 'b'])
    assert rep['a'] == {'slice': [0, 1], 'centreline': [16, 1], 'ends': [2, 0], 'junctions': [0, 0], 'passes': [2, 4],
                        'median': [5.0, None], 'mean': [5.0, None], 'min': [5.0, None], 'p5': [5.0, None], 'max': [5.0, None]}
    b = rep['b']
    assert b['slice'] == [1] and b['centreline'] == [4] and b['ends'] == [2] and b['passes'] == [1]
    assert b['median'] == [3.0] and b['min'] == [1.0] and b['max'] == [3.0] and b['mean'] == [2.5]
    assert b['p5'][0] == pytest.approx(float(np.percentile([1.0, 3.0, 3.0, 3.0], 5)), abs=1e-12)
    json.dumps(rep)
    half = skeleton.build_thickness(d2, offsets, census, ['a', 'b'], names=['s0', 's1'], ratio=2)
    assert half['a']['image'] == ['s0', 's1'] and half['b']['image'] == ['s1']
    assert half['a']['median'] == [2.5, None] and half['b']['max'] == [1.5] and half['a']['centreline'] == [16, 1]
    with pytest.raises(ValueError):
        skeleton.build_thickness(d2, offsets, census, ['a', 'b'], ratio=0)
    with pytest.raises(ValueError):
        skeleton.build_thickness(d2, offsets, census, ['a'])
    with pytest.raises(ValueError):
        skeleton.build_thickness(d2, offsets[:-1], census, ['a', 'b'])
    with pytest.raises(ValueError):
        skeleton.build_thickness(d2, [0, 15, 16, 17, 21], census, ['a', 'b'])
    with pytest.raises(ValueError):
        skeleton.build_thickness(d2, offsets, census, ['a', 'b'], names=['only one'])


# ---- 6. the command line
def test_main_on_a_tiff_directory(tmp_path, monkeypatch):
    from PIL import Image
    mask_dir, save_dir = tmp_path / 'masks', tmp_path / 'out'
    mask_dir.mkdir()
    cases = K.hand_cases()
    masks = []
    for name, lumen, cap in (('s1.tiff', cases['bar5'][0], cases['bar4'][0]), ('s0.tiff', cases['bar4'][0], np.zeros((9, 24), bool))):
        arr = np.zeros((9, 24, 4), np.uint8)
        arr[:, :, 0] = lumen * 255
        arr[:, :, 1] = cap * 255
        Image.fromarray(arr).save(str(mask_dir / name))
        masks.append((name, arr))

    def lists(stack, channels):                              # what the GPU would return, from the restatement
        out, cen = R.skeleton_stack(stack)
        d2, off, _ = R.width_lists(np.asarray(stack)[..., list(channels)], out[..., list(channels)])
        return d2, off, cen[:, list(channels)]
    monkeypatch.setattr(skeleton, '_host_lists', lists)
    report = skeleton.main([str(mask_dir), str(save_dir)])
    saved = json.load(open(save_dir / 'medial_thickness.json'))
    assert saved == json.loads(json.dumps(report))
    assert saved['images'] == ['s0.tiff', 's1.tiff'] and saved['classes'] == ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    lumen, cap = saved['thickness']['Lumen'], saved['thickness']['Fibrous cap']
    assert lumen['slice'] == [0, 1] and lumen['image'] == ['s0.tiff', 's1.tiff'] and lumen['centreline'] == [17, 16] and lumen['ends'] == [2, 2]
    assert lumen['max'] == [3.0, 5.0] and lumen['passes'] == [2, 2]
    assert cap['slice'] == [1] and cap['centreline'] == [17] and cap['max'] == [3.0]
    assert saved['thickness']['Lipid core']['slice'] == []
    assert skeleton.main([str(mask_dir)])['images'] == saved['images'] and os.path.exists(mask_dir / 'medial_thickness.json')
    with pytest.raises(SystemExit):
        skeleton.main([])
    with pytest.raises(ValueError):
        skeleton.main([str(save_dir)])
