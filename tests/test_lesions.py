"""Lesions in 3-D without a GPU: the ABI's declarations and refusals, the wrappers' argument checks, the scipy reference the GPU tests hold the
kernels to (tests/lesions_ref.py) on hand-made volumes, build_report on hand-written tables, and the reference's counts on the demo excerpt
tests/golden/pullback_demo_excerpt.npz."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lesions_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import lesions

HERE = os.path.dirname(os.path.abspath(__file__))


def test_library_exports_the_new_symbols_with_the_declared_signatures():
    lib = L.lib()
    _P = C.c_void_p
    want = {'octseg_lesions_scratch_bytes': (C.c_size_t, [C.c_int] * 4),
            'octseg_volume_components': (C.c_int, [_P] + [C.c_int] * 5 + [_P, C.c_size_t, _P, _P, _P, _P, _P]),
            'octseg_volume_cleanup': (C.c_int, [_P] + [C.c_int] * 8 + [_P, C.c_size_t, _P, _P, _P, _P])}
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'octseg.h')).read()
    for name, (res, args) in want.items():
        assert hasattr(lib, name), name
        assert L.SYMBOLS[name] == (res, args)
        assert f'{name}(' in header
    assert ' *   octseg_volume_components / octseg_volume_cleanup / octseg_lesions_scratch_bytes\n' in header      # the table at the top
    assert '#define OCTSEG_ACROSS_OVERLAP 0' in header and '#define OCTSEG_ACROSS_FULL 1' in header
    assert lesions.ACROSS == {'overlap': 0, 'full': 1}


def test_abi_argument_checks_need_no_gpu():
    lib = L.lib()
    one = 8      # any non-null, 8-byte aligned pointer value: every refusal below happens before any HIP call
    big = 1 << 50
    sb = lib.octseg_lesions_scratch_bytes
    assert sb(0, 2, 4, 4) == 0 and sb(17, 2, 4, 4) == 0 and sb(1, 0, 4, 4) == 0 and sb(1, 2, 0, 4) == 0 and sb(1, 2, 4, -1) == 0
    assert sb(1, 1 << 11, 1 << 10, 1 << 10) == 0 and sb(1, 2, 1 << 15, 1 << 15) == 0                 # N * H * W = 2^31
    assert sb(1, 1, 2 ** 31 - 1, 1) == 0 and sb(1, 1, 2 ** 31 - 2, 1) > 0                             # refused from 2^31 - 1 on
    # parent + vox + zmax (4 B per voxel each), the lesion list (N * ceil(H / 2) * ceil(W / 2) entries), the count and the threshold per channel,
    # 32 ranked roots per channel, two sets of bits; every part rounded up to 256 bytes
    al = lambda v: (v + 255) // 256 * 256                                                          # noqa: E731
    assert sb(2, 3, 5, 70) == 3 * al(2 * 3 * 350 * 4) + al(2 * 3 * 3 * 35 * 4) + 2 * al(2 * 4) + al(2 * 32 * 4) + 2 * al(2 * 3 * 5 * 2 * 8)

    def comp(stack=one, N=2, H=4, W=4, ch=4, across=0, scratch=one, nbytes=big, labels=one, nles=None, top=None, profile=None):
        return lib.octseg_volume_components(stack, N, H, W, ch, across, scratch, nbytes, labels, nles, top, profile, None)

    def clean(stack=one, N=2, H=4, W=4, ch=4, across=0, keep=0, min_voxels=0, min_slices=2, scratch=one, nbytes=big, out=16):
        return lib.octseg_volume_cleanup(stack, N, H, W, ch, across, keep, min_voxels, min_slices, scratch, nbytes, out, None, None, None)

    for call in (comp, clean):
        assert call(stack=None) == -5 and call(scratch=None) == -5 and call(scratch=12) == -5
        for kw in ({'N': 0}, {'H': 0}, {'W': -1}, {'ch': 0}, {'ch': 17}, {'N': 2, 'H': 1 << 15, 'W': 1 << 15}, {'N': 1, 'H': 2 ** 31 - 1, 'W': 1}):
            assert call(**kw) == -1, kw
        assert call(nbytes=sb(4, 2, 4, 4) - 1) == -5
        assert call(across=2) == -5 and call(across=-1) == -5
        assert b'across' in lib.octseg_last_error()
    assert comp(labels=None) == -5                                                  # no output requested
    assert b'no output' in lib.octseg_last_error()
    assert clean(out=None) == -5 and clean(out=one) == -5                           # null / aliasing output
    assert clean(keep=-1) == -5 and clean(min_voxels=-1) == -5
    assert clean(min_slices=0) == -5 and clean(min_slices=-3) == -5
    assert b'min_slices' in lib.octseg_last_error()


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    host = torch.zeros((2, 4, 4, 4))
    for fn in (lesions.label_volume, lesions.lesion_table, lesions.clean_volume, lesions.lesion_report):
        with pytest.raises(ValueError, match='float32 CUDA tensor'):
            fn(host)
        with pytest.raises(ValueError, match='float32 CUDA tensor'):
            fn(np.zeros((2, 4, 4, 4), np.float32))
        with pytest.raises(ValueError, match='float32 CUDA tensor'):
            fn(torch.zeros((2, 4, 4, 4), dtype=torch.float64))                      # wrong dtype (and host)
        with pytest.raises(ValueError, match='float32 CUDA tensor'):
            fn(torch.zeros((4, 4, 4)))                                              # wrong rank
        for bad in ('6', 'OVERLAP', 26, None):
            with pytest.raises(ValueError, match='across'):
                fn(host, across=bad)
    with pytest.raises(ValueError, match='min_slices'):
        lesions.clean_volume(host, min_slices=0)
    with pytest.raises(ValueError, match='negative'):
        lesions.clean_volume(host, keep=-1)
    with pytest.raises(ValueError, match='negative'):
        lesions.clean_volume(host, min_voxels=-1)
    assert lesions.clean_kwargs(None) is None and lesions.clean_kwargs(False) is None and lesions.clean_kwargs(True) == {}
    assert lesions.clean_kwargs({'min_slices': 3}) == {'min_slices': 3}
    with pytest.raises(ValueError):
        lesions.clean_kwargs({'smooth': 3})
    with pytest.raises(ValueError):
        lesions.clean_kwargs('yes')
    assert lesions.default_classes(5) == ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum', 'channel_4']


# ---- the reference on hand-made volumes
def test_reference_structures():
    assert R.structure('full').sum() == 27 and R.structure('overlap').sum() == 11
    assert R.structure('overlap')[1].all() and R.structure('overlap')[0].sum() == 1 and R.structure('overlap')[0, 1, 1] == 1


def test_reference_staircase_checkerboard_and_join():
    n, h, w = 4, 3, 70
    stair = np.zeros((n, h, w), np.uint8)
    for z in range(n):
        stair[z, 1, 62 + z] = 1                                                      # one pixel moving +1 in x per slice across the 63 / 64 seam
    assert len(R.lesions(stair, 'full')) == 1 and len(R.lesions(stair, 'overlap')) == n
    assert R.lesions(stair, 'full')[0] == (4, 1 * w + 62, 0, 3, 1, 1, 62, 65)
    assert [r[1] for r in R.lesions(stair, 'overlap')] == [z * h * w + w + 62 + z for z in range(n)]    # equal sizes: first voxel ascending
    zz, yy, xx = np.mgrid[:3, :5, :6]
    checker = (zz + yy + xx) % 2 == 0
    assert len(R.lesions(checker, 'overlap')) == 3 and len(R.lesions(checker, 'full')) == 1
    join = np.zeros((3, 4, 9), np.uint8)
    join[:, :, 1] = 1
    join[:, :, 7] = 1
    join[2, 2, 1:8] = 1                                                              # two columns that meet in the last slice only
    lab = R.canonical_labels(join)
    assert set(np.unique(lab)) == {0, 2} and lab[0, 0, 7] == 2                       # the label is the smallest index, in slice 0
    assert (R.canonical_labels(join[:2]) == 8)[:, :, 7].all()
    gap = np.zeros((5, 2, 2), np.uint8)
    gap[::2] = 1                                                                     # present in every second slice only
    assert [r[:4] for r in R.lesions(gap, 'full')] == [(4, 0, 0, 0), (4, 8, 2, 2), (4, 16, 4, 4)]
    assert R.lesions(np.zeros((2, 3, 3)), 'full') == [] and not R.canonical_labels(np.zeros((2, 3, 3))).any()
    assert R.lesions(np.ones((2, 3, 3)), 'overlap') == [(18, 0, 0, 1, 0, 2, 0, 2)]


def flicker_volume():
    """[5, 12, 20]: a persistent blob in slices 0..4, a speck alone in slice 2 and a speck in slice 3 that overlaps the blob of slice 4 only."""
    v = np.zeros((5, 12, 20), np.uint8)
    v[:, 2:6, 2:6] = 1
    v[3, 2:6, 2:6] = 0
    v[3, 2:6, 3:6] = 1
    v[2, 9, 15] = 1                      # flicker
    v[3, 3, 2] = 0
    v[4, 8, 8:10] = 1
    v[3, 8, 9] = 1                       # a speck with a neighbour slice: stays
    return v


def test_reference_keep_rule_and_profile():
    v = flicker_volume()
    rows = R.lesions(v)
    assert [r[0] for r in rows] == [16 * 4 + 12, 3, 1] and rows[2][1:4] == (2 * 240 + 9 * 20 + 15, 2, 2)
    kept = R.clean(v, min_slices=2)
    assert kept.sum() == v.sum() - 1 and kept[2, 9, 15] == 0 and kept[3, 8, 9] == 1
    assert R.clean(v, min_slices=1).sum() == v.sum() and R.clean(v, min_slices=3).sum() == 76 and R.clean(v, min_slices=6).sum() == 0
    assert R.clean(v, min_slices=1, min_voxels=2).sum() == v.sum() - 1 and R.clean(v, min_slices=1, keep=1).sum() == 76
    assert R.threshold([5, 3, 3, 3, 3, 1], 2) == 3 and R.threshold([5, 3], 3) == 0 and R.threshold([5, 9], 0, 6) == 6
    nles, top, prof = R.table(v)
    assert nles == 3 and prof[0].tolist() == [16, 16, 16, 12, 16] and prof[1].tolist() == [0, 0, 0, 1, 2] and prof[2].tolist() == [0, 0, 1, 0, 0]
    assert top[1].tolist() == [3, 3 * 240 + 8 * 20 + 9, 3, 4, 8, 8, 8, 9] and not top[3:].any() and not prof[3:].any()
    lab, n2, top2, prof2 = R.analyse(v)
    assert np.array_equal(lab, R.canonical_labels(v)) and n2 == 3 and np.array_equal(top2, top) and np.array_equal(prof2, prof)


# ---- build_report
def test_build_report_on_hand_written_tables():
    h, w, n = 10, 20, 6
    nles = np.array([2, 0, 40], np.int32)
    top = np.zeros((3, 32, 8), np.int32)
    prof = np.zeros((3, 32, n), np.int32)
    top[0, 0] = [30, 1 * 200 + 2 * 20 + 3, 1, 3, 2, 5, 3, 9]
    prof[0, 0] = [0, 8, 14, 8, 0, 0]
    top[0, 1] = [5, 4 * 200 + 7, 4, 4, 0, 0, 7, 11]
    prof[0, 1] = [0, 0, 0, 0, 5, 0]
    for r in range(32):
        top[2, r] = [2, r * 2, 0, 0, 0, 0, 2 * r % 20, 2 * r % 20 + 1]
        prof[2, r, 0] = 2
    names = [f's{i}' for i in range(n)]
    rep = lesions.build_report(nles, top, prof, h, w, image_names=names, classes=['a', 'b', 'c'], ratio=4)
    assert list(rep) == ['a', 'b', 'c'] and json.loads(json.dumps(rep)) == rep
    assert rep['b'] == {'n_lesions': 0, 'truncated': False, 'lesions': []}
    assert rep['c']['n_lesions'] == 40 and rep['c']['truncated'] is True and len(rep['c']['lesions']) == 32
    assert rep['a']['truncated'] is False
    a0, a1 = rep['a']['lesions']
    assert a0 == {'id': 0, 'first_slice': 1, 'last_slice': 3, 'length': 3, 'voxels': 30, 'first_voxel': [1, 2, 3],
                  'bbox': {'z0': 1, 'z1': 3, 'y0': 2, 'y1': 5, 'x0': 3, 'x1': 9}, 'area': [8, 14, 8], 'peak_area': 14, 'peak_slice': 2,
                  'first_image': 's1', 'last_image': 's3', 'area_ratio': [pow(2, 0.5), pow(3, 0.5), pow(2, 0.5)], 'peak_area_ratio': pow(3, 0.5)}
    assert a1['id'] == 1 and a1['length'] == 1 and a1['area'] == [5] and a1['peak_slice'] == 4 and a1['area_ratio'] == [1.0]
    plain = lesions.build_report(nles[:2], top[:2], prof[:2], h, w)
    assert list(plain) == ['Lumen', 'Fibrous cap'] and 'area_ratio' not in plain['Lumen']['lesions'][0] and 'first_image' not in plain['Lumen']['lesions'][0]
    tie = prof.copy()
    tie[0, 0] = [0, 14, 14, 8, 0, 0]
    assert lesions.build_report(nles, top, tie, h, w)['Lumen']['lesions'][0]['peak_slice'] == 1        # the first slice of the largest area
    for bad in (dict(image_names=names[:-1]), dict(classes=['a', 'b']), dict(classes=['a', 'a', 'b']), dict(ratio=0)):
        with pytest.raises(ValueError):
            lesions.build_report(nles, top, prof, h, w, **bad)
    with pytest.raises(ValueError):
        lesions.build_report(nles, top[:, :8], prof, h, w)
    with pytest.raises(ValueError):
        lesions.build_report(nles, top, prof[:2], h, w)


# ---- the demo excerpt
def test_reference_counts_on_the_golden_excerpt():
    stack, names, recorded = R.golden_stack()
    assert stack.shape == (48, 750, 750, 4) and len(names) == 48
    classes = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    planes = [sum(R.ndimage.label(stack[z, :, :, c], structure=np.ones((3, 3)))[1] for z in range(48)) for c in range(4)]
    assert planes == [50, 10, 10, 46]                                                # 2-D components, slice by slice
    want = {'overlap': [1, 5, 5, 17], 'full': [1, 5, 5, 16]}
    for across in ('overlap', 'full'):
        nles, top, prof = R.golden_table(across)
        assert nles.tolist() == want[across] and (nles <= 32).all()
        assert top[:, 0, 0].tolist() == [4365762, 58721, 271842, 13183]              # the largest lesion of every class
        assert [int((top[c, :nles[c], 2] == top[c, :nles[c], 3]).sum()) for c in range(4)] == [0, 1, 1, 9]      # one-slice lesions
        assert np.array_equal(prof.sum(axis=1).T, stack.reshape(48, -1, 4).sum(axis=1))                      # every set pixel is in a ranked lesion
        for c, name in enumerate(classes):
            covered = set()
            for z0, z1 in top[c, :nles[c], 2:4]:
                covered |= set(range(int(z0), int(z1) + 1))
            assert sorted(covered) == recorded['objects'][name]['slice'], name      # the slices the app's record lists as present
        rep = lesions.build_report(nles, top, prof, 750, 750, image_names=names, ratio=recorded['ratio'])
        assert [rep[k]['n_lesions'] for k in classes] == want[across] and not any(rep[k]['truncated'] for k in classes)
        lumen = rep['Lumen']['lesions'][0]
        assert lumen['length'] == 48 and lumen['first_image'] == '001_1_085' and lumen['area_ratio'] == recorded['objects']['Lumen']['area']
