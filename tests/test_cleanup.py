"""Mask clean-up without a GPU: the ABI's declarations and refusals, the wrappers' argument checks, and the scipy reference the GPU tests hold
the kernels to (tests/cleanup_ref.py) on hand-made planes and on the demo planes of tests/golden/cleanup_demo_masks.npz."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import cleanup_ref as R
from cleanup_ref import golden_planes, salt
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import cleanup
from oct_segmentation_amd.postprocess import ellipse

HERE = os.path.dirname(os.path.abspath(__file__))


def test_library_exports_the_new_symbols_with_the_declared_signatures():
    lib = L.lib()
    _P = C.c_void_p
    want = {'octseg_components_scratch_bytes': (C.c_size_t, [C.c_int] * 3),
            'octseg_stack_components': (C.c_int, [_P] + [C.c_int] * 4 + [_P, C.c_size_t, _P, _P, _P, _P]),
            'octseg_stack_cleanup': (C.c_int, [_P] + [C.c_int] * 8 + [_P, C.c_size_t, _P, _P, _P, _P])}
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'octseg.h')).read()
    for name, (res, args) in want.items():
        assert hasattr(lib, name), name
        assert L.SYMBOLS[name] == (res, args)
        assert f'{name}(' in header


def test_abi_argument_checks_need_no_gpu():
    lib = L.lib()
    one = 8      # any non-null, 8-byte aligned pointer value: every refusal below happens before a launch
    big = 1 << 40
    assert lib.octseg_components_scratch_bytes(0, 4, 4) == 0 and lib.octseg_components_scratch_bytes(1, 0, 4) == 0
    assert lib.octseg_components_scratch_bytes(1, 1 << 16, 1 << 15) == 0            # H * W = 2^31
    need = lib.octseg_components_scratch_bytes(2, 5, 70)
    # parent + area (4 B per pixel each), the component list, two counters per plane, two bit planes; every part rounded up to 256 bytes
    al = lambda v: (v + 255) // 256 * 256                                           # noqa: E731
    assert need == 2 * al(2 * 350 * 4) + al(2 * 3 * 35 * 4) + 2 * al(2 * 4) + 2 * al(2 * 5 * 2 * 8)

    def comp(stack=one, N=1, H=4, W=4, ch=4, scratch=one, nbytes=big, labels=one, ncomp=None, top=None):
        return lib.octseg_stack_components(stack, N, H, W, ch, scratch, nbytes, labels, ncomp, top, None)

    def clean(stack=one, N=1, H=4, W=4, ch=4, k=0, keep=3, min_area=0, fill=1, scratch=one, nbytes=big, out=16):
        return lib.octseg_stack_cleanup(stack, N, H, W, ch, k, keep, min_area, fill, scratch, nbytes, out, None, None, None)

    for call in (comp, clean):
        assert call(stack=None) == -5 and call(scratch=None) == -5 and call(scratch=12) == -5
        for kw in ({'N': 0}, {'H': 0}, {'W': -1}, {'ch': 0}, {'ch': 17}, {'H': 1 << 16, 'W': 1 << 15}):
            assert call(**kw) == -1, kw
        assert call(nbytes=lib.octseg_components_scratch_bytes(4, 4, 4) - 1) == -5
    assert comp(labels=None) == -5                                                  # no output requested
    assert clean(out=None) == -5 and clean(out=one) == -5                           # null / aliasing output
    assert clean(k=8) == -1 and clean(k=-1) == -1
    assert clean(keep=-1) == -5 and clean(min_area=-1) == -5
    assert b'smooth_k' in lib.octseg_last_error() or b'keep' in lib.octseg_last_error()


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    host = torch.zeros((1, 4, 4, 4))
    for fn in (cleanup.label_stack, cleanup.component_table, cleanup.smooth_stack, cleanup.keep_largest, cleanup.clean_stack):
        with pytest.raises(ValueError):
            fn(host)
        with pytest.raises(ValueError):
            fn(np.zeros((1, 4, 4, 4), np.float32))
    with pytest.raises(ValueError):
        cleanup.label_stack(host, connectivity=4)
    assert cleanup.smooth_kernel_size(400, 600) == 2 and cleanup.smooth_kernel_size(750, 750) == 3 and cleanup.smooth_kernel_size(100, 100) == 1
    assert cleanup.smooth_kernel_size(1000, 1000) == 5 and cleanup.smooth_kernel_size(1600, 2000) == 8
    assert cleanup.clean_kwargs(None) is None and cleanup.clean_kwargs(False) is None and cleanup.clean_kwargs(True) == {}
    assert cleanup.clean_kwargs({'keep': 1}) == {'keep': 1}
    with pytest.raises(ValueError):
        cleanup.clean_kwargs({'keeps': 1})
    with pytest.raises(ValueError):
        cleanup.clean_kwargs('yes')


def test_ellipse_of_even_size():
    assert ellipse(2).tolist() == [[0, 1], [1, 1]]
    assert ellipse(4).tolist() == [[0, 0, 1, 0], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
    for k in range(1, 8):
        assert np.array_equal(ellipse(k), R.ellipse(k)), k


def _boxes(h, w, boxes):
    m = np.zeros((h, w), np.uint8)
    for y, x, bh, bw in boxes:
        m[y:y + bh, x:x + bw] = 1
    return m


def test_reference_tie_rule():
    # areas 664, 477, 144, 144: keep = 3 keeps four components (the reference's `area in sorted_areas`)
    m = _boxes(60, 120, [(0, 0, 8, 83), (10, 0, 9, 53), (30, 0, 12, 12), (30, 20, 12, 12), (50, 0, 2, 5)])
    assert [r[0] for r in R.components(m)] == [664, 477, 144, 144, 10]
    assert R.threshold([664, 477, 144, 144, 10], 3) == 144 and R.threshold([664, 477], 3) == 0 and R.threshold([5, 9], 0, 6) == 6
    kept = R.keep_largest(m, 3, 0, False)
    assert kept.sum() == 664 + 477 + 144 + 144 and R.table(kept)[0] == 4
    assert R.keep_largest(m, 2, 0, False).sum() == 664 + 477
    assert R.keep_largest(m, 100, 0, False).sum() == m.sum()                       # more than exist: everything stays
    assert R.keep_largest(m, 0, 145, False).sum() == 664 + 477
    # the table: area descending, then first pixel ascending
    n, top = R.table(m)
    assert n == 5 and top[2].tolist() == [144, 30 * 120, 0, 30, 11, 41] and top[3].tolist() == [144, 30 * 120 + 20, 20, 30, 31, 41]
    assert not top[5:].any()


def test_reference_labels_and_fill():
    m = _boxes(9, 9, [(1, 1, 5, 5)])
    m[2:5, 2:5] = 0
    m[3, 3] = 1                  # an island inside the hole
    m[7, 7] = 1
    m[6, 6] = 1                  # touches the ring's corner diagonally: one 8-connected component with the ring
    lab = R.canonical_labels(m)
    assert sorted(np.unique(lab).tolist()) == [0, 1 + 1 * 9 + 1, 1 + 3 * 9 + 3]
    assert lab[7, 7] == lab[1, 1] == 11
    filled = R.keep_largest(m, 0, 0, True)
    assert filled[2:5, 2:5].all() and filled.sum() == 25 + 2
    u = _boxes(9, 9, [(0, 2, 6, 5)])
    u[0:5, 3:6] = 0              # a ring whose opening lies on the frame border: its inside is no hole
    assert np.array_equal(R.keep_largest(u, 0, 0, True), u)
    yy, xx = np.mgrid[:37, :53]
    checker = ((yy + xx) % 2 == 0).astype(np.uint8)
    assert R.table(checker)[0] == 1 and int((checker == 0).sum()) == 980
    assert int(R.keep_largest(checker, 0, 0, True).sum() - checker.sum()) == 892


@pytest.mark.parametrize('k', range(2, 8))
def test_smoothing_definition_agrees_with_scipy_rank_filters(k):
    rng = np.random.RandomState(k)
    for h, w in ((37, 53), (20, 9)):
        for density in (0.5, 0.9, 0.1):
            m = (rng.rand(h, w) < density).astype(np.uint8)
            fp = R.ellipse(k)
            assert np.array_equal(R._morph(m, fp, True), ndimage.minimum_filter(m, footprint=fp, mode='constant', cval=1).astype(bool))
            assert np.array_equal(R._morph(m, fp, False), ndimage.maximum_filter(m, footprint=fp, mode='constant', cval=0).astype(bool))
            assert np.array_equal(R.smooth(m, k), R.smooth_scipy(m, k))
    assert np.array_equal(R.smooth(m, 1), m)


def test_reference_on_the_golden_planes():
    planes, slices, channels, ncomp, holes = golden_planes()
    assert planes.shape == (6, 750, 750)
    assert list(zip(slices.tolist(), channels.tolist())) == [(17, 2), (25, 0), (126, 0), (129, 3), (134, 3), (159, 3)]
    for i, p in enumerate(planes):
        assert R.table(p)[0] == ncomp[i]
        assert int(ndimage.binary_fill_holes(p).sum() - p.sum()) == holes[i]
        assert int(R.keep_largest(p, 3, 0, True).sum()) == int(p.sum()) + holes[i]      # at most four components, ties kept: only the fill changes
    v129 = planes[3]
    assert [r[0] for r in R.components(v129)] == [664, 478, 144, 144]
    assert R.keep_largest(v129, 3, 0, False).sum() == 1430                           # the 144 / 144 tie keeps four components
    assert [r[0] for r in R.components(planes[5])] == [485, 228, 228, 228]
    assert R.keep_largest(planes[5], 2, 0, False).sum() == 485 + 3 * 228
    noisy = v129 | salt(v129.shape, 129)
    assert R.table(noisy)[0] > 1000                                                  # specks: a thousand components against four real ones
    back = R.keep_largest(noisy, 3, 0, True).astype(bool)
    assert (back & v129).sum() == 1430 and back.sum() - 1430 <= 8                    # every original pixel returns; at most specks that touch a blob
