"""The lumen geometry on the host: tests/shape_ref.py (the pin of csrc/shape.hip) against scipy, the offset table, discs and an ellipse with known
diameters, the arithmetic of the lumen report on hand-made areas, the int64 bound and the host refusals.  No GPU."""
import json
import math
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import shape_ref as S
from oct_segmentation_amd import shape
from oct_segmentation_amd.model import CLASS_IDS

IN, OUT, LAST, HITS, RUNS = range(5)
H, W = 97, 130


def _blobs(rng, h, w, p, smooth):
    a = rng.random((h + 2 * smooth, w + 2 * smooth))
    s = sum(a[i:i + h, j:j + w] for i in range(2 * smooth + 1) for j in range(2 * smooth + 1))
    return s > np.quantile(s, 1 - p)


def _ellipse(h, w, cx, cy, a, b):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1.0


def test_restatement_agrees_with_scipy():
    rng = np.random.default_rng(11)
    for h, w, p in ((17, 33, 0.4), (64, 48, 0.2), (97, 130, 0.6)):
        masks = np.stack([_blobs(rng, h, w, p, 1 + k) for k in range(3)], axis=-1)[None].astype(np.float32)
        mom = S.moments(masks)
        yy, xx = np.mgrid[0:h, 0:w]
        for k in range(3):
            plane = masks[0, :, :, k] != 0
            m = mom[0, k]
            for field, img in ((0, np.ones_like(xx)), (1, xx), (2, yy), (3, xx * xx), (4, xx * yy), (5, yy * yy)):
                assert m[field] == int(ndimage.sum_labels(img.astype(np.float64), plane, 1)), (h, w, k, field)
            cy, cx = ndimage.center_of_mass(plane)
            assert abs(m[1] / m[0] - cx) < 1e-9 and abs(m[2] / m[0] - cy) < 1e-9
            ys, xs = ndimage.find_objects(plane.astype(np.int32))[0]
            assert tuple(m[6:10]) == (xs.start, xs.stop - 1, ys.start, ys.stop - 1)
            # every boundary pixel (set, not in the 4-connected erosion with a clear border) counted once per clear or outside neighbour
            rim = plane & ~ndimage.binary_erosion(plane, ndimage.generate_binary_structure(2, 1), border_value=0)
            pad = np.pad(plane, 1)
            clear_nb = sum((~pad[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]).astype(np.int64) for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)))
            assert m[10] == int(clear_nb[rim].sum()) and not clear_nb[plane & ~rim].any() and m[11] == 0
    empty = S.moments(np.zeros((1, 5, 4, 1), np.float32))[0, 0]
    assert tuple(empty) == (0, 0, 0, 0, 0, 0, 4, -1, 5, -1, 0, 0)
    full = S.moments(np.ones((1, 130, 97, 1), np.float32))[0, 0]
    assert full[10] == 2 * (130 + 97) and full[0] == 130 * 97


def test_ray_offsets_values_and_width():
    for h, w in ((1, 1), (5, 4), (97, 130), (40, 300)):
        off = shape.ray_offsets(h, w)
        R = int(math.hypot(h, w))
        assert off.dtype == np.int32 and off.shape == (360, R, 2)
        r = np.arange(1, R + 1)
        zero = np.zeros_like(r)
        assert (off[0] == np.stack([r, zero], 1)).all() and (off[90] == np.stack([zero, r], 1)).all()
        assert (off[180] == np.stack([-r, zero], 1)).all() and (off[270] == np.stack([zero, -r], 1)).all()
        d = np.floor(r * math.cos(math.radians(45)) + 0.5).astype(np.int64)
        assert (off[45, :, 0] == d).all() and (np.abs(off[45, :, 1] - d) <= 1).all()
        assert (off == S.offsets(h, w)).all()                   # numpy's element-wise doubles are CPython's
    assert list(shape.ray_offsets(97, 130)[45, :4, 0]) == [1, 1, 2, 3]
    with pytest.raises(ValueError):
        shape.ray_offsets(0, 4)


def _report(masks, ratio=1, **kw):
    """The report of the restatement's integers for channel 0 through the package's host arithmetic."""
    n, h, w, _ = masks.shape
    mom = S.moments(masks)
    org = S.origins(masks, mom)
    prof, length = S.polar_at(masks, org, shape.ray_offsets(h, w))
    return shape.build_lumen_report(mom[:, 0], org[:, 0], prof[:, 0], length[:, 0], h, w, ratio=ratio, **kw), mom, org, prof, length


def test_discs_and_an_ellipse_have_their_diameters():
    masks = np.zeros((3, H, W, 1), np.float32)
    masks[0, :, :, 0] = _ellipse(H, W, 70, 40, 30, 30)
    masks[1, :, :, 0] = _ellipse(H, W, 60, 50, 40, 20)
    masks[2, :, :, 0] = _ellipse(H, W, 30, 60, 9, 9)
    rep, mom, org, prof, length = _report(masks)
    lum = rep['lumen']
    assert lum['slice'] == [0, 1, 2] and lum['inside'] == [1, 1, 1] and lum['cut'] == [False, False, False]
    assert tuple(org[0, 0]) == (70, 40, 1) and tuple(org[1, 0]) == (60, 50, 1) and tuple(org[2, 0]) == (30, 60, 1)
    for i, radius in ((0, 30), (2, 9)):
        e = np.where(prof[i, 0, :, IN] == 1, prof[i, 0, :, OUT], 0)
        d = e[:180] + e[180:] + 1
        assert (np.abs(d - (2 * radius + 1)) <= 2).all(), (i, d.min(), d.max())
        assert lum['d_min'][i] == d.min() and lum['d_max'][i] == d.max()
    e = np.where(prof[0, 0, :, IN] == 1, prof[0, 0, :, OUT], 0)
    assert 59 <= (e[:180] + e[180:] + 1).min() and (e[:180] + e[180:] + 1).max() <= 61
    assert (lum['d_min'][1], lum['d_max'][1]) == (39.0, 81.0) and 60 <= lum['d_argmin'][1] <= 90   # the first degree of the flat minimum around 90
    assert abs(lum['eccentricity'][1] - 42 / 81) < 1e-12 and lum['eccentricity'][0] <= 2 / 61
    t = shape.shape_table(mom)
    assert round(float(t['minor'][1, 0]), 2) == 39.88 and round(float(t['major'][1, 0]), 2) == 80.12
    assert abs(t['major'][1, 0] - 80) <= 0.8 and abs(t['minor'][1, 0] - 40) <= 0.4          # within 1 % of 2a, 2b
    assert abs(t['major'][0, 0] - 60) <= 0.6 and abs(t['minor'][0, 0] - 60) <= 0.6 and abs(t['orientation'][1, 0]) < 1e-9
    assert (t['cx'][1, 0], t['cy'][1, 0]) == (60.0, 50.0) and t['area'][1, 0] == mom[1, 0, 0] and t['perimeter'][1, 0] == mom[1, 0, 10]
    assert (t['xmin'][1, 0], t['xmax'][1, 0], t['ymin'][1, 0], t['ymax'][1, 0]) == (20, 100, 30, 70)
    assert 0.5 < t['compactness'][0, 0] < 0.8                   # a digital disc's crack perimeter is its bounding square's: pi / 4 in the limit
    ct = shape.centroid_thickness(prof[0, 0])
    assert ct['min'] >= 29 and ct['max'] <= 30 and len(ct['all_measurements']) == 360
    assert shape.centroid_thickness(np.zeros((360, 5), np.int32)) == {'median': 0, 'min': 0, 'max': 0, 'all_measurements': []}
    assert 'NOT' in shape.centroid_thickness.__doc__ and 'calculate_thickness_contour' in shape.centroid_thickness.__doc__


def _areas_report(areas, h=20, w=20, **kw):
    """Slices whose lumen is a row-major run of `areas[i]` pixels: only the areas matter."""
    masks = np.zeros((len(areas), h, w, 1), np.float32)
    for i, a in enumerate(areas):
        masks[i].reshape(-1)[:a] = 1
    return _report(masks, **kw)[0]


def test_lumen_report_arithmetic():
    rep = _areas_report([50, 30, 60, 30, 40], ratio=2)
    assert rep['mla'] == {'slice': 1, 'area_px': 30, 'area': 7.5}                      # the first on ties
    assert rep['reference']['proximal']['slice'] == 0 and rep['reference']['distal']['slice'] == 2
    assert rep['reference']['area_px'] == 55.0 and rep['area_stenosis'] == 100.0 * (1 - 30 / 55)
    assert rep['lumen']['area'] == [12.5, 7.5, 15.0, 7.5, 10.0] and rep['ratio'] == 2 and rep['images'] == ['0', '1', '2', '3', '4']
    assert json.loads(json.dumps(rep)) == rep
    one = _areas_report([20, 50, 60])                                                   # MLA first: only a distal side
    assert one['mla']['slice'] == 0 and one['reference']['proximal'] is None and one['reference']['distal']['slice'] == 2
    assert one['reference']['area_px'] == 60.0 and one['area_stenosis'] == 100.0 * (1 - 20 / 60)
    win = _areas_report([90, 50, 40, 20, 45, 80, 95], ref_window=2)
    assert win['mla']['slice'] == 3 and win['reference']['proximal']['slice'] == 1 and win['reference']['distal']['slice'] == 5
    assert win['reference']['area_px'] == 65.0
    assert _areas_report([90, 50, 40, 20, 45, 80, 95])['reference']['area_px'] == 92.5
    none = _areas_report([0, 400, 0])                                                   # empty and completely full masks are absent
    assert none['lumen']['slice'] == [] and none['mla'] is None and none['reference'] is None and none['area_stenosis'] is None
    alone = _areas_report([0, 30, 400])
    assert alone['lumen']['slice'] == [1] and alone['reference']['area_px'] == 30.0 and alone['area_stenosis'] == 0.0
    assert json.loads(json.dumps(none)) == none
    # a ring: the centroid is in the hole, there is no diameter through it
    masks = np.zeros((1, 41, 41, 1), np.float32)
    masks[0, :, :, 0] = _ellipse(41, 41, 20, 20, 15, 15) & ~_ellipse(41, 41, 20, 20, 8, 8)
    ring, mom, org, prof, length = _report(masks)
    assert tuple(org[0, 0]) == (20, 20, 0) and ring['lumen']['inside'] == [0]
    for k in ('d_min', 'd_max', 'd_mean', 'd_argmin', 'eccentricity'):
        assert ring['lumen'][k] == [None]
    assert ring['lumen']['d_equivalent'][0] == 2 * math.sqrt(int(mom[0, 0, 0]) / math.pi) and json.loads(json.dumps(ring)) == ring
    # the package's arithmetic equals the restatement's
    masks = np.zeros((4, H, W, 1), np.float32)
    for i, (a, b) in enumerate(((30, 20), (12, 9), (45, 50), (20, 20))):
        masks[i, :, :, 0] = _ellipse(H, W, 50 + 5 * i, 45, a, b)
    got, mom, org, prof, length = _report(masks, ratio=14, ref_window=1)
    assert got == S.lumen_report(mom[:, 0], org[:, 0], prof[:, 0], length[:, 0], H, W, range(4), 14, ref_window=1)
    assert got['lumen']['cut'] == [False, False, True, False] and got['mla']['slice'] == 1


def test_int64_bound_from_the_exported_constants():
    assert shape.MAX_EXTENT == 32768 and shape.MAX_PIXELS == 2 ** 31 and shape.MOMENT_FIELDS == 12
    assert shape.MAX_EXTENT ** 2 * shape.MAX_EXTENT ** 2 < 2 ** 63
    assert (shape.MAX_PIXELS - 1) * (shape.MAX_EXTENT - 1) ** 2 < 2 ** 61
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'octseg.h')) as f:
        header = f.read()
    assert f'#define OCTSEG_SHAPE_MAX_EXTENT {shape.MAX_EXTENT}' in header and f'#define OCTSEG_MOMENT_FIELDS {shape.MOMENT_FIELDS}' in header
    from oct_segmentation_amd import _lib as L
    for name in ('octseg_stack_moments', 'octseg_moment_origins', 'octseg_stack_polar_at'):
        assert f'int {name}(const float* stack, ' in header and name in L.SYMBOLS and hasattr(L.lib(), name)


def test_host_refusals():
    ok = torch.zeros((1, 8, 8, 4), dtype=torch.float32)
    for fn in (shape.moments_stack, shape.centred_profile, shape.lumen_report):
        with pytest.raises(ValueError, match='host'):
            fn(ok)                                              # a CPU tensor
        with pytest.raises(ValueError, match='float32'):
            fn(ok.to(torch.float64))
        with pytest.raises(ValueError, match='float32'):
            fn(ok.numpy())
        with pytest.raises(ValueError, match='empty'):
            fn(torch.zeros((0, 8, 8, 4)))
    with pytest.raises(ValueError, match='at most 16'):
        shape.moments_stack(torch.zeros((1, 4, 4, 17)))
    with pytest.raises(ValueError, match='at most 8'):
        shape.centred_profile(torch.zeros((1, 4, 4, 9)))
    with pytest.raises(ValueError, match='at most 8'):
        shape.lumen_report(torch.zeros((1, 4, 4, 9)))
    with pytest.raises(ValueError, match='host'):
        shape.origins(ok, torch.zeros((1, 4, 12), dtype=torch.int64))
    meta = torch.zeros((1, 8, 8, 4), dtype=torch.float32, device='meta')          # is_cuda is False: refused like a host tensor
    with pytest.raises(ValueError):
        shape.moments_stack(meta)
    z = np.zeros((1, 12), np.int64)
    args = (z, np.zeros((1, 3), np.int32), np.zeros((1, 360, 5), np.int32), np.zeros((1, 360), np.int32))
    with pytest.raises(ValueError, match='ratio'):
        shape.build_lumen_report(*args, 5, 5)                   # int(5 * 150 // 1000) == 0
    with pytest.raises(ValueError, match='ratio'):
        shape.build_lumen_report(*args, 50, 50, ratio=0)
    with pytest.raises(ValueError, match='ref_window'):
        shape.build_lumen_report(*args, 50, 50, ref_window=0)
    with pytest.raises(ValueError, match='names'):
        shape.build_lumen_report(*args, 50, 50, image_names=['a', 'b'])
    with pytest.raises(ValueError, match='unknown class'):
        shape.lumen_report(ok, lumen='Thrombus')
    with pytest.raises(ValueError, match='unknown class'):
        shape._channel('Thrombus', 4)
    with pytest.raises(ValueError, match='channel'):
        shape._channel(CLASS_IDS['Lumen'] - 1 + 4, 4)
    assert shape._channel(None, 4) == -1 and shape._channel('Lumen', 4) == CLASS_IDS['Lumen'] - 1 and shape._channel(2, 4) == 2
    with pytest.raises(ValueError, match='mom'):
        shape.shape_table(np.zeros((2, 12)))
