"""Host half of the rendering path (oct_segmentation_amd/postprocess.py) and the restatement the GPU tests compare against
(tests/postprocess_ref.py): constants against their definitions, the restatement against scipy's grey morphology and PIL's paste, and against
the reference's own published run (tests/golden/demo_overlay_crop.npz)."""
import os

import numpy as np
import pytest
from PIL import Image

import postprocess_ref as R
from oct_segmentation_amd import postprocess

HERE = os.path.dirname(os.path.abspath(__file__))
PIN = os.path.join(HERE, 'golden', 'demo_overlay_crop.npz')


def _blobs(rng, h, w, p=0.5, smooth=2):
    """Random blobs that touch every border: thresholded box-filtered noise."""
    a = rng.random((h + 2 * smooth, w + 2 * smooth))
    s = sum(a[i:i + h, j:j + w] for i in range(2 * smooth + 1) for j in range(2 * smooth + 1)) / (2 * smooth + 1) ** 2
    return s > np.quantile(s, 1 - p)


def test_host_constants():
    assert [int(r.sum()) for r in postprocess.ellipse(5)] == [1, 5, 5, 5, 1]
    assert [int(r.sum()) for r in postprocess.ellipse(7)] == [1, 5, 7, 7, 7, 5, 1]
    for n in (5, 7):
        e = postprocess.ellipse(n)
        assert e.dtype == np.uint8 and np.array_equal(e, e[::-1]) and np.array_equal(e, e[:, ::-1]) and np.array_equal(e != 0, R.footprint(n))
    t = postprocess.alpha_table()
    assert t.dtype == np.uint8 and t.shape == (257,)
    assert t[256] == 48 and t[0] == 0 and postprocess.RING_ALPHA == 231
    assert np.array_equal(t, (np.arange(257) / 256 * 64 * 0.85 * 255).astype(np.int64) & 255)
    assert np.array_equal(t, R.wrap_alpha(np.arange(257) / 256.0 * 64 * 0.85 * 255))
    assert postprocess.RING_ALPHA == int(R.wrap_alpha(1.0 * 255 * 0.85 * 255))
    assert postprocess.CLASS_COLORS_RGB == R.CLASS_COLORS_RGB


@pytest.mark.parametrize('n', [5, 7])
def test_restated_morphology_equals_scipy(n):
    ndi = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(n)
    for h, w in ((40, 52), (9, 7), (3, 30), (1, 1), (2, 5)):
        for p in (0.3, 0.7):
            if h * w < 36:
                m = rng.random((h, w)) < p
            else:
                m = _blobs(rng, h, w, p)
                m[0, w // 3] = m[-1, w // 2] = m[h // 2, 0] = m[h // 3, -1] = True
                assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
            f = m.astype(np.float64)
            assert np.array_equal(R.dilate(m, n), ndi.grey_dilation(f, footprint=R.footprint(n), mode='constant', cval=-np.inf) > 0)
            assert np.array_equal(R.erode(m, n), ndi.grey_erosion(f, footprint=R.footprint(n), mode='constant', cval=np.inf) > 0)


def test_closing_is_extensive_and_idempotent_and_blur_is_dyadic():
    rng = np.random.default_rng(2)
    for h, w in ((48, 60), (11, 5)):
        m = _blobs(rng, h, w, 0.4, smooth=1)
        for it in (1, 2, 3):
            c = R.close(m, it)
            assert np.all(c >= m) and np.array_equal(R.close(c, it), c)
        assert np.array_equal(R.close(np.ones((h, w), bool), 3), np.ones((h, w), bool))       # the border does not erode a full frame
        k = R.blur256(m)
        assert k.min() >= 0 and k.max() <= 256 and R.blur256(np.ones((h, w))).min() == 256
        # the same blur in float64 with explicit reflect-101 indices: exactly k / 256
        idx = lambda n: np.array([[(-q if q < 0 else (2 * n - 2 - q if q >= n else q)) for q in range(i - 2, i + 3)] for i in range(n)])
        g = np.array([1, 4, 6, 4, 1]) / 16.0
        f = m.astype(np.float64)
        hor = (f[:, idx(w)] * g).sum(axis=2)
        ver = (hor[idx(h), :] * g[None, :, None]).sum(axis=1)
        assert np.array_equal(ver, k / 256.0)


def test_integer_paste_equals_pil():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    a = rng.integers(0, 256, (64, 96), dtype=np.uint8)
    a[:4] = np.array([0, 255, 48, 231], np.uint8)[:, None]
    for col in R.CLASS_COLORS_RGB.values():
        pil = Image.fromarray(img)
        pil.paste(Image.new('RGB', pil.size, col), (0, 0), Image.fromarray(a))
        want = np.stack([R.paste_int(img[:, :, c], col[c], a) for c in range(3)], axis=2)
        assert np.array_equal(np.asarray(pil), want)


def test_restatement_equals_the_reference_run():
    """Reference pin.  Re-rendering the authors' frame from the authors' colour mask gives the authors' overlay, bit for bit, on every pixel
    far enough from an anti-aliased mask pixel: that holds PIL's resize of the frame, the paste formula, the interior alpha 48 of the uint8
    wrap and the class order.  (Edges are not pinned: the masks of that run were not binary there.)"""
    frame, masks, overlay, compared = R.load_pin(PIN)
    n_cmp, n_changed = R.check_pin_coverage(frame, overlay, compared)
    print('compared', n_cmp, 'of', compared.size, '; changed by the overlay', n_changed)
    for it in (1, 3):
        got, cm = R.render(Image.fromarray(frame), masks, R.ALL_CLASSES, it)
        assert np.array_equal(got[compared], overlay[compared])
        assert np.array_equal(cm[compared], np.load(PIN)['mask'][compared])


def test_render_wrappers_refuse_host_tensors():
    import torch
    with pytest.raises(ValueError):
        postprocess.render_results(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), torch.zeros((1, 8, 8, 4)), ['Lumen'])
    with pytest.raises(ValueError):
        postprocess.save_results([Image.new('RGB', (8, 8))], [np.full((8, 8, 4), 0.5)], ['a'], ['Lumen'], '/nonexistent')
