"""Host side of the raw-volume path (oct_segmentation_amd/pullback.py): the resample tables against Pillow itself -- applied by the numpy
restatement (tests/volume_ref.py), 0 differing bytes -- and against values worked out by hand from Resample.c's formulas, and the
properties of the normalisation restatement the GPU tests hold the kernel to."""
import numpy as np
import pytest
from PIL import Image

import volume_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd.pullback import pil_resample_table

# source (h, w) -> destination (h, w): both axes up, one axis skipped, up and down mixed, identity, tiny, a reduction to one pixel (129-tap
# and 97-tap windows cut by both borders)
SHAPES = [((13, 9), (7, 21)), ((40, 64), (40, 37)), ((33, 17), (100, 5)), ((5, 5), (5, 5)), ((1, 3), (4, 2)), ((64, 48), (1, 1))]


def checkerboard(h, w, c, cell=1):
    """0 / 255 squares: bicubic overshoot on both sides of the clamp."""
    yy, xx = np.mgrid[0:h, 0:w]
    a = ((((yy // cell) + (xx // cell)) & 1) * 255).astype(np.uint8)
    return np.repeat(a[:, :, None], c, axis=2) if c else a


def _pil(a, oh, ow):
    return np.array(Image.fromarray(a).resize((ow, oh)))


@pytest.mark.parametrize('src,dst', SHAPES)
def test_tables_reproduce_pillow(src, dst):
    (h, w), (oh, ow) = src, dst
    rng = np.random.default_rng(100 * h + w)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8), checkerboard(h, w, 3), checkerboard(h, w, 3, 2),
              rng.integers(0, 256, (h, w), dtype=np.uint8), checkerboard(h, w, 0)]             # the last two: mode L
    for k, a in enumerate(frames):
        got, want = R.pil_resize_ref(a, oh, ow), _pil(a, oh, ow)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert int((got != want).sum()) == 0, (src, dst, k)


def test_tables_reproduce_pillow_at_the_demo_size():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (750, 750, 3), dtype=np.uint8)
    a[100:300, 100:300] = checkerboard(200, 200, 3)
    assert int((R.pil_resize_ref(a, 1000, 1000) != _pil(a, 1000, 1000)).sum()) == 0


def test_the_clamp_is_live():
    """A checkerboard enlarged: some unclamped sums lie below 0 and some above 255."""
    a = checkerboard(12, 12, 0, 3).astype(np.int64)
    bounds, kk = pil_resample_table(12, 31)
    raw = np.array([((1 << 21) + (kk[i, :n].astype(np.int64)[:, None] * a[f:f + n]).sum(axis=0)) >> 22 for i, (f, n) in enumerate(bounds)])
    assert raw.min() < 0 and raw.max() > 255


def test_table_extents_by_hand():
    """filterscale = max(in / out, 1), support = 2 * filterscale, ksize = 2 * ceil(support) + 1; centre = (i + 0.5) * in / out;
    first = max(int(centre - support + 0.5), 0), last = min(int(centre + support + 0.5), in)."""
    # 750 -> 1000: scale 0.75, support 2, ksize 5.  i = 0: centre 0.375 -> int(-1.125) = -1 -> 0 .. int(2.875) = 2: (0, 2);
    # i = 999: centre 749.625 -> int(748.125) = 748 .. min(int(752.125), 750) = 750: (748, 2); i = 500: centre 375.375 -> 373 .. 377: (373, 4)
    bounds, kk = pil_resample_table(750, 1000)
    assert bounds.dtype == kk.dtype == np.int32 and bounds.shape == (1000, 2) and kk.shape == (1000, 5)
    assert tuple(bounds[0]) == (0, 2) and tuple(bounds[999]) == (748, 2) and tuple(bounds[500]) == (373, 4)
    # 1000 -> 250: scale 4, support 8, ksize 17.  i = 0: centre 2 -> int(-5.5) = -5 -> 0 .. int(10.5) = 10: (0, 10);
    # i = 249: centre 998 -> int(990.5) = 990 .. min(int(1006.5), 1000): (990, 10); i = 100: centre 402 -> 394 .. 410: (394, 16)
    bounds, kk = pil_resample_table(1000, 250)
    assert bounds.shape == (250, 2) and kk.shape == (250, 17)
    assert tuple(bounds[0]) == (0, 10) and tuple(bounds[249]) == (990, 10) and tuple(bounds[100]) == (394, 16)
    # coefficients sum to one (22 fractional bits, each rounded by itself) and are zero behind the count
    for tab_in, tab_out in ((750, 1000), (1000, 250), (5, 5), (64, 1)):
        bounds, kk = pil_resample_table(tab_in, tab_out)
        assert (np.abs(kk.sum(axis=1) - (1 << 22)) <= kk.shape[1]).all()
        for i, (f, n) in enumerate(bounds):
            assert f >= 0 and n >= 1 and f + n <= tab_in and not kk[i, n:].any()
    # the identity table of an interior pixel is the bicubic kernel at integer offsets: one tap of weight 1
    bounds, kk = pil_resample_table(5, 5)
    # (centre 2.5 -> int(1.0) = 1 .. int(5.0) = 5: offsets -1, 0, 1, 2 from the pixel)
    assert tuple(bounds[2]) == (1, 4) and list(kk[2]) == [0, 1 << 22, 0, 0, 0]
    with pytest.raises(ValueError):
        pil_resample_table(0, 4)


def test_normalize_ref_properties():
    rng = np.random.default_rng(9)
    h, w = 10, 9
    vol = np.empty((4, h, w, 3), np.uint16)
    vol[0] = 1234                                                   # constant: all zero
    vol[1] = rng.permutation(np.arange(h * w * 3) % 256).reshape(h, w, 3)     # spans 0..255 already: unchanged but for the channel order
    vol[2] = rng.integers(1000, 60000, (h, w, 3)); vol[2, 0, 0, 0] = 1000; vol[2, -1, -1, 2] = 60000
    vol[3] = rng.integers(7, 90, (h, w, 3)); vol[3, 1, 1, 1] = 7; vol[3, 2, 2, 0] = 89
    out = R.normalize_ref(vol)
    assert out.dtype == np.uint8 and out.shape == vol.shape
    assert not out[0].any()
    assert np.array_equal(out[1], vol[1, :, :, ::-1])
    assert np.array_equal(R.normalize_ref(vol, swap_rb=False)[1], vol[1])
    # slices are independent: each equals the result of normalising it alone, and each reaches both ends of the range
    for s in (2, 3):
        assert np.array_equal(out[s], R.normalize_ref(vol[s:s + 1])[0])
        assert out[s].min() == 0 and out[s].max() == 255
    assert out[2, 0, 0, 2] == 0 and out[2, -1, -1, 0] == 255       # reversed channels
    assert np.array_equal(R.slice_minmax(vol), [[1234, 1234], [0, 255], [1000, 60000], [7, 89]])
    # a grey volume: three equal channels, the same values as its colour form
    grey = R.normalize_ref(vol[..., 0])
    assert grey.shape == vol.shape and (grey[..., 0] == grey[..., 1]).all() and (grey[..., 0] == grey[..., 2]).all()
    # uint8 takes the same route
    assert np.array_equal(R.normalize_ref(vol[1].astype(np.uint8)[None]), out[1:2])


def test_symbols_declared():
    assert len(L.SYMBOLS['octseg_volume_normalize'][1]) == 10 and len(L.SYMBOLS['octseg_resize_pil_u8'][1]) == 16
