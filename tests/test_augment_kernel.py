"""The float64 restatement of augment_kernel (tests/augment_kernel_ref.py) must not be a transliteration of the kernel: it is anchored here, on
the CPU, to things that exist without it --

  * torch indexing (flip, slices, transpose, index_select) on the Rule X cases: bit for bit, nothing two-valued;
  * oracle/augment_ref.py: its warp on frames with ONE resampling stage, its brightness / contrast LUT, its 8-bit HSV round trip, its noise stage fed
    the restated field -- each must be among the restatement's candidates;
  * the statistics of the restated noise field (the GPU has to reproduce it candidate for candidate, so this is the check on the generator);
  * its own caps: the share of two-valued and open pixels of every family, which test_gpu_augment.py asserts again on the GPU.
"""
import numpy as np
import pytest

import augment_cases as AC
import augment_kernel_ref as KR


def _hwc_u8(t):
    return np.ascontiguousarray(np.moveaxis(np.asarray(t), 0, -1)).astype(np.uint8)


def _among(got_chw, res, n, what):
    """got (numpy [K, H, W]) is one of frame n's image candidates wherever the pixel is not open."""
    g = got_chw.astype(np.float32)
    bad = (g != res.img_a[n]) & (g != res.img_b[n]) & ~res.img_open[n][None]
    assert not bad.any(), f'{what}: {int(bad.sum())} elements are none of the candidates; first {tuple(int(t[0]) for t in np.nonzero(bad))}'


@pytest.mark.parametrize('family', ['exact', 'stride'])
def test_restatement_equals_torch_indexing(family):
    for case in AC.FAMILIES[family]():
        res = case.ref()
        ei, em = case.expect
        assert np.array_equal(res.img_a, ei.numpy()) and np.array_equal(res.img_b, ei.numpy()), case.id
        assert np.array_equal(res.mask_a, em.numpy()) and np.array_equal(res.mask_b, em.numpy()), case.id
        assert not res.img_open.any() and not res.mask_open.any(), case.id
        assert res.report['img_two_pixels'] == 0 and res.report['mask_two_pixels'] == 0, (case.id, res.report)
    if family == 'stride':
        B, _, H, W = case.img.shape
        assert B * H * W > 16384 * 256          # the launch's grid cap: the loop runs a second trip


def test_exact_cases_cover_what_they_claim():
    cases = AC.FAMILIES['exact']()
    names = ' '.join(c.id for c in cases)
    for key in ('identity', 'hflip', 'vflip', 'shift', 'shift_out', 'shift_far', 'transpose', 'magnify', 'magnify_w2', 'crop', 'crop_one', 'crop_empty',
                'crop_flip'):
        assert key in names, key
    assert {tuple(c.img.shape[2:]) for c in cases} == {(1, 1), (1, 70), (7, 5), (48, 80), (80, 48)}
    assert {c.mask.shape[1] for c in cases} == {1, 4, 5}
    for c in cases:
        assert c.img.shape[0] == 3 and len({r.tobytes() for r in c.params}) == 3, c.id      # a different row per frame
    assert any(bool(c.expect[0].any()) for c in cases if 'magnify' in c.id)
    assert np.isfinite(np.concatenate([c.params[:, :12].ravel() for c in cases])).all()


@pytest.mark.parametrize('kind', ['ssr', 'crop+perspective'])
def test_single_resampling_stage_against_the_oracle_warp(kind):
    """Frames whose chain resamples once: the oracle's sequential chain and the kernel's composed homography describe the same gather, and
    both round float64 bilinear values to nearest-even.  Masks agree outside the two-valued set; the oracle's image is one of the candidates.
    One difference is by design and excluded: after crop + pad the oracle interpolates between the window's rim and the PADDING, the kernel
    between the rim and the source pixels beyond it (it blanks by the window test alone), so image pixels whose bilinear cell reaches across a
    window edge (cx or cy within one pixel of it) are compared through the mask only.  That is the statistical, not bit, parity DESIGN states."""
    from oracle.augment_ref import apply_chain
    S, N = 64, 12
    keep = (lambda l: 'ssr' in l and 'crop' not in l and 'perspective' not in l) if kind == 'ssr' else \
        (lambda l: 'crop' in l and 'perspective' in l and 'ssr' not in l)
    rows, logs = AC._sampled(S, N, 5 if kind == 'ssr' else 6, keep)
    assert any('hflip' in l for l in logs) and any('hflip' not in l for l in logs)
    img, mask = AC._smooth(N, 2, S, S, seed=9)
    res = KR.augment_ref(rows, img.numpy(), mask.numpy())
    compared = 0
    for n in range(N):
        oi, om = apply_chain(_hwc_u8(img[n]), _hwc_u8(mask[n]), logs[n], S)
        oi, om = np.moveaxis(oi, -1, 0).astype(np.float32), np.moveaxis(om, -1, 0).astype(np.float32)
        settled = ~res.mask_open[n][None] & (res.mask_a[n] == res.mask_b[n])
        assert np.array_equal(om[settled], res.mask_a[n][settled]), (n, logs[n])
        ok = (oi == res.img_a[n]) | (oi == res.img_b[n]) | res.img_open[n][None]
        if kind != 'ssr':
            ok |= _window_rim(rows[n], S)[None]
        compared += int(ok.size - (0 if kind == 'ssr' else 3 * _window_rim(rows[n], S).sum()))
        assert ok.all(), (n, logs[n], int((~ok).sum()))
    assert compared > 0.85 * N * 3 * S * S
    assert res.uncertain_img() <= 0.01 and res.uncertain_mask() <= 0.001


def _window_rim(r, S):
    p = r.astype(np.float64)
    ys, xs = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing='ij')
    w = p[26] * xs + p[27] * ys + p[28]
    cx, cy = (p[20] * xs + p[21] * ys + p[22]) / w, (p[23] * xs + p[24] * ys + p[25]) / w
    near = lambda c, e: np.abs(c - (e - 0.5)) <= 1.0 + 1e-6      # noqa: E731
    return near(cx, p[29]) | near(cx, p[31]) | near(cy, p[30]) | near(cy, p[32])


def test_oracle_brightness_contrast_is_a_candidate():
    from oracle.augment_ref import brightness_contrast_uint8
    (case,) = AC.FAMILIES['bc']()
    res = case.ref()
    for n in range(case.img.shape[0]):
        want = brightness_contrast_uint8(_hwc_u8(case.img[n]), float(case.params[n, 9]), float(case.params[n, 10]))
        _among(np.moveaxis(want, -1, 0), res, n, f'bc frame {n}')
    skip = res.img_a[-1]
    assert np.array_equal(skip, case.img[-1].numpy())            # (1, 0): the stage is skipped


def test_oracle_hsv_is_a_candidate():
    from oracle.augment_ref import shift_hsv_uint8
    for case in AC.FAMILIES['hsv']():
        res = case.ref()
        for n in range(case.img.shape[0]):
            h, s, v = (float(case.params[n, k]) for k in (13, 14, 15))
            want = shift_hsv_uint8(_hwc_u8(case.img[n]), h, s, v)
            _among(np.moveaxis(want, -1, 0), res, n, f'{case.id} frame {n}')
    # a true tie of the backward conversion is reported as two-valued: (255, 254, 254) is h = 0, s = 1, v = 255; shifted to h = 15 the second
    # channel is 255 (1 - 1/255 * 1/2) = 254.5 on paper
    r = KR.augment_ref(AC.row(hue=15.0, hsv_on=True)[None], np.array([255.0, 254.0, 254.0], np.float32).reshape(1, 3, 1, 1), np.zeros((1, 1, 1, 1), np.float32))
    assert (r.img_a.ravel().tolist(), r.img_b.ravel().tolist()) == ([255.0, 254.0, 254.0], [255.0, 255.0, 254.0])


def test_oracle_noise_stage_fed_the_restated_field_is_a_candidate():
    from oracle.augment_ref import gauss_noise_uint8
    (case,) = AC.FAMILIES['noise']()
    res = case.ref()
    for n in range(case.img.shape[0]):
        want = gauss_noise_uint8(_hwc_u8(case.img[n]), np.moveaxis(res.noise[n], 0, -1))
        _among(np.moveaxis(want, -1, 0), res, n, f'noise frame {n}')
    assert (res.img_a == 0).any() and (res.img_b == 255).any()                    # both clamps are hit
    assert res.noise_yard.min() > 0
    # frames 4 and 5 share seed and sigma: the hash takes the flat index, so their fields differ
    assert case.params[4].tobytes() == case.params[5].tobytes()
    assert not np.array_equal(res.noise[4], res.noise[5])
    assert abs(np.corrcoef(res.noise[4].ravel(), res.noise[5].ravel())[0, 1]) < 4 / np.sqrt(res.noise[4].size)


def test_restated_generator_bits():
    """hash3 / u01 against a scalar evaluation in Python integers, and u01's rounding addition."""
    def h3(a, b, c):
        m = 0xFFFFFFFF
        x = ((a * 0x9E3779B1) & m) ^ ((((b + 0x7F4A7C15) & m) * 0x85EBCA77) & m) ^ ((((c + 0x165667B1) & m) * 0xC2B2AE3D) & m)
        x ^= x >> 16; x = (x * 0x7FEB352D) & m; x ^= x >> 15; x = (x * 0x846CA68B) & m; x ^= x >> 16
        return x
    for a, b, c in ((0, 0, 0), (1, 2, 3), (0xFFFFFFFF, 0xFFFFFFFF, 5), (2 ** 31 - 2, 4095, 1)):
        assert int(KR.hash3(a, b, c)) == h3(a, b, c)
    u = KR.u01(np.array([0, 0xFFFFFFFF, 0x80000100, 0x800001FF], dtype=np.uint64))
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -25) and u[1] == np.float32(1.0)             # 16777215.5 rounds to even: 2^24
    assert u[2] == np.float32((2 ** 23 + 2) / 2 ** 24) and u[3] == np.float32((2 ** 23 + 2) / 2 ** 24)   # 8388609.5 -> 8388610 (ties to even)
    assert float(KR.TWO_PI_F32) != 2 * np.pi


def test_restated_noise_field_quality():
    """3 x 256 x 256 samples per frame, two frames, sigma = 2, no clamping: moments within 4 standard errors, correlations (channels, x and y
    neighbours, frames) within 4 / sqrt(n), Kolmogorov-Smirnov distance against N(0, sigma^2) below the 0.1 % critical value."""
    from scipy import stats
    S, sigma = 256, 2.0
    idx = np.arange(2 * S * S, dtype=np.uint64).reshape(2, S, S)
    f = KR.noise_field(np.uint32(20240), sigma, idx)              # [3, 2, S, S]
    n = f.size
    assert abs(f.mean()) <= 4 * sigma / np.sqrt(n)
    assert abs(f.std() - sigma) <= 4 * sigma / np.sqrt(2 * n)
    corr = lambda a, b: np.corrcoef(a.ravel(), b.ravel())[0, 1]   # noqa: E731
    for a, b, what in ((f[0], f[1], 'c0 c1'), (f[0], f[2], 'c0 c2'), (f[1], f[2], 'c1 c2'), (f[..., :-1], f[..., 1:], 'x'), (f[..., :-1, :], f[..., 1:, :], 'y'),
                       (f[:, 0], f[:, 1], 'frames')):
        assert abs(corr(a, b)) <= 4 / np.sqrt(a.size), (what, corr(a, b))
    d = stats.kstest(f.ravel(), 'norm', args=(0.0, sigma)).statistic
    assert d < 1.94947 / np.sqrt(n), d                            # c(0.001) = sqrt(-ln(0.0005) / 2)
    # another seed gives another field
    assert abs(corr(f, KR.noise_field(np.uint32(20241), sigma, idx))) <= 4 / np.sqrt(n)


@pytest.mark.parametrize('family', sorted(AC.FAMILIES))
def test_caps_hold_for_the_restatement_alone(family):
    for case in AC.FAMILIES[family]():
        res = case.ref()
        sh = res.shares()
        print(f'SHARES {case.id}: ' + ' '.join(f'{k} {100 * v:.4f}%' for k, v in sh.items()), {k: v for k, v in res.report.items() if 'pixels' not in k})
        assert res.uncertain_img(case.unit) <= case.cap_img, (case.id, sh, res.report)
        assert res.uncertain_mask() <= case.cap_mask, (case.id, sh, res.report)
        assert (res.img_a <= res.img_b).all() and (res.mask_a <= res.mask_b).all()
        assert res.img_a.min() >= 0 and res.img_b.max() <= 255 and np.array_equal(res.img_a, np.rint(res.img_a))


def test_chain_holds_every_decision_and_sampled_cases_are_what_they_say():
    (case,) = AC.FAMILIES['chain']()
    for k in AC.DECISIONS:
        assert any(k in l for l in case.logs), k
    for case in AC.FAMILIES['warp']():
        assert all('ssr' in l or 'perspective' in l for l in case.logs) and len(case.logs) == 24
        assert (case.params[:, 9] == 1).all() and (case.params[:, 10:12] == 0).all() and (case.params[:, 16] == 0).all()
    for case in AC.FAMILIES['cropwarp']():
        assert all('crop' in l and 'perspective' in l and 'ssr' not in l for l in case.logs)
    assert sum(c.img.shape[0] for c in AC.FAMILIES['cropwarp']()) == 16
    assert {tuple(c.img.shape[2:]) for c in AC.FAMILIES['warp']()} == {(64, 64), (48, 80)}
