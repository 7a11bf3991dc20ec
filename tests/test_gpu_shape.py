"""csrc/shape.hip on the GPU against the numpy restatement (tests/shape_ref.py): exact integer equality everywhere -- moments, box and crack
perimeter, the centroid pixel, and the polar profile walked from it -- plus the profile's invariants, the ABI's refusals, the demo excerpt and
the predict CLI's lumen=true."""
import functools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import analysis_ref as R
import shape_ref as S
from oct_segmentation_amd import polar, shape
from oct_segmentation_amd.model import CLASS_IDS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'pullback_demo_excerpt.npz')
IN, OUT, LAST, HITS, RUNS = range(5)
SHAPES = [(1, 1), (2, 3), (5, 4), (17, 33), (64, 48), (97, 130), (130, 97)]


@functools.lru_cache(maxsize=None)
def _offsets(h, w):
    return S.offsets(h, w)


def _blobs(rng, h, w, p, smooth):
    if h * w < 36:
        return rng.random((h, w)) < p
    a = rng.random((h + 2 * smooth, w + 2 * smooth))
    s = sum(a[i:i + h, j:j + w] for i in range(2 * smooth + 1) for j in range(2 * smooth + 1))
    return s > np.quantile(s, 1 - p)


def _masks(n, h, w, channels):
    """Random blobs, the same for every test of a shape; set values drawn from {1, 255, -2.5, 1e-30}: any value != 0 is set."""
    rng = np.random.default_rng(7000 * h + 10 * w + n)
    ps = (0.15, 0.4, 0.7, 0.3, 0.55, 0.05, 0.9, 0.25, 0.6, 0.1, 0.35, 0.8, 0.45, 0.2, 0.65, 0.5)
    m = np.stack([np.stack([_blobs(rng, h, w, ps[c], 1 + (c & 1)) for c in range(channels)], axis=-1) for _ in range(n)]).astype(np.float32)
    m[m != 0] = rng.choice(np.array([1.0, 255.0, -2.5, 1e-30], np.float32), size=int((m != 0).sum()))
    return m


def _diff(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError((what, len(bad), bad[:5].tolist(), got[got != want][:5].tolist(), want[got != want][:5].tolist()))


def _dev(cuda, masks):
    return torch.from_numpy(np.ascontiguousarray(masks, np.float32)).to(cuda)


def _unaligned(cuda, m4):
    """A 4-channel view that starts 4 bytes into its storage: the dword path."""
    m4 = np.ascontiguousarray(m4)
    buf = torch.zeros(m4.size + 8, dtype=torch.float32, device=cuda)
    buf[1:1 + m4.size] = torch.from_numpy(m4).to(cuda).flatten()
    view = buf[1:1 + m4.size].view(*m4.shape)
    assert view.data_ptr() % 16 == 4
    return view


def _moments(stack):
    mom = shape.moments_stack(stack)
    assert mom.dtype == torch.int64 and tuple(mom.shape) == (stack.shape[0], stack.shape[3], 12)
    return mom.cpu().numpy()


@pytest.mark.parametrize('h,w', SHAPES)
@pytest.mark.parametrize('n', [1, 3])
def test_moments_equal_restatement(cuda, n, h, w):
    """One reference per shape over sixteen channels, its channels reused for the 1-, 4-, 5-, 8- and 16-channel stacks (dword path, 16-byte path,
    passes of four channels with a partial last one) and for the unaligned 4-channel view."""
    masks = _masks(n, h, w, 16)
    want = S.moments(masks)
    for sc in (1, 4, 5, 8, 16):
        _diff(_moments(_dev(cuda, masks[..., :sc])), want[:, :sc], (n, h, w, sc))
    _diff(_moments(_unaligned(cuda, masks[..., :4])), want[:, :4], (n, h, w, 'unaligned'))


def test_moments_designed_frames(cuda):
    # 3 x 5000: a workgroup's 16384-pixel tile and the waves' 4096-pixel runs end inside rows; x^2 is large
    rng = np.random.default_rng(3)
    m = (rng.random((2, 3, 5000, 4)) < np.array([0.5, 0.02, 0.98, 1.0])).astype(np.float32)
    m[1, :, :, 0] = 0
    m[1, 1, 4095:4098, 0] = 1                                   # a run across the first wave seam of row 1 ...
    m[1, 0, 4999, 0] = m[1, 1, 0, 0] = 1                        # ... and the end of one row and the start of the next: not neighbours
    want = S.moments(m)
    _diff(_moments(_dev(cuda, m)), want, '3 x 5000')
    _diff(_moments(_dev(cuda, m[..., :3])), want[:, :3], '3 x 5000, three channels')
    assert want[0, 3, 10] == 2 * (3 + 5000) and want[1, 0, 10] == 4 * 5 - 2 * 2
    # all set, 130 x 97: the largest sums of the shape, EDGES is the frame's perimeter
    full = np.ones((1, 130, 97, 5), np.float32)
    got = _moments(_dev(cuda, full))
    _diff(got, S.moments(full), 'full')
    assert (got[0, :, 10] == 2 * (130 + 97)).all() and (got[0, :, 0] == 130 * 97).all()
    assert tuple(got[0, 0, 6:10]) == (0, 96, 0, 129) and got[0, 0, 3] == 130 * sum(x * x for x in range(97))
    # empty planes keep the initial box; single pixels in each corner
    h, w = 33, 70
    c = np.zeros((6, h, w, 4), np.float32)
    for i, (y, x) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))):
        c[i, y, x, i] = 1
    c[4, 0, 0, 1] = c[4, 0, w - 1, 1] = c[4, h - 1, 0, 1] = c[4, h - 1, w - 1, 1] = 1
    got = _moments(_dev(cuda, c))
    _diff(got, S.moments(c), 'corners')
    assert tuple(got[5, 2]) == (0, 0, 0, 0, 0, 0, w, -1, h, -1, 0, 0) and tuple(got[0, 1]) == tuple(got[5, 2])
    assert tuple(got[3, 3]) == (1, w - 1, h - 1, (w - 1) ** 2, (w - 1) * (h - 1), (h - 1) ** 2, w - 1, w - 1, h - 1, h - 1, 4, 0)
    assert tuple(got[4, 1, 6:11]) == (0, w - 1, 0, h - 1, 16)


def test_moment_origins(cuda):
    h, w = 41, 52
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((3, h, w, 4), np.float32)
    m[0, :, :, 0] = (xx - 40) ** 2 + (yy - 12) ** 2 <= 64                                  # a disc: AT = 1
    m[0, :, :, 1] = ((xx - 20) ** 2 + (yy - 20) ** 2 <= 15 ** 2) & ((xx - 20) ** 2 + (yy - 20) ** 2 >= 8 ** 2)   # a ring: AT = 0
    m[0, 5, 0, 2] = m[0, 5, 1, 2] = 1                           # the rounding tie: x = 0 and x = 1 give x = 1
    m[0, 0, 7, 3] = m[0, 1, 7, 3] = 1                           # and in y
    m[1, :, :, 1] = m[0, :, :, 0]                               # slice 1: channel 0 empty
    m[2, :, :, 0] = _blobs(np.random.default_rng(8), h, w, 0.3, 2)
    m[2, :, :, 2] = _blobs(np.random.default_rng(9), h, w, 0.5, 1)
    stack = _dev(cuda, m)
    mom = shape.moments_stack(stack)
    want_mom = S.moments(m)
    _diff(mom.cpu().numpy(), want_mom, 'moments')
    own = shape.origins(stack, mom)
    assert own.dtype == torch.int32 and tuple(own.shape) == (3, 4, 3)
    own = own.cpu().numpy()
    _diff(own, S.origins(m, want_mom), 'own')
    assert tuple(own[0, 0]) == (40, 12, 1) and tuple(own[0, 1]) == (20, 20, 0) and tuple(own[0, 2]) == (1, 5, 1) and tuple(own[0, 3]) == (7, 1, 1)
    assert tuple(own[1, 0]) == (-1, -1, 0) and tuple(own[1, 2]) == (-1, -1, 0)
    for ref in (0, 1, 2, 'Lumen'):
        ch = CLASS_IDS[ref] - 1 if isinstance(ref, str) else ref
        got = shape.origins(stack, mom, ref).cpu().numpy()
        _diff(got, S.origins(m, want_mom, ch), ('ref', ref))
        assert (got[:, :, :2] == got[:, ch:ch + 1, :2]).all()
    got = shape.origins(stack, mom, 0).cpu().numpy()
    assert (got[1] == (-1, -1, 0)).all() and tuple(got[0, 1]) == (40, 12, 0)    # an empty source plane; the ring is clear at the disc's centroid
    with pytest.raises(ValueError, match='channel'):
        shape.origins(stack, mom, 4)
    with pytest.raises(ValueError, match='mom'):
        shape.origins(stack, mom.to(torch.int32))


def _check_profile(prof, length, org, h, w):
    """Shapes, and the invariants of the five fields against the ray's own length."""
    met = prof[..., IN] > 0
    assert (prof >= 0).all() and (length >= 0).all()
    assert (prof[..., IN] <= prof[..., OUT]).all() and (prof[..., OUT] <= prof[..., LAST]).all() and (prof[..., LAST] <= length).all()
    assert (prof[..., OUT] >= 1)[met].all() and not prof[~met].any()
    assert (prof[..., HITS] >= prof[..., OUT] - prof[..., IN] + 1)[met].all()
    assert ((prof[..., RUNS] >= 1) == met).all()
    outside = ~((org[..., 0] >= 0) & (org[..., 0] < w) & (org[..., 1] >= 0) & (org[..., 1] < h))
    assert not length[outside].any() and not prof[outside].any()


def _walk(stack, origin):
    n, h, w, sc = (int(v) for v in stack.shape)
    prof, length, org = shape.centred_profile(stack, origin)
    assert prof.dtype == length.dtype == org.dtype == torch.int32
    assert tuple(prof.shape) == (n, sc, 360, 5) and tuple(length.shape) == (n, sc, 360) and tuple(org.shape) == (n, sc, 3)
    prof, length, org = prof.cpu().numpy(), length.cpu().numpy(), org.cpu().numpy()
    _check_profile(prof, length, org, h, w)
    return prof, length, org


@pytest.mark.parametrize('h,w', SHAPES)
@pytest.mark.parametrize('n', [1, 3])
def test_polar_at_equals_restatement(cuda, n, h, w):
    """Own origins (a walk per channel) and shared origins (one gather for all channels); one reference per mode over eight channels: a
    channel's walk depends on its own plane and origin only, so the 1-, 4-, 5-channel stacks and the unaligned view reuse it.  The shared
    origin is channel 0's centroid, which every sub-stack contains."""
    masks = _masks(n, h, w, 8)
    mom = S.moments(masks)
    off = _offsets(h, w)
    for mode, ref in (('own', -1), (0, 0)):
        want_org = S.origins(masks, mom, ref)
        want, want_len = S.polar_at(masks, want_org, off)
        for sc in (1, 4, 5, 8):
            prof, length, org = _walk(_dev(cuda, masks[..., :sc]), mode)
            _diff(org, want_org[:, :sc], (n, h, w, sc, mode, 'origins'))
            _diff(prof, want[:, :sc], (n, h, w, sc, mode, 'prof'))
            _diff(length, want_len[:, :sc], (n, h, w, sc, mode, 'len'))
        prof, length, org = _walk(_unaligned(cuda, masks[..., :4]), mode)
        _diff(prof, want[:, :4], (n, h, w, 'unaligned', mode, 'prof'))
        _diff(length, want_len[:, :4], (n, h, w, 'unaligned', mode, 'len'))
    if h * w == 97 * 130:
        assert want_len.max() > 64 and (want_len < 64).any()    # rays on both sides of a chunk seam


def test_polar_at_explicit_origins(cuda):
    h, w = 33, 70
    masks = _masks(2, h, w, 4)
    masks[1] = 1                                                # a full slice: every ray runs to the frame, OUT == len
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (-1, 5), (w, 5), (5, -1), (5, h), (-1, -1), (2 ** 31 - 1, 3), (-2 ** 31, 3), (35, 16)]
    off = _offsets(h, w)
    for k in range(0, len(pts), 4):
        org = np.zeros((2, 4, 2), np.int32)
        org[:, :] = np.array(pts[k:k + 4], np.int64).astype(np.int32)
        want, want_len = S.polar_at(masks, org, off)
        prof, length, got_org = _walk(_dev(cuda, masks), torch.from_numpy(org).to(cuda))
        _diff(got_org[..., :2], org, 'two columns are padded, not changed')
        _diff(prof, want, ('explicit', k, 'prof'))
        _diff(length, want_len, ('explicit', k, 'len'))
        inside = (org[1, :, 0] >= 0) & (org[1, :, 0] < w) & (org[1, :, 1] >= 0) & (org[1, :, 1] < h)
        assert (prof[1, inside, :, OUT] == length[1, inside]).all() and (length[1, ~inside] == 0).all()
    assert length[0, 3, 0] == w - 1 - 35 and length[0, 3, 180] == 35 and length[0, 3, 90] == h - 1 - 16 and length[0, 3, 270] == 16
    three = torch.zeros((2, 4, 3), dtype=torch.int32, device=cuda)
    three[:, :, 0], three[:, :, 1], three[:, :, 2] = 35, 16, 77           # the third column is not read
    prof3, length3, _ = _walk(_dev(cuda, masks), three)
    same = np.zeros((2, 4, 2), np.int32)
    same[:, :] = (35, 16)
    want, want_len = S.polar_at(masks, same, off)
    _diff(prof3, want, 'shared explicit')
    _diff(length3, want_len, 'shared explicit len')
    for bad in (three.to(torch.int64), three[:1], three.cpu(), three[:, :, :1]):
        with pytest.raises(ValueError, match='origin'):
            shape.centred_profile(_dev(cuda, masks), bad)


def test_chunk_seams_of_the_64_lane_walk_from_an_edge_origin(cuda):
    """A 40 x 300 frame, origin (0, 20): angle 0 has 299 steps inside the frame, chunks of 64, 64, 64, 64 and 43.  The step patterns of
    test_gpu_polar.py's seam test laid along it, and their like at the later seams and at the ray's end."""
    h, w = 40, 300
    patterns = [([64], (64, 64, 64, 1, 1)), ([65], (65, 65, 65, 1, 1)), ([128], (128, 128, 128, 1, 1)), ([129], (129, 129, 129, 1, 1)),
                (list(range(60, 65)) + list(range(66, 71)), (60, 64, 70, 10, 2)),
                (list(range(1, 65)), (1, 64, 64, 64, 1)), (list(range(65, 150)), (65, 149, 149, 85, 1)),
                (list(range(1, 150)), (1, 149, 149, 149, 1)),
                (list(range(1, 150, 2)), (1, 1, 149, 75, 75)), (list(range(2, 150, 2)), (2, 2, 148, 74, 74)),
                (list(range(1, 150, 3)), (1, 1, 148, 50, 50)), (list(range(3, 150, 3)), (3, 3, 147, 49, 49)),
                (list(range(2, 150, 3)) + list(range(3, 150, 3)), (2, 3, 149, 99, 50)),
                (list(range(140, 150)), (140, 149, 149, 10, 1)), ([63, 64, 65, 127, 128, 129], (63, 65, 129, 6, 2)),
                ([64, 128], (64, 64, 128, 2, 2)), ([1, 149], (1, 1, 149, 2, 2)),
                ([192, 193, 256, 257], (192, 193, 257, 4, 2)), (list(range(1, 300)), (1, 299, 299, 299, 1)),
                (list(range(257, 300)), (257, 299, 299, 43, 1)), ([299], (299, 299, 299, 1, 1)), ([256, 299], (256, 256, 299, 2, 2)),
                (list(range(1, 300, 2)), (1, 1, 299, 150, 150)), (list(range(190, 260)), (190, 259, 259, 70, 1))]
    while len(patterns) % 4:
        patterns.append(([], (0, 0, 0, 0, 0)))
    m = np.zeros((len(patterns) // 4, h, w, 4), np.float32)
    for i, (steps, _) in enumerate(patterns):
        for r in steps:
            m[i // 4, 20, r, i % 4] = 1                         # angle 0 from (0, 20): step r is pixel (20, r)
    org = np.zeros((m.shape[0], 4, 2), np.int32)
    org[:, :] = (0, 20)
    prof, length, _ = _walk(_dev(cuda, m), torch.from_numpy(org).to(cuda))
    want, want_len = S.polar_at(m, org, _offsets(h, w))
    _diff(prof, want, 'seams prof')
    _diff(length, want_len, 'seams len')
    assert (length[:, :, 0] == 299).all() and (length[:, :, 180] == 0).all()
    for i, (steps, fields) in enumerate(patterns):
        assert tuple(prof[i // 4, i % 4, 0]) == fields, (i, steps[:4], tuple(prof[i // 4, i % 4, 0]), fields)


def test_abi_on_the_device(cuda):
    """Every refusal returns -5 and leaves sentinel-filled outputs untouched; a null table is fine without steps; wild table entries end the ray,
    they are never followed."""
    from oct_segmentation_amd import _lib as L
    lib = L.lib()
    h, w = 8, 9
    off_np = shape.ray_offsets(h, w)
    width = off_np.shape[1]
    s = torch.ones((1, h, w, 4), dtype=torch.float32, device=cuda)
    big = torch.ones((1, 2, 2, 17), dtype=torch.float32, device=cuda)
    off = torch.from_numpy(off_np).to(cuda)
    mom = torch.full((2 * 17 * 12 + 1,), 9, dtype=torch.int64, device=cuda)
    org = torch.full((2 * 17 * 3,), 9, dtype=torch.int32, device=cuda)
    prof = torch.full((2 * 9 * 360 * 5,), 9, dtype=torch.int32, device=cuda)
    length = torch.full((2 * 9 * 360,), 9, dtype=torch.int32, device=cuda)
    at = torch.tensor([[[4, 4, 0]] * 4], dtype=torch.int32, device=cuda)
    st, p = L.stream_ptr(), L.ptr

    def moments(stack=s, N=1, H=h, W=w, SC=4, out=mom):
        return lib.octseg_stack_moments(p(stack), N, H, W, SC, p(out), st)

    def origins(stack=s, m=mom, N=1, H=h, W=w, SC=4, ref=-1, out=org):
        return lib.octseg_moment_origins(p(stack), p(m), N, H, W, SC, ref, p(out), st)

    def walk(stack=s, N=1, H=h, W=w, SC=4, o=at, ro=off, R_=width, pr=prof, ln=length):
        return lib.octseg_stack_polar_at(p(stack), N, H, W, SC, p(o), p(ro), R_, p(pr), p(ln), st)

    shapes = ({'N': 0}, {'H': 0}, {'W': -1}, {'SC': 0}, {'H': 32769, 'W': 1}, {'H': 1, 'W': 32769}, {'H': 65536, 'W': 32768})
    for kw in ({'stack': None}, {'out': None}, {'SC': 17, 'stack': big}, {'out': mom[1:].view(torch.uint8)[4:]}) + shapes:
        assert moments(**kw) == -5, kw
    for kw in ({'stack': None}, {'m': None}, {'out': None}, {'SC': 17, 'stack': big}, {'ref': 4}, {'ref': 100}, {'m': mom.view(torch.uint8)[4:]}) + shapes:
        assert origins(**kw) == -5, kw
    for kw in ({'stack': None}, {'o': None}, {'ro': None}, {'pr': None}, {'ln': None}, {'SC': 9}, {'R_': -1}) + shapes:
        assert walk(**kw) == -5, kw
    torch.cuda.synchronize()
    assert (mom == 9).all() and (org == 9).all() and (prof == 9).all() and (length == 9).all()      # nothing was launched
    assert b'stack_polar_at' in lib.octseg_last_error()
    # accepted calls write their own extent and nothing beyond it
    assert moments() == 0 and origins(ref=-5) == 0 and walk(ro=None, R_=0) == 0                     # any negative ref_channel is "own"
    torch.cuda.synchronize()
    assert (mom[4 * 12:] == 9).all() and (org[4 * 3:] == 9).all() and (prof[4 * 360 * 5:] == 9).all() and (length[4 * 360:] == 9).all()
    assert tuple(mom[:12].tolist()) == (72, 72 * 4, 36 * 7, 8 * 204, 36 * 28, 9 * 140, 0, 8, 0, 7, 34, 0)
    assert tuple(org[:3].tolist()) == (4, 4, 1)                 # (2 * 288 + 72) // 144 = 4, (2 * 252 + 72) // 144 = 4
    assert not prof[:4 * 360 * 5].any() and not length[:4 * 360].any()      # no table, no steps
    wild = off.clone()
    wild[0, 2] = torch.tensor([2 ** 31 - 1, 0], dtype=torch.int32)          # step 3 of degree 0 ...
    wild[1, 1] = torch.tensor([0, -2 ** 31], dtype=torch.int32)
    wild[2, 0] = torch.tensor([10 ** 6, 10 ** 6], dtype=torch.int32)
    wild[3, 3] = torch.tensor([-2 ** 31, -2 ** 31], dtype=torch.int32)
    far = torch.tensor([[[4, 4, 0], [2 ** 31 - 1, 2 ** 31 - 1, 0], [-2 ** 31, 0, 0], [8, 7, 0]]], dtype=torch.int32, device=cuda)
    assert walk(ro=wild, o=far) == 0
    torch.cuda.synchronize()
    got = prof[:4 * 360 * 5].view(1, 4, 360, 5).cpu().numpy()
    got_len = length[:4 * 360].view(1, 4, 360).cpu().numpy()
    want, want_len = S.polar_at(np.ones((1, h, w, 4), np.float32), far.cpu().numpy(), wild.cpu().numpy())
    _diff(got, want, 'wild prof')
    _diff(got_len, want_len, 'wild len')
    assert list(got_len[0, 0, :4]) == [2, 1, 0, 3] and not got_len[0, 1:3].any() and got_len[0, 3, 0] == 0 and got_len[0, 3, 180] == 8
    assert (prof[4 * 360 * 5:] == 9).all() and (length[4 * 360:] == 9).all()


def test_demo_excerpt_equals_restatement(cuda):
    """Slices 0, 1, 8, 12 and 2 of the demo excerpt, 750 x 750: moments, origins and both walks against the restatement, the lumen report
    against the report of the restatement's integers, and polar.build_report on the lumen-centred profile."""
    fx = R.load_fixture(FIXTURE)
    pick = [0, 1, 8, 12, 2]
    masks = fx['stack'][pick]
    names = [fx['names'][i] for i in pick]
    n, h, w, sc = masks.shape
    stack = _dev(cuda, masks)
    lumen = CLASS_IDS['Lumen'] - 1
    off = _offsets(h, w)
    want_mom = S.moments(masks)
    _diff(_moments(stack), want_mom, 'demo moments')
    for mode, ref in (('own', -1), ('Lumen', lumen)):
        want_org = S.origins(masks, want_mom, ref)
        want, want_len = S.polar_at(masks, want_org, off)
        prof, length, org = _walk(stack, mode)
        _diff(org, want_org, ('demo origins', mode))
        _diff(prof, want, ('demo prof', mode))
        _diff(length, want_len, ('demo len', mode))
    assert (want_mom[:, lumen, 0] > 0).all() and (want_org[:, lumen, 2] == 1).all()
    rep = shape.lumen_report(stack, names)
    assert rep == S.lumen_report(want_mom[:, lumen], want_org[:, lumen], want[:, lumen], want_len[:, lumen], h, w, names, 112)
    assert rep['ratio'] == 112 and rep['lumen']['slice'] == [0, 1, 2, 3, 4] and json.loads(json.dumps(rep)) == rep
    assert all(d is not None and 0 < lo <= d <= hi for lo, d, hi in zip(rep['lumen']['d_min'], rep['lumen']['d_equivalent'], rep['lumen']['d_max']))
    windowed = shape.lumen_report(stack, names, ratio=100, ref_window=1)
    assert windowed == S.lumen_report(want_mom[:, lumen], want_org[:, lumen], want[:, lumen], want_len[:, lumen], h, w, names, 100, ref_window=1)
    # the lumen-centred profile is a profile: the plaque report's host code takes it unchanged
    plaque = polar.build_report(prof, h, names)
    assert plaque == polar.build_report(want, h, names) and json.loads(json.dumps(plaque)) == plaque
    assert polar.carpet_view(prof, list(CLASS_IDS)).shape == (360, n, 3)
    t = shape.shape_table(shape.moments_stack(stack))
    assert (t['area'] == want_mom[:, :, 0]).all() and (t['major'] >= t['minor']).all() and (t['minor'][:, lumen] > 0).all()
    own = shape.centred_profile(stack, 'own')[0]
    ct = shape.centroid_thickness(own[0, lumen])
    assert ct['min'] >= 1 and ct['max'] >= ct['median'] >= ct['min'] and len(ct['all_measurements']) == 360


def test_report_with_clean_and_other_outputs_unchanged(cuda):
    from oct_segmentation_amd import analysis, cleanup
    rng = np.random.default_rng(5)
    n, h, w = 3, 60, 64
    masks = np.stack([np.stack([_blobs(rng, h, w, 0.35, 2) for _ in range(4)], axis=-1) for _ in range(n)]).astype(np.float32)
    stack = _dev(cuda, masks)
    before = analysis.analyze_stack(stack)
    rep = shape.lumen_report(stack, clean=True)
    cleaned = cleanup.clean_stack(stack)
    assert not torch.equal(cleaned, stack)
    assert rep == shape.lumen_report(cleaned) and rep != shape.lumen_report(stack) and rep == shape.lumen_report(stack, clean={})
    assert rep['images'] == ['0', '1', '2'] and rep['ratio'] == 9
    assert torch.equal(stack, _dev(cuda, masks)) and analysis.analyze_stack(stack) == before      # the input is not written
    with pytest.raises(ValueError, match='ratio'):
        shape.lumen_report(torch.ones((1, 5, 5, 4), device=cuda))
    with pytest.raises(ValueError, match='ratio'):
        shape.lumen_report(stack, ratio=0)
    with pytest.raises(ValueError, match='unknown class'):
        shape.lumen_report(stack, lumen='Thrombus')
    with pytest.raises(ValueError, match='unknown class'):
        shape.centred_profile(stack, 'Thrombus')
    with pytest.raises(ValueError, match='channel'):
        shape.lumen_report(stack[..., :1], lumen='Vasa vasorum')
    with pytest.raises(NotImplementedError):                    # the refusal of the contour thickness stands
        analysis.analyze_stack(stack, thickness='contour')


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


def test_predict_main_writes_lumen_json(cuda, tmp_path):
    """Both input kinds: a directory of files (sorted file-name order, as analysis=true) and a .npy volume (analyze_pullback)."""
    from oct_segmentation_amd import predict, pullback
    models = _models_dir(cuda, os.path.join(tmp_path, 'models'))
    rng = np.random.default_rng(17)
    data_dir = os.path.join(tmp_path, 'input')
    os.makedirs(data_dir)
    created = ['z_last', 'a_first', 'm_mid']                    # sorted order differs from creation order
    for name in created:
        Image.fromarray(rng.integers(0, 255, (90, 90, 3), dtype=np.uint8)).save(os.path.join(data_dir, f'{name}.png'))
    args = [f'data_dir={data_dir}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32', 'analysis=true', 'plaque=true']
    off, on, cl = os.path.join(tmp_path, 'off'), os.path.join(tmp_path, 'on'), os.path.join(tmp_path, 'clean')
    assert predict.main(args + [f'save_dir={off}']) == 0
    assert predict.main(args + [f'save_dir={on}', 'lumen=true']) == 0
    a, b = _files(off), _files(on)
    assert sorted(b) == sorted(list(a) + ['lumen.json']) and 'analysis.json' in a and 'plaque.json' in a
    for name in a:                                              # analysis.json, plaque files, overlays and colour masks do not change
        assert a[name] == b[name], name
    names = sorted(created)
    images, _ = predict.data_processing([os.path.join(data_dir, f'{n}.png') for n in names], [120, 120])
    stack = predict.segment_stack(images, [120, 120], list(CLASS_IDS), models, device='cuda', compute_dtype=torch.float32, device_preprocess=True)
    want = shape.lumen_report(stack, names)
    got = json.loads(b['lumen.json'])
    assert got == json.loads(json.dumps(want)) and got['images'] == names and got['ratio'] == 18
    assert predict.main(args + [f'save_dir={cl}', 'lumen=true', 'clean=true']) == 0
    assert json.loads(_files(cl)['lumen.json']) == json.loads(json.dumps(shape.lumen_report(stack, names, clean=True)))
    # the volume path
    vol = rng.integers(0, 256, (2, 90, 90, 3), dtype=np.uint8)
    np.save(os.path.join(tmp_path, 'pull.npy'), vol)
    vargs = [f'data_dir={os.path.join(tmp_path, "pull.npy")}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32', 'analysis=true']
    voff, von = os.path.join(tmp_path, 'voff'), os.path.join(tmp_path, 'von')
    assert predict.main(vargs + [f'save_dir={voff}']) == 0
    assert predict.main(vargs + [f'save_dir={von}', 'lumen=true']) == 0
    a, b = _files(voff), _files(von)
    assert sorted(b) == sorted(list(a) + ['lumen.json']) and len(a) == 5
    for name in a:
        assert a[name] == b[name], name
    res = pullback.analyze_pullback(vol, models, list(CLASS_IDS), output_size=(120, 120), names=['pull_001', 'pull_002'], compute_dtype=torch.float32,
                                    lumen=True)
    assert res.lumen == shape.lumen_report(res.stack, ['pull_001', 'pull_002'], ratio=13) and res.lumen['ratio'] == 13 and res.plaque is None
    assert json.loads(b['lumen.json']) == json.loads(json.dumps(res.lumen))
    plain = pullback.analyze_pullback(vol, models, list(CLASS_IDS), output_size=(120, 120), names=['pull_001', 'pull_002'], compute_dtype=torch.float32)
    assert plain.lumen is None and plain.data == res.data and torch.equal(plain.stack, res.stack)
    wide = pullback.analyze_pullback(vol, models, list(CLASS_IDS), output_size=(120, 120), compute_dtype=torch.float32,
                                     lumen={'ref_window': 1, 'ratio': 7}, clean=True)
    assert wide.lumen == shape.lumen_report(wide.stack, ['001', '002'], ratio=7, ref_window=1)
    for bad in ({'bogus': 1}, 'yes'):                           # refused before any work
        with pytest.raises(ValueError, match='lumen'):
            pullback.analyze_pullback(vol, models, list(CLASS_IDS), output_size=(120, 120), compute_dtype=torch.float32, lumen=bad)
