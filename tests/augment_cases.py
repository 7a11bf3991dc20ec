"""Cases of the augmentation kernel's element-wise tests, shared by tests/test_augment_kernel.py (CPU: the restatement against torch
indexing, the oracle's stages and its own caps) and tests/test_gpu_augment.py (GPU: the kernel against the restatement).

Families (FAMILIES[name]() -> list of Case; built once per process and kept):
  exact     Rule X, B = 3 with a different row per frame (the per-frame parameter stride), C in {1, 4, 5}, frames 1 x 1, 1 x 70, 7 x 5, 48 x 80,
            80 x 48, random uint8 images; tables exact in float32; expected values from torch indexing, bit for bit, nothing two-valued
  stride    B = 17 at 512 x 512: 4 456 448 pixels > 16384 workgroups x 256 threads, so the grid-stride loop takes its second trip
  warp      sample_frame tables that hold ssr or perspective, geometry only, smooth frames (synth.make_batch), 64 x 64 and 48 x 80
  cropwarp  sample_frame tables with crop and perspective and no ssr: where parameters 20 .. 32 matter
  bc        all 256 levels per channel under seeded (alpha, beta) draws and the three skip branches
  hsv       all 256 x 256 (c0, c1) pairs at 16 values of c2: the pure round trip, and seven shift triples
  noise     a ramp with rows of 0 and 255 under four sigmas and five seeds, one seed twice
  chain     200 full sample_frame rows

Non-square frames test the kernel, not the sampler: sample_frame stays square-only, and on 48 x 80 it is called with S = 80 -- the table is only
a transform and the kernel does not care.  Caps (share of pixels that are two-valued or open) are the ones of the issue that introduced these
tests; the restatement alone has to stay inside them (test_augment_kernel.py).
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import augment_kernel_ref as KR
from oct_segmentation_amd import augment as A
from synth import make_batch

NONE_RECT = (-1e9, -1e9, 1e9, 1e9)


@dataclass
class Case:
    id: str
    params: np.ndarray                 # float32 [B, NPARAM]
    img: torch.Tensor                  # float32 [B, 3, H, W]
    mask: torch.Tensor                 # float32 [B, C, H, W]
    expect: Optional[tuple] = None     # (img, mask) from torch indexing: Rule X
    cap_img: float = 0.0               # largest share of two-valued + open image pixels
    cap_mask: float = 0.0
    logs: Optional[list] = None
    unit: str = 'pixel'                # what cap_img counts: pixels (any channel) or elements
    _ref: Optional[KR.Result] = None

    def ref(self):
        if self._ref is None:
            self._ref = KR.augment_ref(self.params, self.img.numpy(), self.mask.numpy())
        return self._ref


def row(Hinv=None, Pinv=None, rect=NONE_RECT, alpha=1.0, beta=0.0, sigma=0.0, seed=0, hue=0.0, sat=0.0, val=0.0, hsv_on=False):
    """One table row from the INVERSE homographies as they are stored (no matrix inversion on the way: the entries stay exact)."""
    r = np.zeros(A.NPARAM, dtype=np.float32)
    r[0:9] = np.asarray(np.eye(3) if Hinv is None else Hinv, dtype=np.float64).reshape(9)
    r[20:29] = np.asarray(np.eye(3) if Pinv is None else Pinv, dtype=np.float64).reshape(9)
    r[29:33] = rect
    r[9], r[10], r[11] = alpha, beta, sigma
    r[12] = np.array([seed], dtype=np.uint32).view(np.float32)[0]
    r[13], r[14], r[15] = hue, sat, val
    r[16] = 1.0 if hsv_on else 0.0
    return r


def geometry_only(M, post, rect):
    return A.pack_params(M, post=post, rect=rect)


def _random_frames(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, 3, H, W), generator=g).float(), (torch.rand(B, C, H, W, generator=g) > 0.5).float()


# ------------------------------------------------------------------------------------------------ torch-indexing expectations (one frame, [K, H, W])
def shifted(t, dx, dy):
    """out(x, y) = t(x - dx, y - dy), 0 outside."""
    K, H, W = t.shape
    out = torch.zeros_like(t)
    ys, xs = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[:, ys, xs] = t[:, ys.start - dy:ys.stop - dy, xs.start - dx:xs.stop - dx]
    return out


def windowed(t, rect):
    xl, yl, xh, yh = (int(v) for v in rect)
    out = torch.zeros_like(t)
    ys, xs = slice(max(0, yl), max(0, yh)), slice(max(0, xl), max(0, xh))
    out[:, ys, xs] = t[:, ys, xs]
    return out


def transposed(t):
    K, H, W = t.shape
    out = torch.zeros_like(t)
    m = min(H, W)
    out[:, :m, :m] = t.transpose(-1, -2)[:, :m, :m]
    return out


def _magnify_axis(t, axis, nearest):
    """sx = x / 2 + 1 / 4: even outputs sit a quarter into cell x / 2, odd ones three quarters (weights 3/4 1/4 | 1/4 3/4; nearest: x / 2 | x / 2 + 1)."""
    n = t.shape[axis]
    tp = torch.cat([t, torch.zeros_like(t.narrow(axis, 0, 1))], dim=axis)
    k = torch.arange(n) // 2
    odd = (torch.arange(n) % 2 == 1)
    if nearest:
        return tp.index_select(axis, k + odd.long())
    shape = [1, 1, 1]
    shape[axis] = n
    w1 = torch.where(odd, 0.75, 0.25).to(torch.float64).view(shape)
    return tp.index_select(axis, k) * (1 - w1) + tp.index_select(axis, k + 1) * w1


def magnified(t, nearest):
    t = t.to(torch.float64)
    v = _magnify_axis(_magnify_axis(t, 2, nearest), 1, nearest)
    return (v if nearest else torch.round(v)).float()            # torch.round: ties to even, like rintf


def _exact_transforms(H, W):
    """-> list of (name, row, f(t, is_mask) -> expected [K, H, W])."""
    flip = [[-1, 0, W - 1], [0, 1, 0], [0, 0, 1]]
    sh = lambda dx, dy: [[1, 0, -dx], [0, 1, -dy], [0, 0, 1]]      # noqa: E731  inverse of a shift by (dx, dy)
    flip_sh = lambda dx, dy: [[-1, 0, W - 1 + dx], [0, 1, -dy], [0, 0, 1]]      # noqa: E731  source of x: flip(x - dx)
    reg = (W // 8, H // 8, max(W // 8 + 1, W - W // 6), max(H // 8 + 1, H - H // 6))
    one = (W // 2, H // 3, W // 2 + 1, H // 3 + 1)
    empty = (W // 2, H // 8, W // 2, H)
    dxc, dyc = 2, -1
    T = [('identity', row(), lambda t, m: t),
         ('hflip', row(flip), lambda t, m: t.flip(-1)),
         ('vflip', row([[1, 0, 0], [0, -1, H - 1], [0, 0, 1]]), lambda t, m: t.flip(-2)),
         ('shift', row(sh(5, -3)), lambda t, m: shifted(t, 5, -3)),
         ('shift_out', row(sh(W + 3, 0)), lambda t, m: torch.zeros_like(t)),
         ('shift_far', row(sh(1000000, -1000000)), lambda t, m: torch.zeros_like(t)),
         ('magnify', row([[.5, 0, .25], [0, .5, .25], [0, 0, 1]]), lambda t, m: magnified(t, m)),
         ('magnify_w2', row([[1, 0, .5], [0, 1, .5], [0, 0, 2]]), lambda t, m: magnified(t, m)),
         ('crop', row(sh(dxc, dyc), rect=reg), lambda t, m: windowed(shifted(t, dxc, dyc), reg)),
         ('crop_one', row(sh(dxc, dyc), rect=one), lambda t, m: windowed(shifted(t, dxc, dyc), one)),
         ('crop_empty', row(sh(dxc, dyc), rect=empty), lambda t, m: windowed(shifted(t, dxc, dyc), empty)),
         ('crop_flip', row(flip_sh(dxc, dyc), rect=reg), lambda t, m: windowed(shifted(t.flip(-1), dxc, dyc), reg)),
         ('crop_one_flip', row(flip_sh(dxc, dyc), rect=one), lambda t, m: windowed(shifted(t.flip(-1), dxc, dyc), one))]
    if H != W:
        T.append(('transpose', row([[0, 1, 0], [1, 0, 0], [0, 0, 1]]), lambda t, m: transposed(t)))
    return T


def exact_cases():
    cases = []
    for k, (H, W) in enumerate([(1, 1), (1, 70), (7, 5), (48, 80), (80, 48)]):
        T = _exact_transforms(H, W)
        for j in range(0, len(T), 3):
            trio = [T[(j + i) % len(T)] for i in range(3)]
            C = (1, 4, 5)[(k + j // 3) % 3]
            img, mask = _random_frames(3, C, H, W, seed=100 * k + j)
            ei = torch.stack([f(img[n], False) for n, (_, _, f) in enumerate(trio)])
            em = torch.stack([f(mask[n], True) for n, (_, _, f) in enumerate(trio)])
            cases.append(Case(f'exact {H}x{W} C{C} ' + '+'.join(t[0] for t in trio), np.stack([t[1] for t in trio]), img, mask, (ei, em)))
    return cases


def stride_cases():
    B, S = 17, 512
    img, mask = _random_frames(B, 1, S, S, seed=7)
    flip = [[-1, 0, S - 1], [0, 1, 0], [0, 0, 1]]
    kinds = [(row(), lambda t: t), (row(flip), lambda t: t.flip(-1)), (row([[1, 0, -5], [0, 1, 3], [0, 0, 1]]), lambda t: shifted(t, 5, -3))]
    ei = torch.stack([kinds[n % 3][1](img[n]) for n in range(B)])
    em = torch.stack([kinds[n % 3][1](mask[n]) for n in range(B)])
    return [Case('stride 17x512x512', np.stack([kinds[n % 3][0] for n in range(B)]), img, mask, (ei, em))]


# ------------------------------------------------------------------------------------------------ sampled geometry
def _sampled(S, n, seed, keep):
    """n frames of sample_frame(S) whose log passes keep(log) -> (geometry-only rows, logs)."""
    rng = np.random.default_rng(seed)
    rows, logs = [], []
    while len(rows) < n:
        M, post, rect, *_, log = A.sample_frame(S, rng)
        if keep(log):
            rows.append(geometry_only(M, post, rect)); logs.append({k: v for k, v in log.items() if k in GEOMETRIC})
    return np.stack(rows), logs


GEOMETRIC = ('hflip', 'ssr', 'crop', 'perspective', 'perspective_matrix')


def _smooth(B, C, H, W, seed):
    img, mask = make_batch(B, C, max(H, W), seed=seed)
    return img[:, :, :H, :W].contiguous(), mask[:, :, :H, :W].contiguous()


def warp_cases():
    keep = lambda log: 'ssr' in log or 'perspective' in log      # noqa: E731
    out = []
    for H, W, seed in ((64, 64, 11), (48, 80, 12)):
        rows, logs = _sampled(max(H, W), 24, seed, keep)
        img, mask = _smooth(24, 2, H, W, seed=seed + 30)
        out.append(Case(f'warp {H}x{W}', rows, img, mask, None, 0.01, 0.001, logs))
    return out


def cropwarp_cases():
    keep = lambda log: 'crop' in log and 'perspective' in log and 'ssr' not in log      # noqa: E731
    out = []
    for H, W, seed in ((64, 64, 21), (48, 80, 22)):
        rows, logs = _sampled(max(H, W), 8, seed, keep)
        img, mask = _smooth(8, 2, H, W, seed=seed + 30)
        out.append(Case(f'cropwarp {H}x{W}', rows, img, mask, None, 0.01, 0.001, logs))
    return out


# ------------------------------------------------------------------------------------------------ photometric
def bc_cases():
    B = 64
    rng = np.random.default_rng(31)
    ab = [(np.float32(1 + rng.uniform(-A.CONTRAST_LIMIT, A.CONTRAST_LIMIT)), np.float32(rng.uniform(-A.BRIGHTNESS_LIMIT, A.BRIGHTNESS_LIMIT)))
          for _ in range(B - 3)]
    ab += [(np.float32(1.0), ab[0][1]), (ab[1][0], np.float32(0.0)), (np.float32(1.0), np.float32(0.0))]      # the kernel's skip branches
    lv = torch.arange(256, dtype=torch.float32)
    img = torch.stack([torch.stack([lv.roll(85 * c + n).view(16, 16) for c in range(3)]) for n in range(B)])
    mask = torch.zeros(B, 1, 16, 16)
    return [Case('bc 64x16x16', np.stack([row(alpha=a, beta=b) for a, b in ab]), img, mask, None, 0.002, 0.0, unit='element')]


HSV_C2 = (0, 1, 2, 30, 63, 64, 100, 127, 128, 129, 191, 200, 222, 253, 254, 255)
HSV_SHIFTS = ((10, -15, 12), (-14.3, 19.6, -7.2), (3.7, 0, 0), (0, -20, 0), (0, 0, 15), (-180, 0, 0), (179.25, 255, -255))


def hsv_cases():
    B, S = 16, 256
    lv = torch.arange(S, dtype=torch.float32)
    img = torch.stack([torch.stack([lv.view(S, 1).expand(S, S), lv.view(1, S).expand(S, S), torch.full((S, S), float(c2))]) for c2 in HSV_C2])
    mask = torch.zeros(B, 1, S, S)
    zero = np.stack([row(hsv_on=True) for _ in range(B)])
    sh = np.stack([row(hue=HSV_SHIFTS[n % 7][0], sat=HSV_SHIFTS[n % 7][1], val=HSV_SHIFTS[n % 7][2], hsv_on=True) for n in range(B)])
    return [Case('hsv round trip', zero, img.contiguous(), mask, None, 0.02, 0.0), Case('hsv shifts', sh, img.contiguous(), mask, None, 0.02, 0.0)]


NOISE_FRAMES = ((0, 1.5 ** 0.5), (1, 2.0), (2 ** 31 - 2, 6.5 ** 0.5), (0xFFFFFFFF, 0.01), (4242, 2.0), (4242, 2.0))


def noise_cases():
    """The sigma = 0.01 frame decides the family's two-valued share: there px + n leaves px's integer only through |n| < band, and with the Rule E
    floor 10 u px that happens with probability 2 * 10 u px / (0.01 sqrt(2 pi)) = 4.8e-5 px: 0.6 % of a frame whose mean level is 127, 0.1 % of the
    family -- the cap itself.  24 rows of 0 (mean level 88) put the frame at 0.42 % and the family, with the other five frames' 0.01 % each,
    at 0.08 %.  The rows of 0 are also where the lower clamp is hit at every sigma; the upper one needs only a few rows."""
    B, S = len(NOISE_FRAMES), 64
    ramp = torch.round(torch.linspace(0, 255, S)).view(1, S).expand(S, S).clone()
    ramp[:24] = 0.0
    ramp[-4:] = 255.0
    img = ramp.view(1, 1, S, S).expand(B, 3, S, S).contiguous()
    mask = torch.zeros(B, 1, S, S)
    return [Case('noise 6x64x64', np.stack([row(sigma=s, seed=seed) for seed, s in NOISE_FRAMES]), img, mask, None, 0.001, 0.0, unit='element')]


DECISIONS = ('hflip', 'ssr', 'crop', 'noise', 'perspective', 'bc', 'hsv')


def chain_cases():
    S, N = 64, 200
    rng = np.random.default_rng(41)
    img, mask = make_batch(N, 2, S, seed=42)
    rows, logs = [], []
    for _ in range(N):
        M, post, rect, alpha, beta, sigma, seed, hue, sat, val, hsv_on, log = A.sample_frame(S, rng)
        rows.append(A.pack_params(M, alpha, beta, sigma, seed, hue, sat, val, hsv_on, post, rect)); logs.append(log)
    return [Case('chain 200x64x64', np.stack(rows), img, mask, None, 0.01, 0.001, logs)]


_BUILDERS = dict(exact=exact_cases, stride=stride_cases, warp=warp_cases, cropwarp=cropwarp_cases, bc=bc_cases, hsv=hsv_cases, noise=noise_cases,
                 chain=chain_cases)
_BUILT = {}


def _family(name):
    def get():
        if name not in _BUILT:
            _BUILT[name] = _BUILDERS[name]()
        return _BUILT[name]
    return get


FAMILIES = {name: _family(name) for name in _BUILDERS}
